"""Shared by test_dmc_parts_cpu.py, test_gpu_dmc_parts.py and test_gpu_dmc_ecp.py: the pieces of one `ds_dmc_step` (csrc/ds_dmc.h)
restated in plain numpy, float64 throughout; with a float32 system (`dtype=np.float32`) what the kernels form in `T` is formed in
np.float32.  No oracle: every function takes arrays, so a GPU test can feed it the device's own values on any cell, dtype and B --
the sums of k_dmc_stats in the device's order (bit for bit), the proposal of k_dmc_propose, the log ratio A of k_dmc_accept with an
a-priori bound on its rounding, and the weight formula."""
import numpy as np

GROUP = 256                       # DMC_GROUP of csrc/ds_dmc.h
EPS = 2.0 ** -52
EPS32 = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------- the sums
def tree_rows(values):
    """The sum over axis 0 of `values` (B,) or (B, k) as k_dmc_stats / k_dmc_stats_final form it: per group of 256 consecutive
    walkers, padded with zeros, thread t adds the value of thread t + s for s = 128, 64, ..., 1; the group sums are then added
    sequentially, in group order, onto 0.  Every addition is one rounded float64 addition: this is the device's result bit for bit."""
    v = np.asarray(values, dtype=np.float64)
    flat = v.reshape(len(v), -1)
    total = np.zeros(flat.shape[1])
    with np.errstate(invalid='ignore', over='ignore'):
        for g0 in range(0, len(flat), GROUP):
            rows = flat[g0:g0 + GROUP]
            sh = np.zeros((GROUP, flat.shape[1]))
            sh[:len(rows)] = rows
            s = GROUP // 2
            while s > 0:
                sh[:s] = sh[:s] + sh[s:2 * s]
                s //= 2
            total = total + sh[0]
    return total[0] if v.ndim == 1 else total


def clip(e, e_ref, e_cut):
    """dmc_clip -> (clipped energy, flag): d = e - e_ref; d > e_cut gives e_ref + e_cut, d < -e_cut gives e_ref - e_cut, anything else
    (a NaN included) e itself, unflagged; e_cut <= 0 clips nothing."""
    e = np.asarray(e, dtype=np.float64)
    if not e_cut > 0.0:
        return e.copy(), np.zeros(e.shape, bool)
    with np.errstate(invalid='ignore'):
        d = e - e_ref
        hi, lo = d > e_cut, d < -e_cut
    return np.where(hi, e_ref + e_cut, np.where(lo, e_ref - e_cut, e)), hi | lo


def stats_from_state(weight, eloc, e_ref, e_cut):
    """-> (columns 0, 1, 2, 7 of the out_stats row of a step that left this state (before a comb), the clipped count of column 5).
    The summands are w, w e, (w e) e and w w, the energy terms dropped where w == 0 (the energy may be NaN there), added by
    `tree_rows`; the count is over all walkers, those of weight 0 included."""
    w, e = np.asarray(weight, dtype=np.float64), np.asarray(eloc, dtype=np.float64)
    live = w != 0.0
    with np.errstate(invalid='ignore', over='ignore'):
        we = np.where(live, w * e, 0.0)
        wee = np.where(live, (w * e) * e, 0.0)
        cols = tree_rows(np.stack([w, we, wee, w * w], axis=1))
    return cols, int(clip(e, e_ref, e_cut)[1].sum())


def ecp_stats_from_state(weight, epp):
    """The out_ecp_stats row of a step that left this state (before a comb): sum w (E_loc, Re E_nl, Im E_nl) over the walkers of
    non-zero weight, added by `tree_rows`."""
    w, epp = np.asarray(weight, dtype=np.float64), np.asarray(epp, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return tree_rows(np.where((w != 0.0)[:, None], w[:, None] * epp, 0.0))


# ------------------------------------------------------------------------------------------------------------ the move
def limiter(v, tau, dtype=np.float64):
    """dmc_limiter per electron, in `dtype`: f = 2 / (1 + sqrt(1 + 2 |v|^2 tau)) -> (B, N, 1)."""
    T = np.dtype(dtype).type
    v3 = np.asarray(v, dtype=dtype).reshape(len(v), -1, 3)
    v2 = v3[..., 0] * v3[..., 0] + v3[..., 1] * v3[..., 1] + v3[..., 2] * v3[..., 2]
    with np.errstate(invalid='ignore', over='ignore'):
        return (T(2) / (T(1) + np.sqrt(T(1) + T(2) * v2 * T(tau))))[..., None]


def proposal(cell, x, drift, chi, tau, dtype=np.float64):
    """k_dmc_propose: wrap(x + tau (f v) + sqrt(tau) chi) with f of `limiter`, formed in `dtype` -> (B, 3N) float64."""
    T = np.dtype(dtype).type
    x, v, chi = (np.asarray(t, dtype=dtype) for t in (x, drift, chi))
    B = len(x)
    f = limiter(v, tau, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        r = x.reshape(B, -1, 3) + T(tau) * (f * v.reshape(B, -1, 3)) + T(np.sqrt(tau)) * chi.reshape(B, -1, 3)
        a64 = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
        a, ainv = a64.astype(dtype), np.linalg.inv(a64).astype(dtype)
        fr = r @ ainv
        out = (fr - np.floor(fr)) @ a
    return out.reshape(B, -1).astype(np.float64)


def min_image_distance(cell, x1, x2):
    """max over the coordinates of |x1 - x2| up to lattice vectors, per walker (a proposal on a cell face may be wrapped to either
    side)."""
    a = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    d = (np.asarray(x1, dtype=np.float64) - np.asarray(x2, dtype=np.float64)).reshape(len(x1), -1, 3)
    f = d @ np.linalg.inv(a)
    return np.abs((f - np.round(f)) @ a).reshape(len(x1), -1).max(1)


def longest_cell_vector(cell):
    return float(np.linalg.norm(np.asarray(cell.a, dtype=np.float64).reshape(3, 3), axis=1).max())


def log_ratio(la, la2, drift, drift2, chi, tau, dtype=np.float64):
    """The A of dmc_decide (k_dmc_accept, k_dmc_tm_decide) = 2 (la2 - la) + 0.5 (|chi|^2 - |chi + sqrt(tau) (f1 v1 + f2 v2)|^2) per walker -> (A (B,), tol_A (B,)).
    The limiter and the products f v are formed in `dtype`, everything else in float64.

    tol_A bounds |A_device - A_host| a priori.  Float64 part: the two sums have 3N terms each, added in another order than here and
    with the products fused or not (each term's rounding is at most a few 2^-53 of it, an accumulation of 3N terms another 3N 2^-53
    of the sum of their moduli), and the last line is four more operations on s1, s2, 2 la and 2 la2:
        (3N + 8) 2^-52 (s1 + s2 + 2 |la| + 2 |la2|).
    Float32 part: f and f v are formed in float32 with contraction allowed, so the host cannot repeat them bit for bit; each f v is
    then off by at most 8 2^-23 |f v| (the squares, their sum, the square root, the division and the product, each half an ulp, with
    room), which moves bk_c by sqrt(tau) times that and bk_c^2 / 2 by |bk_c| times that:
        8 2^-23 sqrt(tau) sum_c |bk_c| (|f1 v1_c| + |f2 v2_c|)."""
    B = len(chi)
    g1, g2 = np.asarray(drift, dtype=dtype).reshape(B, -1, 3), np.asarray(drift2, dtype=dtype).reshape(B, -1, 3)
    n3 = g1.shape[1] * 3
    ch = np.asarray(chi, dtype=dtype).astype(np.float64).reshape(B, n3)
    la, la2 = np.asarray(la, dtype=np.float64), np.asarray(la2, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        p1 = (limiter(g1, tau, dtype) * g1).astype(np.float64).reshape(B, n3)
        p2 = (limiter(g2, tau, dtype) * g2).astype(np.float64).reshape(B, n3)
        bk = ch + np.sqrt(np.float64(tau)) * (p1 + p2)
        s1, s2 = (ch * ch).sum(1), (bk * bk).sum(1)
        A = 2.0 * (la2 - la) + 0.5 * (s1 - s2)
        tol = (n3 + 8) * EPS * (s1 + s2 + 2.0 * np.abs(la) + 2.0 * np.abs(la2))
        if np.dtype(dtype) == np.float32:
            tol = tol + 8.0 * EPS32 * np.sqrt(tau) * (np.abs(bk) * (np.abs(p1) + np.abs(p2))).sum(1)
    return A, tol


def weights_after(w, e_new, e_old, tau_eff, e_trial, e_ref, e_cut):
    """The weight formula of k_dmc_accept: w exp(-tau_eff ((clip(e_new) + clip(e_old)) / 2 - e_trial)); a result that is not finite
    is 0."""
    with np.errstate(invalid='ignore', over='ignore'):
        cn, co = clip(e_new, e_ref, e_cut)[0], clip(e_old, e_ref, e_cut)[0]
        wn = np.asarray(w, dtype=np.float64) * np.exp(-tau_eff * (0.5 * (cn + co) - e_trial))
    return np.where(np.isfinite(wn), wn, 0.0)
