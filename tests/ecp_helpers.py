"""Shared by test_ecp_cpu.py and test_gpu_ecp.py: a plain-numpy model of `ds_ecp_energy` (csrc/ds_ecp.h) --
the minimum image, the radial functions, the Legendre polynomials, the two point sets, the rotation replayed from the Philox
model of sampler_helpers, the pair list, the displaced configurations, the ratios of the float64 CPU oracle and the energy
formed from ratios -- with a synthetic species set and the fixture cases of the GPU tests.

The minimum image and the radial functions restate the kernel's arithmetic operation by operation (no fused multiply-adds, the
inverse of the cell by the cofactor formula the library uses), so r is bit-identical and a radial term differs by exp alone."""
import functools

import numpy as np
import torch

import sampler_helpers as sh

EPS = 2.0 ** -52
SEED, OFFSET = 20241019, 3
ROTATION_STREAM_OFFSET = 1 << 61       # stream 4 = stream number 0 with bit 29 of the fourth counter word set (the header)


# ------------------------------------------------------------------------------------------------------ geometry
def inv3(a):
    """Inverse of a 3 x 3 matrix by cofactors, in the operation order of the library's inv3 (csrc/ds_base.h)."""
    a = [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6])
    o = [(a[4] * a[8] - a[5] * a[7]) / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
         (a[5] * a[6] - a[3] * a[8]) / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
         (a[3] * a[7] - a[4] * a[6]) / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det]
    return np.asarray(o, dtype=np.float64).reshape(3, 3)


def heights(a):
    """height c = 1 / ||column c of inv(a)||."""
    return 1.0 / np.linalg.norm(inv3(a), axis=0)


def min_image(x, atoms, a):
    """x (B, 3N), atoms (A, 3), a (3, 3) rows = lattice vectors -> (r (B, N, A), d (B, N, A, 3), dhat (B, N, A, 3)):
    f = (r_i - R_I) . inv(a);  f <- f - floor(f + 1/2);  d = f . a;  r = |d|;  dhat = d / r (z if r = 0)."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    ai = inv3(a)
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    p = x.reshape(B, -1, 1, 3) - np.asarray(atoms, dtype=np.float64).reshape(1, 1, -1, 3)
    f = np.stack([(p[..., 0] * ai[0, c] + p[..., 1] * ai[1, c]) + p[..., 2] * ai[2, c] for c in range(3)], axis=-1)
    f = f - np.floor(f + 0.5)
    d = np.stack([(f[..., 0] * a[0, c] + f[..., 1] * a[1, c]) + f[..., 2] * a[2, c] for c in range(3)], axis=-1)
    r = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    with np.errstate(divide='ignore', invalid='ignore'):
        dhat = np.where(r[..., None] > 0, d / r[..., None], np.asarray([0.0, 0.0, 1.0]))
    return r, d, dhat


def radial_terms(terms, r):
    """The terms c_k r^(n_k - 2) exp(-zeta_k r^2) of a table [(n, zeta, c), ...] at r (any shape) -> (K, ...)."""
    r = np.asarray(r, dtype=np.float64)
    r2 = r * r
    out = []
    for n, z, c in terms:
        pw = (1.0 / r2, 1.0 / r, np.ones_like(r), r, r2)[int(n)]
        out.append((c * pw) * np.exp(-(z * r2)))
    return np.asarray(out).reshape((len(terms),) + r.shape)


def radial(terms, r):
    """v(r), the terms added in table order."""
    v = np.zeros_like(np.asarray(r, dtype=np.float64))
    for t in radial_terms(terms, r):
        v = v + t
    return v


def legendre(l, t):
    t = np.asarray(t, dtype=np.float64)
    return (np.ones_like(t), t, 0.5 * (3.0 * t * t - 1.0), 0.5 * (5.0 * t ** 3 - 3.0 * t))[l]


def points(n_quad):
    """The unrotated points of the two rules, restated from the text of DESIGN.md section 18 (not imported from the package)."""
    if n_quad == 6:
        return np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    assert n_quad == 12
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    n = np.sqrt(1.0 + phi * phi)
    out = []
    for form in range(3):
        for s1, s2 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            out.append([(0.0, s1, s2 * phi), (s1, s2 * phi, 0.0), (s2 * phi, 0.0, s1)][form])
    return np.asarray(out, dtype=np.float64) / n


# ------------------------------------------------------------------------------------------------------ rotation
def quaternion_matrix(x, y, z, w):
    """The standard rotation matrix of a unit quaternion (x, y, z, w) -> (..., 3, 3), its factor 2 taken as 2 / |quaternion|^2 as the
    kernel does (the rounding of the norm then does not enter the orthogonality)."""
    s = 2.0 / ((x * x + y * y) + (z * z + w * w))
    rows = [[1.0 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
            [s * (x * y + z * w), 1.0 - s * (x * x + z * z), s * (y * z - x * w)],
            [s * (x * z - y * w), s * (y * z + x * w), 1.0 - s * (x * x + y * y)]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def replay_rotations(seed, offset, B):
    """Rot_w (B, 3, 3) of a call: Philox stream 4, block A at index 2w, block B at index 2w + 1, counter `offset`, step 0;
    u1 = u53_co(A0, A1), u2 = u53_co(A2, A3), u3 = u53_co(B0, B1); Shoemake's quaternion."""
    w = np.arange(B, dtype=np.uint64)
    two = np.uint64(2)
    off = (int(offset) + ROTATION_STREAM_OFFSET) & (2 ** 64 - 1)
    A = sh.philox_block(seed, off, 0, two * w, 0)
    Bk = sh.philox_block(seed, off, 0, two * w + np.uint64(1), 0)
    u1, u2, u3 = sh.u53_co(A[0], A[1]), sh.u53_co(A[2], A[3]), sh.u53_co(Bk[0], Bk[1])
    ra, rb = np.sqrt(1.0 - u1), np.sqrt(u1)
    return quaternion_matrix(ra * np.sin(2.0 * np.pi * u2), ra * np.cos(2.0 * np.pi * u2), rb * np.sin(2.0 * np.pi * u3),
                             rb * np.cos(2.0 * np.pi * u3))


def rotated_points(rot, n_quad):
    """U_q = Rot_w u_q -> (B, n_quad, 3)."""
    return np.einsum('wcj,qj->wqc', np.asarray(rot, dtype=np.float64), points(n_quad))


# ------------------------------------------------------------------------------------------------------ the model
def local_energy(ecp, x):
    """E_loc (B,) in (i, I) order with the terms of a pair in table order, sum |term| (B,) and the number of terms added (B,)."""
    r, _, _ = min_image(x, ecp.atoms, ecp.a)
    B, N, A = r.shape
    e, mag, cnt = np.zeros(B), np.zeros(B), np.zeros(B, dtype=int)
    for w in range(B):
        for i in range(N):
            for I in range(A):
                s = int(ecp.atom_species[I])
                if r[w, i, I] < ecp.r_cut_loc[s]:
                    t = radial_terms(ecp.local[s], r[w, i, I])
                    v = 0.0
                    for tk in t:
                        v = v + float(tk)
                    e[w] += v
                    mag[w] += np.abs(t).sum()
                    cnt[w] += len(t)
    return e, mag, cnt


def pair_list(ecp, x):
    """The pairs inside r_cut_nl in (w, i, I) order: dict w, i, I (P,), r (P,), d, dhat (P, 3), counts (B,); a walker with a
    non-finite coordinate has none."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        r, d, dh = min_image(x, ecp.atoms, ecp.a)
    B, N, A = r.shape
    sp = np.asarray(ecp.atom_species)
    nl = np.asarray([len(c) for c in ecp.channels])
    with np.errstate(invalid='ignore'):
        inside = (r < ecp.r_cut_nl[sp][None, None, :]) & (nl[sp] > 0)[None, None, :] & np.isfinite(x).all(axis=1)[:, None, None]
    w, i, I = np.nonzero(inside)
    return dict(w=w, i=i, I=I, r=r[w, i, I], d=d[w, i, I], dhat=dh[w, i, I], counts=inside.sum(axis=(1, 2)))


def displaced(x, pl, rot, n_quad):
    """R' (P n_quad, 3N): configuration pair * n_quad + q is the walker of the pair with r_i replaced by r_i - d + r U_q."""
    x = np.asarray(x, dtype=np.float64)
    U = rotated_points(rot, n_quad)
    P = len(pl['w'])
    xd = np.repeat(x[pl['w']].reshape(P, 1, -1, 3), n_quad, axis=1).copy()
    xd[np.arange(P), :, pl['i']] += -pl['d'][:, None, :] + pl['r'][:, None, None] * U[pl['w']]
    return xd.reshape(P * n_quad, -1)


def weights(ecp, pl, rot, n_quad):
    """W_iIq / N_q (P, n_quad) = sum_l (2l + 1) v_l(r) P_l(U_q . dhat) / N_q."""
    U = rotated_points(rot, n_quad)[pl['w']]
    t = np.einsum('pqc,pc->pq', U, pl['dhat'])
    W = np.zeros_like(t)
    for p in range(len(t)):
        s = int(ecp.atom_species[pl['I'][p]])
        for l, terms in enumerate(ecp.channels[s]):
            W[p] += (2 * l + 1) * radial(terms, pl['r'][p]) * legendre(l, t[p])
    return W / n_quad


def oracle_ratios(o, x, xd, w):
    """q (n_cfg,) complex128 from the oracle `o` (sampler_helpers.Oracle) as onebody_helpers.oracle_ratios forms them:
    exp(log psi(R') - log psi(R)) with the complex eval_logdet; configuration c belongs to walker w[c]."""
    if len(xd) == 0:
        return np.zeros(0, dtype=np.complex128)
    l0, l1 = o.logdet(x), o.logdet(xd)
    return np.exp((l1 - l0[torch.as_tensor(w)]).to(torch.complex128).numpy())


def energy(q, Wn, pl, B, n_quad):
    """E_nl (B,) complex from ratios q (P n_quad,) and the weights W / N_q (P, n_quad), and per walker the sum over its
    configurations of |W / N_q| max(1, |q|) (what a tolerance per ratio scales to)."""
    t = Wn * q.reshape(-1, n_quad)
    scale = np.abs(Wn) * np.maximum(1.0, np.abs(q.reshape(-1, n_quad)))
    e, s = np.zeros(B, dtype=np.complex128), np.zeros(B)
    np.add.at(e, pl['w'], t.sum(axis=1))
    np.add.at(s, pl['w'], scale.sum(axis=1))
    return e, s


# ------------------------------------------------------------------------------------------------------ species and cases
# Synthetic species: l = 0, 1, 2 channels, a local part with an n = 1 and an n = 3 term, n = 0 and n = 4 terms among the channels.
SPECIES_A = dict(local=[(1, 1.2, -1.5), (3, 0.9, 0.7), (2, 1.5, 2.0)],
                 channels=[[(2, 1.1, 3.0), (4, 0.8, -0.6)], [(2, 0.9, -1.2), (0, 1.7, 0.05)], [(2, 0.7, 0.8)]])
SPECIES_B = dict(local=[(1, 0.8, -0.6), (3, 1.3, 0.4)],
                 channels=[[(2, 0.6, 1.5)], [(2, 1.0, -0.7), (1, 1.4, 0.3)], [(4, 1.2, 0.9), (2, 0.5, -0.2)]])

# case -> (non-local cutoff of every species in Bohr, pairs per fixture walker); counted on the CPU.  The smallest heights are
# 4.364 Bohr (LiH cells), 9.158 (bcc-Li), 4.579 (li_polarized).  The local cutoff is 0.8 of the non-local one.
CASES = {
    'lih': (2.18, [3, 5, 3, 4, 4, 3]),
    'lih_twist': (1.746, [2, 2, 0, 2]),
    'bcc_li': (2.747, [15, 14, 16, 15]),
    # (half the smallest height of this cell is 2.28952 Bohr: the cutoff is that, cut to four digits; the nearest pair distance is
    # 0.04 Bohr away, so the counts are those of any cutoff in 2.25..2.33)
    'li_polarized': (2.2895, [0, 1, 2]),
    'lih_fulldet': (2.18, [2, 2, 2]),
}
# The large cells, on their first two fixture walkers (the oracle costs 4-23 ms per configuration there); kept apart from CASES,
# which the tests of the small cells walk with every fixture walker.  Half the smallest height is 3.89 Bohr (diamond) and 6.87
# (bcc_li_333); the nearest distance to a cutoff is 2.2e-3 and 4.7e-3 Bohr.
LARGE_CASES = {
    'diamond': (1.2, [17, 18]),
    'bcc_li_333': (1.2, [5, 9]),
}
LARGE_WALKERS = 2
LOCAL_FRACTION = 0.8
CUTOFF_MARGIN = 1e-6


def make_ecp(cell, r_cut, n_quad=12):
    """The synthetic potential on `cell`: atoms alternate between species A and B, both with the cutoffs (0.8 r_cut, r_cut);
    with n_quad = 6 the channels stop at l = 1."""
    from deepsolid_amd.pseudopotential import SemiLocalECP
    n_l = 3 if n_quad == 12 else 2
    species = [dict(local=s['local'], channels=s['channels'][:n_l], r_cut_loc=LOCAL_FRACTION * r_cut, r_cut_nl=r_cut)
               for s in (SPECIES_A, SPECIES_B)]
    n_atoms = np.asarray(cell.atom_coords()).reshape(-1, 3).shape[0]
    return SemiLocalECP(cell, species, [I % 2 for I in range(n_atoms)], n_quad=n_quad)


@functools.lru_cache(maxsize=None)
def fixture(name, n_quad=12, f32=False, n_walkers=None):
    """Case `name` on its fixture walkers (the first `n_walkers` of them; rounded to float32 with `f32`): dict x, ecp, cell, pairs
    (the pair list).  Asserts the pair counts of CASES / LARGE_CASES and that no pair lies within 1e-6 Bohr of a cutoff, so that
    none can flip between model and kernel."""
    fx, cell, _, _, _ = sh.case(name)
    r_cut, counts = CASES[name] if name in CASES else LARGE_CASES[name]
    x = np.asarray(fx['x'], dtype=np.float64)[:n_walkers]
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    ecp = make_ecp(cell, r_cut, n_quad)
    assert r_cut <= 0.5 * heights(cell.a).min()
    r, _, _ = min_image(x, ecp.atoms, ecp.a)
    for rc in (r_cut, LOCAL_FRACTION * r_cut):
        assert np.abs(r - rc).min() > CUTOFF_MARGIN, (name, rc, np.abs(r - rc).min())
    pl = pair_list(ecp, x)
    assert pl['counts'].tolist() == counts, (name, pl['counts'].tolist())
    x.setflags(write=False)
    return dict(x=x, ecp=ecp, cell=cell, pairs=pl)


@functools.lru_cache(maxsize=None)
def reference(name, n_quad=12, f32=False, n_walkers=None):
    """Oracle side of case `name` with the rotations of (SEED, OFFSET), computed once: the fixture's entries plus rot (B, 3, 3),
    xd, q (oracle ratios), Wn (weights / N_q), e_loc, e_loc_mag, e_loc_terms, e_nl, e_nl_scale."""
    fx = dict(fixture(name, n_quad, f32, n_walkers))
    x, ecp, pl = fx['x'], fx['ecp'], fx['pairs']
    B = len(x)
    rot = replay_rotations(SEED, OFFSET, B)
    xd = displaced(x, pl, rot, n_quad)
    q = oracle_ratios(sh.oracle(name, f32), x, xd, np.repeat(pl['w'], n_quad))
    Wn = weights(ecp, pl, rot, n_quad)
    e_loc, mag, cnt = local_energy(ecp, x)
    e_nl, scale = energy(q, Wn, pl, B, n_quad)
    for v in (rot, q, Wn, e_loc, e_nl):
        v.setflags(write=False)
    fx.update(rot=rot, xd=xd, q=q, Wn=Wn, e_loc=e_loc, e_loc_mag=mag, e_loc_terms=cnt, e_nl=e_nl, e_nl_scale=scale)
    return fx


# ------------------------------------------------------------------------------------------------------ plane waves
def plane_wave_config_ratios(x, pl, rot, n_quad, pw_klist, nelec):
    """q (P n_quad,) of the plane-wave determinant of onebody_helpers for the configurations of `displaced`, from positions alone."""
    import onebody_helpers as oh
    U = rotated_points(rot, n_quad)
    q = np.zeros((len(pl['w']), n_quad), dtype=np.complex128)
    for p, (w, i) in enumerate(zip(pl['w'], pl['i'])):
        s = (-pl['d'][p][None, :] + pl['r'][p] * U[w])[None]                      # (1, n_quad, 3): all samples move electron i
        for k in range(n_quad):
            q[p, k] = oh.plane_wave_ratios(x[w:w + 1], s[:, k:k + 1], int(i), pw_klist, nelec)[0, 0]
    return q.reshape(-1)


def plane_wave_exact_terms(x, pl, ecp, pw_klist, nelec):
    """The exact angular integral of every pair of the plane-wave determinant, (P,) complex:
        sum_l (2l + 1) v_l(r) sum_j [i^l j_l(k_j r) P_l(khat_j . dhat)] exp(-i k_j . d) phi_j(r_e) (M^-1)_{je}
    from  int dOmega / (4 pi) P_l(U . dhat) exp(i k . r U) = i^l j_l(k r) P_l(khat . dhat)  and the ratio of a one-electron move by
    s = -d + r U, q = sum_j exp(i k_j . s) phi_j(r_e) (M^-1)_{je}.  Also the a-priori quadrature bound of every pair for a rule of
    degree D, as a function D -> (P,): the plane wave is sum_L (2L + 1) i^L j_L(kr) P_L(khat . U); the rule integrates the products
    P_l P_L of degree l + L <= D exactly, every other product has the exact integral 0 (L != l) and a rule value of modulus <= 1, so
    the error of channel l is at most sum_{L > D - l} (2L + 1) |j_L(kr)|."""
    from scipy.special import spherical_jn
    x = np.asarray(x, dtype=np.float64)
    N = sum(nelec)
    out = np.zeros(len(pl['w']), dtype=np.complex128)
    per_l = []
    for p, (w, i, I) in enumerate(zip(pl['w'], pl['i'], pl['I'])):
        sp = 0 if i < nelec[0] else 1
        lo = 0 if sp == 0 else nelec[0]
        k = np.asarray(pw_klist[sp], dtype=np.float64)
        rr = x[w].reshape(N, 3)
        mat = np.exp(1j * rr[lo:lo + nelec[sp]] @ k.T)
        inv = np.linalg.inv(mat)
        coef = np.exp(-1j * k @ pl['d'][p]) * mat[i - lo] * inv[:, i - lo]           # per orbital j
        kn = np.linalg.norm(k, axis=1)
        r = pl['r'][p]
        s = int(ecp.atom_species[I])
        rows = []
        for l, terms in enumerate(ecp.channels[s]):
            v = (2 * l + 1) * radial(terms, r)
            with np.errstate(invalid='ignore', divide='ignore'):
                ct = np.where(kn > 0, (k @ pl['dhat'][p]) / np.where(kn > 0, kn, 1.0), 0.0)
            ang = (1j ** l) * spherical_jn(l, kn * r) * np.where(kn > 0, legendre(l, ct), 1.0 if l == 0 else 0.0)
            out[p] += v * np.sum(ang * coef)
            rows.append((l, abs(v), np.abs(coef), kn * r))
        per_l.append(rows)

    def bound(degree):
        b = np.zeros(len(per_l))
        for p, rows in enumerate(per_l):
            for l, v, c, kr in rows:
                tail = sum((2 * L + 1) * np.abs(spherical_jn(L, kr)) for L in range(degree - l + 1, degree - l + 40))
                b[p] += v * np.sum(c * tail)
        return b
    return out, bound
