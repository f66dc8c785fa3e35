"""Shared by test_ecp_force_cpu.py and test_gpu_ecp_force.py: a plain-numpy model of `ds_ecp_forces` (csrc/ds_ecp_force.h, DESIGN.md
section 25) on top of ecp_helpers.py -- the derivative of a radial function, the local force in the kernel's order, the force term of
every quadrature configuration from the oracle's ratios and walker gradients, the sums per walker and ion, the tolerance scale per
(walker, ion), and the central differences of the ENERGY model of ecp_helpers.py in an ion position, with their Richardson bound.

The radial derivative restates the kernel's arithmetic operation by operation, so a term differs by exp alone."""
import copy
import functools

import numpy as np
import torch

import ecp_helpers as eh
import sampler_helpers as sh

EPS = eh.EPS
H = 1e-4                               # step of the central differences in an ion position, Bohr
# float32 walker gradient: max |g_f32-oracle - g_f64-oracle| over the 264 displaced configurations of 'lih' (N_q = 12, walkers rounded
# to float32, (SEED, OFFSET) of ecp_helpers), measured on the CPU: 1.007e-03 (real half 9.5e-04, imaginary half 6.9e-04) at max |g| = 43.8; granted 4 x
GRAD_LOSS_F32 = 1.007e-3
TOL_G_F32 = 4 * GRAD_LOSS_F32


# ------------------------------------------------------------------------------------------------------ radial derivative
def radial_deriv_terms(terms, r):
    """The terms c_k [(n_k - 2) r^(n_k - 3) - 2 zeta_k r^(n_k - 1)] exp(-zeta_k r^2) of v'(r) for a table [(n, zeta, c), ...] at r
    (any shape) -> (terms (K, ...), magnitudes (K, ...) = |c_k| (|n_k - 2| r^(n_k - 3) + 2 zeta_k r^(n_k - 1)) exp(..))."""
    r = np.asarray(r, dtype=np.float64)
    r2 = r * r
    r3 = r2 * r
    one = np.ones_like(r)
    out, mag = [], []
    for n, z, c in terms:
        lo = (1.0 / r3, 1.0 / r2, 1.0 / r, one, r)[int(n)]
        hi = (1.0 / r, one, r, r2, r3)[int(n)]
        e = np.exp(-(z * r2))
        out.append((c * (float(int(n) - 2) * lo - (2.0 * z) * hi)) * e)
        mag.append(abs(c) * (abs(int(n) - 2) * lo + (2.0 * z) * hi) * e)
    shape = (len(terms),) + r.shape
    return np.asarray(out).reshape(shape), np.asarray(mag).reshape(shape)


def radial_deriv(terms, r):
    """v'(r), the terms added in table order."""
    v = np.zeros_like(np.asarray(r, dtype=np.float64))
    for t in radial_deriv_terms(terms, r)[0]:
        v = v + t
    return v


def legendre_deriv(l, t):
    t = np.asarray(t, dtype=np.float64)
    return (np.zeros_like(t), np.ones_like(t), 3.0 * t, 0.5 * (15.0 * t * t - 3.0))[l]


# ------------------------------------------------------------------------------------------------------ the model
def local_force(ecp, x):
    """F^loc (B, A, 3): per ion the electrons added in order; sum |term| (B, A) and the number of terms added (B, A) (what the
    float64 bound of test_gpu_ecp.py for E_loc takes: (8 + terms) 2^-52 sum |term|; |dhat_c| <= 1 is not used)."""
    r, _, dh = eh.min_image(x, ecp.atoms, ecp.a)
    B, N, A = r.shape
    f, mag, cnt = np.zeros((B, A, 3)), np.zeros((B, A)), np.zeros((B, A), dtype=int)
    for w in range(B):
        for I in range(A):
            s = int(ecp.atom_species[I])
            for i in range(N):
                if r[w, i, I] < ecp.r_cut_loc[s]:
                    t, m = radial_deriv_terms(ecp.local[s], r[w, i, I])
                    v = 0.0
                    for tk in t:
                        v = v + float(tk)
                    f[w, I] = f[w, I] + v * dh[w, i, I]
                    mag[w, I] += m.sum()
                    cnt[w, I] += len(t)
    return f, mag, cnt


def force_terms(ecp, pl, rot, n_quad, q, g):
    """Per configuration the complex 3-vector (1 / N_q) rho_q { D_q - W_q J g_q } (P, n_quad, 3) from the ratios q (P n_quad,) and
    the gradient g (P n_quad, 3) of the pair's electron at R'_q; also D (P, n_quad, 3), W (P, n_quad) and J g (P, n_quad, 3)."""
    P = len(pl['w'])
    U = eh.rotated_points(rot, n_quad)[pl['w']].reshape(P, n_quad, 3)
    dh, r = pl['dhat'][:, None, :], pl['r'][:, None]
    t = np.einsum('pqc,pc->pq', U, pl['dhat'])
    W, radial, angular = np.zeros_like(t), np.zeros_like(t), np.zeros_like(t)
    for p in range(P):
        s = int(ecp.atom_species[pl['I'][p]])
        for l, terms in enumerate(ecp.channels[s]):
            v, dv = eh.radial(terms, pl['r'][p]), radial_deriv(terms, pl['r'][p])
            W[p] += (2 * l + 1) * v * eh.legendre(l, t[p])
            radial[p] += (2 * l + 1) * dv * eh.legendre(l, t[p])
            angular[p] += (2 * l + 1) * v * legendre_deriv(l, t[p])
    D = radial[..., None] * dh + (angular / r)[..., None] * (U - t[..., None] * dh)
    g = np.asarray(g, dtype=np.complex128).reshape(P, n_quad, 3)
    Jg = g - np.einsum('pqc,pqc->pq', g, U)[..., None] * dh
    rho = np.asarray(q, dtype=np.complex128).reshape(P, n_quad, 1)
    return rho * (D - W[..., None] * Jg) / n_quad, D, W, Jg


def nonlocal_force(T, pl, B, A):
    """F^nl (B, A, 3) complex: the terms (P, n_quad, 3) added per (walker, ion)."""
    f = np.zeros((B, A, 3), dtype=np.complex128)
    np.add.at(f, (pl['w'], pl['I']), T.sum(axis=1))
    return f


def nonlocal_scale(pl, B, A, n_quad, q, D, W, Jg, tol_q, tol_g):
    """The bound on |F^nl - model| per (walker, ion), the same for the three components: the sum over the ion's configurations of
    (1 / N_q) [ tol_q max(1, |rho|) (|D_q| + |W_q| |J g_q|) + 2 |W_q| |rho| tol_g ], |.| of a vector its Euclidean norm."""
    rho = np.abs(np.asarray(q).reshape(-1, n_quad))
    per = (tol_q * np.maximum(1.0, rho) * (np.linalg.norm(D, axis=-1) + np.abs(W) * np.linalg.norm(Jg, axis=-1))
           + 2.0 * np.abs(W) * rho * tol_g) / n_quad
    s = np.zeros((B, A))
    np.add.at(s, (pl['w'], pl['I']), per.sum(axis=1))
    return s


def pair_gradients(o, xd, pl, n_quad):
    """g (P n_quad, 3) complex: the components of the pair's electron of the oracle's walker gradient at the displaced rows."""
    if len(xd) == 0:
        return np.zeros((0, 3), dtype=np.complex128), np.zeros((0, xd.shape[1] if xd.ndim == 2 else 0), dtype=np.complex128)
    g = o.value_and_grad(xd)[1].to(dtype=torch.complex128).numpy()
    i = np.repeat(pl['i'], n_quad)
    return g.reshape(len(xd), -1, 3)[np.arange(len(xd)), i], g


@functools.lru_cache(maxsize=None)
def reference(name, n_quad=12, f32=False, n_walkers=None):
    """ecp_helpers.reference(name, n_quad, f32) -- cut to its first `n_walkers` walkers and their pairs, if given -- plus the force
    model: g (P n_quad, 3) and g_all (the whole gradient at the displaced rows, what the gradient tolerance is taken from), T, D,
    W, Jg, f_loc, f_loc_mag, f_loc_terms, f_nl (B, A, 3)."""
    ref = dict(eh.reference(name, n_quad, f32))
    if n_walkers is not None:
        keep = ref['pairs']['w'] < n_walkers
        cfg = np.repeat(keep, n_quad)
        ref['pairs'] = {k: (v[:n_walkers] if k == 'counts' else v[keep]) for k, v in ref['pairs'].items()}
        ref.update(xd=ref['xd'][cfg], q=ref['q'][cfg], Wn=ref['Wn'][keep])
        for k in ('x', 'rot', 'e_loc', 'e_loc_mag', 'e_loc_terms', 'e_nl', 'e_nl_scale'):
            ref[k] = ref[k][:n_walkers]
    ecp, pl, x = ref['ecp'], ref['pairs'], ref['x']
    B, A = len(x), len(ecp.atoms)
    g, g_all = pair_gradients(sh.oracle(name, f32), ref['xd'], pl, n_quad)
    T, D, W, Jg = force_terms(ecp, pl, ref['rot'], n_quad, ref['q'], g)
    f_loc, mag, cnt = local_force(ecp, x)
    ref.update(g=g, g_all=g_all, T=T, D=D, W=W, Jg=Jg, f_loc=f_loc, f_loc_mag=mag, f_loc_terms=cnt, f_nl=nonlocal_force(T, pl, B, A))
    return ref


# ------------------------------------------------------------------------------------------------------ central differences
def moved(ecp, I, c, delta):
    """A copy of the potential whose descriptor atom I is displaced by delta along axis c (no device tables)."""
    e = copy.copy(ecp)
    e.__dict__.pop('_ds_tables', None)
    e.atoms = np.array(ecp.atoms, dtype=np.float64)
    e.atoms[I, c] += delta
    return e


def assert_no_pair_flips(ecp, x, delta):
    """Every distance is at least 2 |delta| away from both of its cutoffs: no pair can enter or leave under displacements up to
    |delta| of one atom."""
    r, _, _ = eh.min_image(x, ecp.atoms, ecp.a)
    sp = np.asarray(ecp.atom_species)
    for rc in (ecp.r_cut_loc[sp], ecp.r_cut_nl[sp]):
        assert np.abs(r - rc[None, None, :]).min() > 2 * abs(delta), np.abs(r - rc[None, None, :]).min()


def model_energy(ecp, x, rot, n_quad, o, I):
    """E_loc + the part of E_nl that belongs to ion I (B,) complex, from the energy model of ecp_helpers (local_energy, weights,
    energy) with the oracle's ratios; the pairs of the other ions do not depend on R_I."""
    pl = eh.pair_list(ecp, x)
    keep = pl['I'] == I
    sub = {k: (v[keep] if k != 'counts' else v) for k, v in pl.items()}
    xd = eh.displaced(x, sub, rot, n_quad)
    q = eh.oracle_ratios(o, x, xd, np.repeat(sub['w'], n_quad))
    e_nl, _ = eh.energy(q, eh.weights(ecp, sub, rot, n_quad), sub, len(x), n_quad)
    return eh.local_energy(ecp, x)[0] + e_nl, pl


@functools.lru_cache(maxsize=None)
def energy_differences(name, n_quad=12):
    """Central differences of the energy model in every ion position, psi and the rotations untouched: -> dict d1 = -dE/dR at the
    step H and d2 at 2 H ((B, A, 3) complex), bound (B, A, 3) = 4 |d2 - d1| / 3: four times the Richardson estimate of the h^2
    truncation term of d1."""
    ref = eh.reference(name, n_quad)
    ecp, x, rot = ref['ecp'], ref['x'], ref['rot']
    o = sh.oracle(name)
    B, A = len(x), len(ecp.atoms)
    assert_no_pair_flips(ecp, x, 2 * H)
    d = {1: np.zeros((B, A, 3), dtype=np.complex128), 2: np.zeros((B, A, 3), dtype=np.complex128)}
    for I in range(A):
        for c in range(3):
            for k in (1, 2):
                ep, plp = model_energy(moved(ecp, I, c, k * H), x, rot, n_quad, o, I)
                em, plm = model_energy(moved(ecp, I, c, -k * H), x, rot, n_quad, o, I)
                for pl in (plp, plm):
                    assert all(np.array_equal(pl[key], ref['pairs'][key]) for key in ('w', 'i', 'I'))
                d[k][:, I, c] = -(ep - em) / (2 * k * H)
    return dict(d1=d[1], d2=d[2], bound=4.0 * np.abs(d[2] - d[1]) / 3.0)
