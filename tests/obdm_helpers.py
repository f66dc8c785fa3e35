"""Shared by test_obdm_cpu.py and test_gpu_obdm.py: a plain-numpy model of the one-body density-matrix fold
(`ds_obdm_accumulate`, csrc/ds_obdm.h; conventions in include/deepsolid_hip.h and DESIGN.md section 24) and the made-up bases.

Sample g = w M + m of a call moves electron e = (first_electron + m) % N of walker w; its spin is 0 if e < n_up, else 1.
    dm[s][i][j] += w_s q conj(phi_i(r')) phi_j(r_e),      ov[s][i][j] += w_s conj(phi_i(r')) phi_j(r')
"""
import functools

import numpy as np

import hf_helpers as hh

U = 2.0 ** -53


def sample_electrons(B, M, N, first):
    """-> (walker (B M,), electron (B M,)) of every sample in the library's order g = w M + m."""
    w = np.repeat(np.arange(B), M)
    e = (first + np.tile(np.arange(M), B)) % N
    return w, e


def fold(q, w, phi_new, phi_old, spin, absolute=False):
    """q (P,) complex, w (P,) float or None, phi_new / phi_old (P, Mb) complex: the basis of the sample's spin at r' / r_e (zero
    beyond M_spin), spin (P,) int; a sample with spin < 0 is left out.  -> (dm, ov), each (2, Mb, Mb) complex;
    `absolute`: the sums of the terms' moduli instead (real), for the summation bound."""
    q = np.asarray(q, dtype=np.complex128)
    w = np.ones(q.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    mb = phi_new.shape[1]
    dm = np.zeros((2, mb, mb), dtype=np.float64 if absolute else np.complex128)
    ov = np.zeros_like(dm)
    mod = np.abs if absolute else (lambda v: v)
    for s in range(2):
        k = np.asarray(spin) == s
        if not k.any():
            continue
        a = mod(phi_new[k].conj())
        dm[s] = np.einsum('p,pi,pj->ij', mod(w[k] * q[k]), a, mod(phi_old[k]))
        ov[s] = np.einsum('p,pi,pj->ij', mod(w[k]).astype(dm.dtype), a, mod(phi_new[k]))
    return dm, ov


def bound(P, absolute):
    """16 P 2^-53 sum |term| per entry: the standard bound of a sum of P terms in any order, with room for the few roundings
    inside a term (two complex products)."""
    return 16.0 * P * U * absolute


def det_ratios(Phi, phi_new):
    """Phi (n, n) [electron, orbital], phi_new (n,): the orbitals at a common point r'.  -> q (n,): det with row e replaced by
    phi_new over det Phi, by numpy determinants."""
    d0 = np.linalg.det(Phi)
    q = np.empty(Phi.shape[0], dtype=np.complex128)
    for e in range(Phi.shape[0]):
        m = Phi.copy()
        m[e] = phi_new
        q[e] = np.linalg.det(m) / d0
    return q


def common_point_shifts(x, nelec, points):
    """x (B, N, 3), points (B, 2, 3): the common point r' per (walker, spin).  -> shifts (B, N, 3) with M = N and
    first_electron = 0: sample m moves electron m onto the point of its spin."""
    x = np.asarray(x, dtype=np.float64)
    spin = (np.arange(x.shape[1]) >= nelec[0]).astype(int)
    return np.asarray(points, dtype=np.float64)[:, spin, :] - x


HEX_NOCC = {(5, 4): [[2, 2, 1], [2, 1, 1]], (3, 0): [[1, 1, 1], [0, 0, 0]], (17, 4): [[6, 6, 5], [2, 1, 1]],
            (64, 1): [[22, 21, 21], [1, 0, 0]]}


@functools.lru_cache(maxsize=None)
def hex_basis(norb):
    """`hh.hex_system`'s cell, atoms, shells and k points with `norb` random orbitals per spin (System draws random MO columns, so
    any count is allowed; beyond 18 per k point they are linearly dependent, which the fold does not mind)."""
    if tuple(norb) in ((5, 4), (3, 0)):
        return hh.hex_system(tuple(norb))
    base = hh.hex_system((5, 4))
    return hh.System(base.a, base.atoms, base.shells, base.kpts, HEX_NOCC[tuple(norb)], seed=29)


def sim_cell_of(sysm, S):
    """The supercell S (3, 3 integers) of a System's primitive cell."""
    return np.asarray(S, dtype=np.float64) @ sysm.a
