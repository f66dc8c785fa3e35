"""Shared by test_spin_cpu.py and test_gpu_spin.py: a plain-numpy restatement of what `ds_spin_exchange_ratios` (csrc/ds_spin.h)
proposes, the exchange ratios of the float64 CPU oracle (complex eval_logdet of P_p R and R), the closed form for a determinant of
plane waves, and the plane-wave network whose two spin channels share their k points (the closed-shell singlet whose <S^2> is
known exactly)."""
import functools

import numpy as np
import torch

import onebody_helpers as oh
import sampler_helpers as sh


def pairs(nelec):
    """(P, 2) electrons (i, j) of pair p = i n_dn + (j - n_up), i < n_up <= j."""
    nu, nd = nelec
    p = np.arange(nu * nd)
    return np.stack([p // max(nd, 1), nu + p % max(nd, 1)], axis=1)


def pair_indices(M, nelec, first):
    """Pair taken by sample m of every walker."""
    return (first + np.arange(M)) % (nelec[0] * nelec[1])


def swapped(x, nelec, which=None):
    """x (B, 3N) -> P_p R for every pair, or for the pairs `which` (P,), (B, P, 3N): the positions of electrons i and j exchanged,
    nothing wrapped."""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape[0], x.shape[1] // 3
    pr = pairs(nelec) if which is None else pairs(nelec)[np.asarray(which)]
    P = len(pr)
    xs = np.repeat(x.reshape(B, 1, N, 3), P, axis=1).copy()
    r = x.reshape(B, N, 3)
    xs[:, np.arange(P), pr[:, 0]] = r[:, pr[:, 1]]
    xs[:, np.arange(P), pr[:, 1]] = r[:, pr[:, 0]]
    return xs.reshape(B, P, 3 * N)


def oracle_ratios(o, x, nelec, M, first):
    """q (B, M) complex128 from the oracle `o` (sampler_helpers.Oracle): exp(log psi(P_p R) - log psi(R)) with the complex
    eval_logdet = log|psi| + i arg psi, sample m taking pair (first + m) % P.  Every pair that a sample takes is evaluated once, no
    other.  With a float32 oracle the configurations are rounded to float32 first."""
    taken, where = np.unique(pair_indices(M, nelec, first), return_inverse=True)
    xs = swapped(x, nelec, taken)
    B, P, n3 = xs.shape
    l0 = o.logdet(x)
    l1 = o.logdet(xs.reshape(B * P, n3)).reshape(B, P)
    q = np.exp((l1 - l0[:, None]).to(torch.complex128).numpy())
    return q[:, where]


def plane_wave_pair_ratios(x, pw_klist, nelec):
    """q (B, P) of a determinant of plane waves from positions alone: with M^s_{ek} = phi^s_k(r_e) = exp(i k^s_k . r_e) over the
    electrons and orbitals of spin s,  q_ij = [sum_k phi^up_k(r_j) (M^up^-1)_{ki}] [sum_l phi^dn_l(r_i) (M^dn^-1)_{lj}]:
    row i of the up matrix is evaluated at r_j and row j of the down matrix at r_i."""
    x = np.asarray(x, dtype=np.float64)
    nu, nd = nelec
    B = x.shape[0]
    r = x.reshape(B, nu + nd, 3)
    ku, kd = (np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in pw_klist)
    q = np.zeros((B, nu, nd), dtype=np.complex128)
    for b in range(B):
        inv_u = np.linalg.inv(np.exp(1j * r[b, :nu] @ ku.T))          # [orbital, electron]
        inv_d = np.linalg.inv(np.exp(1j * r[b, nu:] @ kd.T))
        up_at_dn = np.exp(1j * r[b, nu:] @ ku.T) @ inv_u              # [j, i]
        dn_at_up = np.exp(1j * r[b, :nu] @ kd.T) @ inv_d              # [i, j]
        q[b] = up_at_dn.T * dn_at_up
    return q.reshape(B, nu * nd)


def shared_plane_wave_case(cell, klist):
    """`onebody_helpers.plane_wave_case` with the SAME k points in both spin channels: klist (kpts[:n_up], kpts[:n_dn]).  The
    smaller channel's orbitals are a subset of the larger one's, so the state is an eigenstate of S^2 with s = |S_z|.
    -> (klist, net_kw, numpy params)."""
    _, net_kw, params, kpts, _ = oh.plane_wave_case(cell, klist)
    nelec = tuple(int(v) for v in cell.nelec)
    return (kpts[:nelec[0]], kpts[:nelec[1]]), net_kw, params


def small_cell(nelec):
    """The one-atom bcc-Li cell with `nelec` electrons -> (cell, klist)."""
    from deepsolid_amd import systems
    return systems.build('bcc_li', S=1, nelec=tuple(nelec))


def walkers(name):
    """Walkers of a case of sampler_helpers.case: its fixture's, or 5 synthetic ones for the cells without a fixture."""
    from deepsolid_amd import systems
    fx, cell, _, _, _ = sh.case(name)
    return np.asarray(fx['x'], dtype=np.float64) if fx is not None else systems.synthetic_walkers(cell, 5, seed=8)


@functools.lru_cache(maxsize=None)
def reference(name, f32=False):
    """Oracle side of case `name` on its walkers, computed once: dict x, q_all (B, P) (every pair), cell, nelec."""
    _, cell, _, _, _ = sh.case(name)
    x = walkers(name)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    nelec = tuple(int(v) for v in cell.nelec)
    P = nelec[0] * nelec[1]
    q = oracle_ratios(sh.oracle(name, f32), x, nelec, P, 0)
    q.setflags(write=False)
    return dict(x=x, q_all=q, cell=cell, nelec=nelec)


@functools.lru_cache(maxsize=None)
def large_reference(name, M, first_pair, f32=False, n_walkers=2):
    """Oracle side of a large cell on its first `n_walkers` fixture walkers, computed once: only the pairs the M samples from
    `first_pair` take are evaluated.  -> dict x, q (B, M), cell, nelec."""
    fx, cell, _, _, _ = sh.case(name)
    x = np.asarray(fx['x'], dtype=np.float64)[:n_walkers]
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    nelec = tuple(int(v) for v in cell.nelec)
    q = oracle_ratios(sh.oracle(name, f32), x, nelec, M, first_pair)
    q.setflags(write=False)
    return dict(x=x, q=q, cell=cell, nelec=nelec)


@functools.lru_cache(maxsize=None)
def shared_reference(which):
    """The shared-k plane-wave network on 'lih' / 'bcc_li' (fixture walkers) or on the one-atom cell 'n_up,n_dn' (5 synthetic
    walkers): dict cell, klist, net_kw, params, x, nelec, q_all (B, P) from the ORACLE."""
    from deepsolid_amd import systems
    if which in ('lih', 'bcc_li'):
        fx, cell, klist, _, _ = sh.case(which)
        x = np.asarray(fx['x'], dtype=np.float64)
    else:
        cell, klist = small_cell(tuple(int(v) for v in which.split(',')))
        x = systems.synthetic_walkers(cell, 5, seed=8)
    pw_klist, net_kw, params = shared_plane_wave_case(cell, klist)
    nelec = tuple(int(v) for v in cell.nelec)
    o = sh.Oracle(cell, pw_klist, net_kw, params)
    q = oracle_ratios(o, x, nelec, nelec[0] * nelec[1], 0)
    q.setflags(write=False)
    return dict(cell=cell, klist=pw_klist, net_kw=net_kw, params=params, x=x, nelec=nelec, q_all=q)


def spin_value(nelec, M, sum_re, n_good):
    """The formula of DESIGN.md section 17 in plain numpy."""
    nu, nd = nelec
    sz = 0.5 * (nu - nd)
    return sz * (sz + 1.0) + nd - (nu * nd / M) * sum_re / n_good
