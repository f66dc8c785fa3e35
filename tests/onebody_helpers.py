"""Shared by test_onebody_cpu.py and test_gpu_onebody.py: a plain-numpy replay of the shifts `ds_one_body_ratios` draws (Philox
stream 3 on top of sampler_helpers), the one-body ratios of the float64 CPU oracle (complex eval_logdet of R' and R), the numpy
fold of ratios into momentum sums, and a plane-wave network whose ratios are known in closed form."""
import functools

import numpy as np
import torch

import sampler_helpers as sh

SHIFT_STREAM = 3


def shift_blocks(seed, offset, n):
    """The two Philox blocks of samples g = 0..n-1: (A (4, n), B (4, n)), A at index 2g and B at index 2g + 1, step 0."""
    g = np.arange(n, dtype=np.uint64)
    two = np.uint64(2)
    return (sh.philox_block(seed, offset, 0, two * g, SHIFT_STREAM),
            sh.philox_block(seed, offset, 0, two * g + np.uint64(1), SHIFT_STREAM))


def replay_shifts(seed, offset, B, M, a):
    """-> (s (B, M, 3) float64 = f . a, f (B, M, 3) in [0, 1)), products and sums rounded one by one in the kernel's order."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    A, Bk = shift_blocks(seed, offset, B * M)
    f = np.stack([sh.u53_co(A[0], A[1]), sh.u53_co(A[2], A[3]), sh.u53_co(Bk[0], Bk[1])], axis=-1)
    s = (f[:, 0:1] * a[0] + f[:, 1:2] * a[1]) + f[:, 2:3] * a[2]
    return s.reshape(B, M, 3), f.reshape(B, M, 3)


def electrons(M, N, first):
    """Electron moved by sample m of every walker."""
    return (first + np.arange(M)) % N


def displaced(x, s, first):
    """x (B, 3N), s (B, M, 3) -> R' (B, M, 3N): electron (first + m) % N moved by s[:, m], nothing wrapped."""
    x = np.asarray(x, dtype=np.float64)
    B, M = s.shape[:2]
    N = x.shape[1] // 3
    xd = np.repeat(x.reshape(B, 1, N, 3), M, axis=1).copy()
    xd[:, np.arange(M), electrons(M, N, first)] += s
    return xd.reshape(B, M, 3 * N)


def oracle_ratios(o, x, s, first):
    """q (B, M) complex128 from the oracle `o` (sampler_helpers.Oracle): exp(log psi(R') - log psi(R)) with the complex
    eval_logdet = log|psi| + i arg psi.  With a float32 oracle the configurations are rounded to float32 first."""
    xd = displaced(x, s, first)
    B, M, n3 = xd.shape
    l0 = o.logdet(x)
    l1 = o.logdet(xd.reshape(B * M, n3)).reshape(B, M)
    d = (l1 - l0[:, None]).to(torch.complex128).numpy()
    return np.exp(d)


def fold(q, s, kvec, first, nelec):
    """sums (2, n_k, 2) float64: sums[spin(e)][k] += q exp(-i k.s) over all samples."""
    B, M = q.shape
    spin = (electrons(M, sum(nelec), first) >= nelec[0]).astype(int)
    t = q[:, :, None] * np.exp(-1j * np.einsum('bmc,kc->bmk', s, np.asarray(kvec, dtype=np.float64)))
    out = np.zeros((2, len(kvec)), dtype=np.complex128)
    for sp in range(2):
        out[sp] = t[:, spin == sp].sum(axis=(0, 1))
    return np.stack([out.real, out.imag], axis=-1)


def samples_per_spin(B, M, first, nelec):
    up = int(np.count_nonzero(electrons(M, sum(nelec), first) < nelec[0]))
    return np.asarray([B * up, B * (M - up)])


# ------------------------------------------------------------------------------------------------------ plane-wave network
PW_NET_KW = dict(envelope_type='isotropic', bias_orbitals=True, use_last_layer=False, full_det=False,
                 hidden_dims=((32, 8), (32, 8)), determinants=2, distance_type='nu')


def plane_wave_case(cell, klist):
    """A network that IS a determinant of plane waves: orbital weights 0, bias 1 on the real and 0 on the imaginary columns,
    envelope sigma = 0 and pi = 1 / A, so every orbital is exp(i k_j . r) and both determinants are equal.
    The occupied k_j = k_t + n_j . G_S are distinct points of {0, 1, -1}^3 (the HF klist repeats k, which makes the determinant
    singular): points 0.. of `momentum_kpoints` for spin up, the next ones for spin down.
    -> (custom klist, net_kw, numpy params, kpts (27, 3), occupied indices per spin)."""
    from deepsolid_amd import estimator
    from oracle.network import init_solid_fermi_net_params
    kpts, _ = estimator.momentum_kpoints(cell, klist, 1)
    nelec = tuple(int(v) for v in cell.nelec)
    occ = [np.arange(nelec[0]), nelec[0] + np.arange(nelec[1])]
    pw_klist = (kpts[occ[0]], kpts[occ[1]])
    atoms = np.asarray(cell.original_cell.atom_coords()).reshape(-1, 3)
    params = init_solid_fermi_net_params(np.random.default_rng(5), atoms, nelec, **PW_NET_KW)
    for orb, env in zip(params['orbital'], params['envelope']):
        npar = orb['w'].shape[1] // 2
        orb['w'] = np.zeros_like(orb['w'])
        orb['b'] = np.concatenate([np.ones(npar), np.zeros(npar)])
        env['sigma'] = np.zeros_like(env['sigma'])
        env['pi'] = np.full_like(env['pi'], 1.0 / len(atoms))
    return pw_klist, dict(PW_NET_KW), params, kpts, occ


def plane_wave_ratios(x, s, first, pw_klist, nelec):
    """q (B, M) of the plane-wave determinant from positions alone: q = sum_j exp(i k_j . s) phi_j(r_e) (M^-1)_{je} with
    M_ij = phi_j(r_i) = exp(i k_j . r_i) over the electrons and orbitals of the moved electron's spin."""
    x = np.asarray(x, dtype=np.float64)
    B, M = s.shape[:2]
    N = sum(nelec)
    r = x.reshape(B, N, 3)
    q = np.zeros((B, M), dtype=np.complex128)
    for m, e in enumerate(electrons(M, N, first)):
        sp = 0 if e < nelec[0] else 1
        lo = 0 if sp == 0 else nelec[0]
        k = np.asarray(pw_klist[sp], dtype=np.float64)
        for b in range(B):
            mat = np.exp(1j * r[b, lo:lo + nelec[sp]] @ k.T)              # [electron, orbital]
            inv = np.linalg.inv(mat)
            q[b, m] = np.sum(np.exp(1j * k @ s[b, m]) * mat[e - lo] * inv[:, e - lo])
    return q


def grid_shifts(a, B, N):
    """(B, 27 N, 3): for every electron in turn (sample m moves electron m % N with first_electron = 0) one full 3 x 3 x 3 grid of
    the cell: sample m = N t + e carries grid point t."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    pts = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(3) / 3.0] * 3, indexing='ij')], axis=1) @ a
    return np.broadcast_to(np.repeat(pts, N, axis=0)[None], (B, 27 * N, 3)).copy()


@functools.lru_cache(maxsize=None)
def reference(name, seed, offset, M, first, f32=False, n_walkers=None):
    """Oracle side of the Philox-mode tests of case `name` on its fixture walkers (the first `n_walkers` of them), computed once:
    dict x, s, q, cell, nelec."""
    fx, cell, _, _, _ = sh.case(name)
    x = np.asarray(fx['x'], dtype=np.float64)[:n_walkers]
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    s, _ = replay_shifts(seed, offset, len(x), M, cell.a)
    q = oracle_ratios(sh.oracle(name, f32), x, s, first)
    return dict(x=x, s=s, q=q, cell=cell, nelec=tuple(int(v) for v in cell.nelec))
