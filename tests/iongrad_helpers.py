"""Shared by test_iongrad_cpu.py and test_gpu_iongrad.py: the float64 CPU reference of d log psi / d R_a (csrc/ds_iongrad.h,
DESIGN.md section 22) -- torch autograd of `oracle.network.eval_func` with the primitive cell's atoms as a leaf tensor -- its
finite-difference and translation checks, and a numpy model of `estimator.PrimitiveForces`.  Nothing here needs a GPU."""
import functools

import numpy as np
import torch

from oracle import network as onet

from common import load_case


def _eval(params_t, x, atoms, cell, klist, net_kw):
    return onet.eval_func(params_t, x, klist, cell, atoms, tuple(int(s) for s in cell.nelec), net_kw.get('envelope_type', 'full'),
                          net_kw.get('full_det', True), net_kw.get('distance_type', 'nu'), 'eval_logdet')


def ion_grad_ref(cell, klist, net_kw, params, x, dtype=None, atoms=None):
    """-> (O (B, A, 3) complex128 = d log|psi| + i d arg psi in the atoms of the primitive cell, log psi (B,) complex128) at the
    walkers x (B, 3N).  `dtype=torch.float32`: the same computation run in float32 (what a straight float32 evaluation loses)."""
    x = np.asarray(x)
    atoms_np = np.asarray(cell.original_cell.atom_coords() if atoms is None else atoms, dtype=np.float64).reshape(-1, 3)
    out, lps = [], []

    def run():
        pt = onet.params_to_torch(params, dtype=dtype)
        for xx in x:
            at = torch.tensor(atoms_np, dtype=dtype or torch.float64, requires_grad=True)
            lp = _eval(pt, torch.as_tensor(xx, dtype=dtype or torch.float64), at, cell, klist, net_kw)
            re, = torch.autograd.grad(lp.real, at, retain_graph=True)
            im, = torch.autograd.grad(lp.imag, at)
            out.append(re.double().numpy() + 1j * im.double().numpy())
            lps.append(complex(lp.detach()))
    if dtype is None:
        run()
    else:
        with onet.working_dtype(dtype):
            run()
    return np.stack(out), np.asarray(lps)


def ion_grad_fd(cell, klist, net_kw, params, x, h=1e-5):
    """Central differences of log psi in the atoms (the phase difference is taken on the unit circle)."""
    atoms = np.asarray(cell.original_cell.atom_coords(), dtype=np.float64).reshape(-1, 3)
    pt = onet.params_to_torch(params)
    out = np.zeros((len(x),) + atoms.shape, dtype=np.complex128)

    def lp(xx, at):
        with torch.no_grad():
            return complex(_eval(pt, torch.as_tensor(xx, dtype=torch.float64), torch.as_tensor(at), cell, klist, net_kw))
    for b, xx in enumerate(np.asarray(x)):
        for a in range(atoms.shape[0]):
            for c in range(3):
                ap, am = atoms.copy(), atoms.copy()
                ap[a, c] += h
                am[a, c] -= h
                p, m = lp(xx, ap), lp(xx, am)
                out[b, a, c] = ((p.real - m.real) + 1j * np.angle(np.exp(1j * (p.imag - m.imag)))) / (2 * h)
    return out


def walker_grad_ref(cell, klist, net_kw, params, x):
    """-> (B, 3N) complex: d log psi / d x by the same autograd (the other side of the translation identities)."""
    pt = onet.params_to_torch(params)
    atoms = torch.as_tensor(np.asarray(cell.original_cell.atom_coords(), dtype=np.float64).reshape(-1, 3))
    out = []
    for xx in np.asarray(x):
        xt = torch.tensor(xx, dtype=torch.float64, requires_grad=True)
        lp = _eval(pt, xt, atoms, cell, klist, net_kw)
        re, = torch.autograd.grad(lp.real, xt, retain_graph=True)
        im, = torch.autograd.grad(lp.imag, xt)
        out.append(re.numpy() + 1j * im.numpy())
    return np.stack(out)


def klist_row_sum(klist, nelec):
    """Sum of the k-points of all occupied orbitals of both spins: a rigid translation t of electrons and atoms multiplies psi by
    exp(i t . this), whatever the determinant layout (with full_det the concatenated list, the same rows)."""
    tot = np.zeros(3)
    for s, n in enumerate(nelec):
        if n:
            tot += np.asarray(klist[s], dtype=np.float64).reshape(-1, 3)[:n].sum(0)
    return tot


@functools.lru_cache(maxsize=None)
def reference(name, B, seed=77):
    """(x, O, log psi) of `systems.synthetic_walkers(cell, B, seed)` of a case, computed once per session; read-only."""
    from deepsolid_amd import systems
    fx, cell, klist, net_kw, params = load_case(name)
    x = systems.synthetic_walkers(cell, B, seed=seed)
    O, lp = ion_grad_ref(cell, klist, net_kw, params, x)
    for a in (x, O, lp):
        a.setflags(write=False)
    return x, O, lp


# ---------------------------------------------------------------- numpy model of estimator.PrimitiveForces
def fold_model(sim_atoms, prim_atoms, prim_latvec):
    """image s of the simulation cell -> primitive atom s // scale, or ValueError when that is not a lattice translate."""
    sim_atoms, prim_atoms = np.asarray(sim_atoms, dtype=np.float64), np.asarray(prim_atoms, dtype=np.float64)
    scale = len(sim_atoms) // len(prim_atoms)
    if scale * len(prim_atoms) != len(sim_atoms):
        raise ValueError('ion count is not a multiple of the primitive cell')
    owner = np.arange(len(sim_atoms)) // scale
    frac = (sim_atoms - prim_atoms[owner]) @ np.linalg.inv(np.asarray(prim_latvec, dtype=np.float64))
    if np.abs(frac - np.round(frac)).max() > 1e-8:
        raise ValueError('not atom-major')
    return owner


def block_row_model(E, zv_sim, hf_sim, O, owner, A):
    """One block row [n_good, sum Re E, sum Im E, per (a, c): sum zv, sum hf, sum t] from per-walker arrays read back:
    E (B,) complex, zv_sim / hf_sim (B, As, 3) with NaN rows for bad walkers, O (B, A, 3) complex."""
    good = np.isfinite(zv_sim).all(axis=(1, 2)) & np.isfinite(hf_sim).all(axis=(1, 2))
    E, O = E[good], O[good]
    fold = np.zeros((A, len(owner)))
    fold[owner, np.arange(len(owner))] = 1
    zv = np.einsum('as,bsc->bac', fold, zv_sim[good])
    hf = np.einsum('as,bsc->bac', fold, hf_sim[good])
    d = E - E.mean()
    t = (np.conj(d)[:, None, None] * O).real.sum(0)
    row = [float(good.sum()), E.real.sum(), E.imag.sum()]
    for a in range(A):
        for c in range(3):
            row += [zv[:, a, c].sum(), hf[:, a, c].sum(), t[a, c]]
    return np.asarray(row)


def forces_model(rows, A, reblock):
    """rows (nblocks, 3 + 9 A) -> dict of (value, error) arrays (A, 3) for total / zv / hf / pulay as PrimitiveForces.forces():
    per block zv = sum / n, pulay = -2 sum t / (n - 1); block averages weighted by n; error = reblock(series) (at least eight blocks per level, or all of them when there are fewer)."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows[:, 0]
    body = rows[:, 3:].reshape(len(rows), A, 3, 3)
    series = dict(zv=body[..., 0] / n[:, None, None], hf=body[..., 1] / n[:, None, None], pulay=-2 * body[..., 2] / (n - 1)[:, None, None])
    series['total'] = series['zv'] + series['pulay']
    out = {}
    for k, v in series.items():
        val = (v * n[:, None, None]).sum(0) / n.sum()
        err = np.array([[reblock(v[:, a, c], min(8, max(2, len(v))))[1] for c in range(3)] for a in range(A)])
        out[k] = (val, err)
    return out
