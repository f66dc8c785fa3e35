"""Shared by test_force_cpu.py and test_gpu_force.py: float64 CPU references of the ionic forces of csrc/ds_force.h (DESIGN.md
section 21), made from the oracle's Ewald sum by automatic differentiation, and a numpy model of the order in which the call adds
its `sums`.

  HF force    the oracle `EwaldSum` with its atom tensor replaced by a leaf: `ion_exp_re`, `ion_exp_im` and the ion-ion energy are
              rebuilt in torch from that leaf, F = -autograd(E_ei + E_ii).  The minimal-image choice is an argmin / a remainder, so
              it is held fixed under the derivative, as in the kernel.
  ZV term     Q_a(x) = -Z_a sum_i c(r_ia) v_ia / r_ia coded directly, v_ia the nearest image by brute force over lattice
              vectors; grad Q and lap Q (the trace of the Hessian over all 3N coordinates) by forward-mode autograd, dF = -1/2 lap Q - grad Q . d.  `zv_delta_closed` is the closed form of
              DESIGN.md section 21 in numpy.
  tables32    the same references with the handle's tables (atoms, charges, lattice, its inverse, the displacement and shift
              tables, G points, weights, alpha) rounded to float32: what a float32 handle holds.
"""
import copy

import numpy as np
import torch

from oracle import ewaldsum as oew

GROUP = 256          # ds::FORCE_GROUP: walkers per row of partial sums


class ShiftedCell:
    """What `oracle.ewaldsum.EwaldSum` reads of a cell, with other atom positions."""

    def __init__(self, cell, coords):
        self._cell, self._coords = cell, np.asarray(coords, np.float64)
        self.nelec = cell.nelec

    def atom_coords(self):
        return self._coords

    def atom_charges(self):
        return self._cell.atom_charges()

    def lattice_vectors(self):
        return self._cell.lattice_vectors()


def _r32(t):
    return t.to(torch.float32).to(torch.float64)


_EWALDS = {}


def ewald(cell, tables32=False):
    """The oracle's EwaldSum of `cell` (cached per cell object); `tables32`: every table rounded to float32."""
    key = (id(cell), bool(tables32))
    if key not in _EWALDS:
        ew = oew.EwaldSum(cell)
        if tables32:
            ew = copy.copy(ew)
            ew.dist = copy.copy(ew.dist)
            for name in ('atom_coords', 'atom_charges', 'lattice_displacements', 'gpoints', 'gweight'):
                setattr(ew, name, _r32(getattr(ew, name)))
            ew.alpha = float(np.float32(ew.alpha))
            for name in ('_latvec', '_invvec', 'shifts'):
                setattr(ew.dist, name, _r32(getattr(ew.dist, name)))
        _EWALDS[key] = (ew, cell)       # (the cell is kept alive: its id is the key)
    return _EWALDS[key][0]


def energies_from_atoms(ew, atoms, x):
    """(E_ei, E_ii) of walker x (3N,) as torch functions of the atom tensor `atoms` (A, 3): the oracle's own `ewald_electron` on a
    shallow copy whose atom tensor and ion structure factor are rebuilt from `atoms`, and `_ewald_ion` restated in torch."""
    e = copy.copy(ew)
    q = ew.atom_charges
    gr = ew.gpoints @ atoms.T                                   # (NG, A)
    e.atom_coords = atoms
    e.ion_exp_re = torch.cos(gr) @ q
    e.ion_exp_im = torch.sin(gr) @ q
    nelec = sum(ew.nelec)
    _, ei = e.ewald_electron(x)
    ei = ei + ew.ei_const(nelec)
    if len(q) == 1:
        real = torch.zeros((), dtype=torch.float64)
    else:
        d = ew.dist.dist_matrix(atoms.reshape(-1))
        rv = d[None] + ew.lattice_displacements[:, None, None, :]
        # (the diagonal, which triu drops, holds a zero vector: + 1 keeps the derivative of its norm finite)
        r = torch.sqrt(torch.sum(rv * rv, dim=-1) + torch.eye(len(q), dtype=torch.float64))
        real = torch.sum(torch.triu(q[:, None] * q[None, :] * torch.erfc(ew.alpha * r) / r, diagonal=1))
    ii = real + torch.dot(ew.gweight, e.ion_exp_re ** 2 + e.ion_exp_im ** 2) + ew.ii_const
    return ei, ii


def hf_parts(ew, x):
    """-> (F_ei (B, A, 3), F_ii (A, 3)) numpy: minus the autograd derivatives of E_ei (per walker) and E_ii with respect to the atoms."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64).reshape(-1, 3 * sum(ew.nelec))
    f_ei = []
    for b in range(x.shape[0]):
        atoms = ew.atom_coords.detach().clone().requires_grad_(True)
        ei, ii = energies_from_atoms(ew, atoms, x[b])
        f_ei.append(-torch.autograd.grad(ei, atoms, retain_graph=True)[0])
        if b == 0:
            f_ii = -torch.autograd.grad(ii, atoms)[0]
    return torch.stack(f_ei).numpy(), f_ii.numpy()


def hf_force(ew, x):
    """(B, A, 3): the Hellmann-Feynman force -d(E_ei + E_ii)/dR_a of every walker."""
    f_ei, f_ii = hf_parts(ew, x)
    return f_ei + f_ii[None]


def nearest_shift(ew, x):
    """(N, A, 3) torch, a constant: the lattice vector that takes r_i - R_a to its nearest image, by brute force over the lattice
    vectors with coefficients in -3..3 -- NOT the oracle's `dist_i`, whose fractional wrap of a non-orthogonal cell (the bcc
    cells) is the nearest image only within half the smallest plane spacing."""
    n = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(-3, 4)] * 3, indexing='ij')], axis=1).astype(np.float64)
    lat = torch.as_tensor(n) @ ew.dist._latvec                                       # (343, 3)
    d = x.detach().reshape(-1, 1, 3) - ew.atom_coords.reshape(1, -1, 3)              # (N, A, 3)
    cand = d[None] + lat[:, None, None, :]
    return lat[torch.argmin(torch.sum(cand * cand, dim=-1), dim=0)]


def nearest_image(ew, x, shift=None):
    """(N, A, 3) torch: the nearest image of r_i - R_a; with `shift` (of `nearest_shift`) the choice is held fixed."""
    shift = nearest_shift(ew, x) if shift is None else shift
    return x.reshape(-1, 1, 3) - ew.atom_coords.reshape(1, -1, 3) + shift


def kernel_zv_image(latvec, d):
    """The image of d = r_i - R_a that k_ion_forces gives the zero-variance term (csrc/ds_force.h), restated in numpy: the
    fractional wrap of d (coordinates minus their nearest integers), then the nearest of the 27 images around it."""
    latvec = np.asarray(latvec, np.float64)
    f = np.asarray(d, np.float64) @ np.linalg.inv(latvec)
    w = (f - np.rint(f)) @ latvec
    disp = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing='ij'), -1).reshape(-1, 3) @ latvec
    cand = w[None, :] + disp
    return cand[np.argmin((cand ** 2).sum(axis=1))]


def q_function(ew, x, r_c, shift=None):
    """Q (A, 3) of walker x (3N,) torch: -Z_a sum_i c(r_ia) v_ia / r_ia, v = the nearest image of r_i - R_a (`shift`: its lattice
    vectors, computed ahead where x is traced by a torch.func transform)."""
    v = nearest_image(ew, x, shift)                             # (N, A, 3)
    r = torch.linalg.norm(v, dim=-1)
    c = torch.where(r < r_c, (1 - (r / r_c) ** 2) ** 3, torch.zeros_like(r))
    return -ew.atom_charges[:, None] * torch.sum(c[..., None] * v / r[..., None], dim=0)


def zv_delta_autograd(ew, x, drift, r_c):
    """(B, A, 3): dF = -1/2 lap Q - grad Q . d by forward-mode autograd of `q_function`: lap Q = the trace of the Hessian over all 3N
    coordinates (the second directional derivative along every unit vector, a jvp of a jvp), grad Q . d = one jvp along d."""
    n3 = 3 * sum(ew.nelec)
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64).reshape(-1, n3)
    d = torch.as_tensor(np.asarray(drift), dtype=torch.float64).reshape(-1, n3)
    out = []
    for xb, db in zip(x, d):
        shift = nearest_shift(ew, xb)
        f = lambda y: q_function(ew, y, r_c, shift)
        second = lambda v: torch.func.jvp(lambda y: torch.func.jvp(f, (y,), (v,))[1], (xb,), (v,))[1]
        lap = torch.func.vmap(second)(torch.eye(n3, dtype=torch.float64)).sum(0)
        out.append((-0.5 * lap - torch.func.jvp(f, (xb,), (db,))[1]).numpy())
    return np.stack(out)


def zv_delta_closed(ew, x, drift, r_c):
    """(B, A, 3): the closed form  sum_i [ -1/2 (g'' + 4 g'/r) v - g d_i - (g'/r) (v.d_i) v ],  g = -Z c(r)/r,  in numpy."""
    n = sum(ew.nelec)
    x = np.asarray(x, np.float64).reshape(-1, 3 * n)
    d = np.asarray(drift, np.float64).reshape(-1, n, 3)
    Z = ew.atom_charges.numpy()
    out = np.zeros((x.shape[0], len(Z), 3))
    for b in range(x.shape[0]):
        v = nearest_image(ew, torch.as_tensor(x[b])).numpy()                                 # (N, A, 3)
        r = np.linalg.norm(v, axis=-1)
        inside = r < r_c
        u = 1 - (r / r_c) ** 2
        c, c1, c2 = u ** 3, -6 * r * u ** 2 / r_c ** 2, -6 * u ** 2 / r_c ** 2 + 24 * r ** 2 * u / r_c ** 4
        g = -Z * c / r
        g1 = -Z * (c1 / r - c / r ** 2)
        g2 = -Z * (c2 / r - 2 * c1 / r ** 2 + 2 * c / r ** 3)
        vd = np.einsum('iak,ik->ia', v, d[b])
        term = (-0.5 * (g2 + 4 * g1 / r) - g1 / r * vd)[..., None] * v - g[..., None] * d[b][:, None, :]
        out[b] = np.where(inside[..., None], term, 0.0).sum(axis=0)
    return out


def reference(ew, x, drift, r_c):
    """-> (hf, zv) (B, A, 3): the two outputs of `ds_ion_forces`."""
    hf = hf_force(ew, x)
    return hf, hf + zv_delta_autograd(ew, x, drift, r_c)


# ------------------------------------------------------------------------------------------------ the order of `sums`
def tree(v):
    """The LDS tree over GROUP entries: entry t += entry t + s for s = GROUP/2 .. 1."""
    v = np.array(v, dtype=np.float64)
    assert v.shape[0] == GROUP
    s = GROUP // 2
    while s:
        v[:s] += v[s:2 * s]
        s //= 2
    return v[0]


def sums_model(sums, hf, zv):
    """`sums` (12 A + 1,) after a call whose walker outputs are hf, zv (B, A, 3; NaN rows = bad walkers), bit for bit: per group of
    GROUP walkers the tree over (f, f * f) of the good ones (0 for the others and for the padding), the groups added in order."""
    sums = np.array(sums, dtype=np.float64)
    B, A = hf.shape[0], hf.shape[1]
    hf, zv = hf.reshape(B, 3 * A), zv.reshape(B, 3 * A)
    good = ~np.isnan(hf[:, 0])
    for g0 in range(0, B, GROUP):
        sl = slice(g0, min(B, g0 + GROUP))
        ok = np.zeros(GROUP, bool)
        ok[:sl.stop - g0] = good[sl]
        for j in range(3 * A):
            fh, fz = np.zeros(GROUP), np.zeros(GROUP)
            fh[:sl.stop - g0] = np.where(good[sl], hf[sl, j], 0.0)
            fz[:sl.stop - g0] = np.where(good[sl], zv[sl, j], 0.0)
            for k, col in enumerate((fh, fh * fh, fz, fz * fz)):
                sums[4 * j + k] += tree(col)
        sums[12 * A] += tree(ok.astype(np.float64))
    return sums


# ------------------------------------------------------------------------------------------------ walkers
def min_ion_distance(ew, x):
    """Smallest nearest-image electron-ion distance of every walker (B,)."""
    n3 = 3 * sum(ew.nelec)
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64).reshape(-1, n3)
    return np.array([float(torch.linalg.norm(nearest_image(ew, xb), dim=-1).min()) for xb in x])


def spread_walkers(cell, ew, batch, seed, r_min=0.3):
    """`batch` uniform-in-cell walkers whose electrons all stay `r_min` bohr away from every ion (rejection per walker)."""
    rng = np.random.default_rng(seed)
    n = sum(cell.nelec)
    out = []
    while len(out) < batch:
        x = (rng.uniform(size=(n, 3)) @ np.asarray(cell.lattice_vectors())).reshape(3 * n)
        if min_ion_distance(ew, x[None])[0] > r_min:
            out.append(x)
    return np.stack(out)
