"""Shared by test_stress_cpu.py and test_gpu_stress.py: float64 CPU references of the strain derivatives of csrc/ds_stress.h
 and a numpy model of the order in which the call adds its `sums`.

  closed form      `closed_form(ew, x)`: dE_ee / d eps, dE_ei / d eps per walker and dE_ii / d eps in numpy from the oracle's tables and
                   the oracle's own minimal images; `kinetic(grad)`: the kinetic tensor of a complex gradient.
  strained oracle  `strained(ew, eps)`: a copy of the oracle `EwaldSum` on the cell strained by eps, with alpha and the integer G list
                   held fixed: lattice, displacements, G points (g (1 + eps)^-1), weights, atoms, the ion structure factor and the
                   constants are rebuilt; its `MinimalImageDistance` is replaced by one that takes the image of the UNSTRAINED cell
                   at the unstrained positions and strains it (the choice is a function of fractional coordinates, which the strain
                   does not change; a fresh `MinimalImageDistance` of a sheared cubic cell would switch its dispatch).
                   `fd_strain` takes central differences of its energy.
  tables32         `ewald(cell, tables32=True)`: every table a float32 handle holds rounded to float32 (force_helpers.ewald, plus the
                   ion structure factor, and the minimal image taken on the rounded lattice).
"""
import copy

import numpy as np
import torch
from scipy.special import erfc

import force_helpers as fh

GROUP = fh.GROUP
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))          # xx, yy, zz, yz, xz, xy


def to_voigt(m):
    """(..., 3, 3) -> (..., 6)."""
    m = np.asarray(m, np.float64)
    return np.stack([m[..., a, b] for a, b in VOIGT], axis=-1)


def strain_matrix(k, h):
    """The symmetric strain with eps_ab = eps_ba = h for component k of VOIGT (so d/dh is d/d eps_ab for a = b and the sum of the ab and
    ba derivatives, twice the symmetric one, otherwise: `fd_strain` halves it)."""
    a, b = VOIGT[k]
    e = np.zeros((3, 3))
    e[a, b] = e[b, a] = h
    return e


_EWALDS = {}


def ewald(cell, tables32=False):
    """The oracle's EwaldSum of `cell` (cached per cell object; force_helpers.ewald); `tables32`: every table of a float32 handle rounded
    to float32, the ion structure factor included, and `dist_i` bound to the copy that holds the rounded lattice."""
    if not tables32:
        return fh.ewald(cell)
    key = id(cell)
    if key not in _EWALDS:
        ew = copy.copy(fh.ewald(cell, tables32=True))
        ew.dist = copy.copy(ew.dist)
        ew.dist.dist_i = getattr(ew.dist, ew.dist.mode + '_dist_i')
        ew.ion_exp_re, ew.ion_exp_im = fh._r32(ew.ion_exp_re), fh._r32(ew.ion_exp_im)
        _EWALDS[key] = (ew, cell)
    return _EWALDS[key][0]


def volume(ew):
    return float(abs(torch.linalg.det(ew.dist._latvec)))


# ------------------------------------------------------------------------------------------------ the closed form
def _real_tensor(v, alpha):
    """sum over the leading axes' images of f'(r) v_a v_b / r for vectors v (..., 3) -> (3, 3)."""
    v = v.reshape(-1, 3)
    r = np.linalg.norm(v, axis=1)
    h = -(erfc(alpha * r) / r ** 2 + 2 * alpha / np.sqrt(np.pi) * np.exp(-(alpha * r) ** 2) / r) / r
    return np.einsum('s,sa,sb->ab', h, v, v)


def strain_weights(ew):
    """(NG, 3, 3): dw_G / d eps_ab = w_G [-delta_ab + 2 G_a G_b (1 / G^2 + 1 / (4 alpha^2))]."""
    g, w = ew.gpoints.numpy(), ew.gweight.numpy()
    g2 = np.einsum('gk,gk->g', g, g)
    f = 2.0 * (1.0 / g2 + 0.25 / ew.alpha ** 2)
    return w[:, None, None] * (f[:, None, None] * g[:, :, None] * g[:, None, :] - np.eye(3)[None])


def closed_form(ew, x):
    """-> (ee (B, 3, 3), ei (B, 3, 3), ii (3, 3)): the strain derivatives of the three energies of `ew.energy` in Hartree."""
    n = sum(ew.nelec)
    x = np.asarray(x, np.float64).reshape(-1, 3 * n)
    q = ew.atom_charges.numpy()
    disp = ew.lattice_displacements.numpy()
    al = ew.alpha
    V = volume(ew)
    ijconst = -np.pi / (V * al ** 2)
    dw = strain_weights(ew)
    g = ew.gpoints.numpy()
    ion = ew.ion_exp_re.numpy() + 1j * ew.ion_exp_im.numpy()
    ee, ei = np.zeros((len(x), 3, 3)), np.zeros((len(x), 3, 3))
    for b, xb in enumerate(x):
        xt = torch.as_tensor(xb)
        d_ei = ew.dist.dist_i(ew.atom_coords.reshape(-1), xt).numpy()             # (N, A, 3) = r_i - R_a
        for a in range(len(q)):
            ei[b] += -q[a] * _real_tensor(d_ei[:, a, None, :] + disp[None], al)
        if n > 1:
            d_ee = ew.dist.dist_matrix(xt).numpy()                                # (N, N, 3) = r_i - r_j
            iu = np.triu_indices(n, 1)
            ee[b] += _real_tensor(d_ee[iu][:, None, :] + disp[None], al)
        s = np.exp(1j * (xb.reshape(n, 3) @ g.T)).sum(axis=0)
        ee[b] += np.einsum('g,gab->ab', np.abs(s) ** 2, dw)
        ei[b] += 2 * np.einsum('g,gab->ab', -ion.real * s.real - ion.imag * s.imag, dw)
        ee[b] += -(0.5 * n * n * ijconst) * np.eye(3)
        ei[b] += n * q.sum() * ijconst * np.eye(3)
    ii = np.einsum('g,gab->ab', np.abs(ion) ** 2, dw) - 0.5 * q.sum() ** 2 * ijconst * np.eye(3)
    if len(q) > 1:
        d = ew.dist.dist_matrix(ew.atom_coords.reshape(-1)).numpy()
        for a in range(len(q)):
            for c in range(a + 1, len(q)):
                ii += q[a] * q[c] * _real_tensor(d[a, c][None, :] + disp, al)
    return ee, ei, ii


def kinetic(grad):
    """kin (B, 3, 3) = -sum_i (Re d_i Re d_i^T + Im d_i Im d_i^T) of a complex gradient (B, 3N)."""
    d = np.asarray(grad).reshape(len(grad), -1, 3)
    return -(np.einsum('bia,bic->bac', d.real, d.real) + np.einsum('bia,bic->bac', d.imag, d.imag))


def reference_parts(ew, x, grad=None):
    """(B, 4, 6): the rows kin, ee, ei, total of `ds_stress` (kin zero without a gradient)."""
    ee, ei, ii = closed_form(ew, x)
    kin = kinetic(grad) if grad is not None else np.zeros_like(ee)
    return to_voigt(np.stack([kin, ee, ei, kin + ee + ei + ii[None]], axis=1))


# ------------------------------------------------------------------------------------------------ the strained oracle
class StrainedDistance:
    """The minimal images of the unstrained cell, strained: `dist_i` and `dist_matrix` of a `MinimalImageDistance` evaluated at the
    positions taken back to the unstrained cell, times F = 1 + eps."""

    def __init__(self, dist, F):
        self._dist, self._F = dist, torch.as_tensor(F)
        self._Finv = torch.linalg.inv(self._F)
        self._latvec = dist._latvec @ self._F
        self._invvec = torch.linalg.inv(self._latvec)
        self.shifts = dist.shifts @ self._F

    def _back(self, p):
        return (p.reshape(-1, 3) @ self._Finv).reshape(p.shape)

    def dist_i(self, configs, vec):
        return self._dist.dist_i(self._back(configs), self._back(vec)) @ self._F

    def dist_matrix(self, configs):
        return self._dist.dist_matrix(self._back(configs)) @ self._F


def strained(ew, eps):
    """-> (oracle EwaldSum of the cell strained by the symmetric `eps`, F = 1 + eps): alpha and the integer G list are those of `ew`."""
    F = np.eye(3) + np.asarray(eps, np.float64)
    Finv = np.linalg.inv(F)
    e = copy.copy(ew)
    lat = ew.dist._latvec.numpy() @ F
    e.latvec_np = lat
    e.dist = StrainedDistance(ew.dist, F)
    e.lattice_displacements_np = ew.lattice_displacements.numpy() @ F
    e.atom_coords_np = ew.atom_coords.numpy() @ F
    e.atom_charges_np = ew.atom_charges.numpy()
    e.gpoints_np = ew.gpoints.numpy() @ Finv
    V = abs(np.linalg.det(lat))
    g2 = np.einsum('gk,gk->g', e.gpoints_np, e.gpoints_np)
    e.gweight_np = 4 * np.pi * np.exp(-g2 / (4 * ew.alpha ** 2)) / (V * g2)
    e._set_constants(V)                        # ijconst, squareconst, ii_const, ion_exp_np and ion_ion of the strained cell
    for name in ('atom_coords', 'lattice_displacements', 'gpoints', 'gweight'):
        setattr(e, name, torch.as_tensor(getattr(e, name + '_np')))
    e.ion_exp_re, e.ion_exp_im = torch.as_tensor(e.ion_exp_np.real.copy()), torch.as_tensor(e.ion_exp_np.imag.copy())
    return e, F


def fd_strain(ew, x, h=1e-5):
    """-> (ee (B, 3, 3), ei (B, 3, 3), ii (3, 3)): central differences of the strained oracle's energies, electrons scaled along."""
    n = sum(ew.nelec)
    x = np.asarray(x, np.float64).reshape(-1, n, 3)
    out = np.zeros((3, len(x), 3, 3))
    for k, (a, c) in enumerate(VOIGT):
        vals = []
        for sgn in (+1, -1):
            e, F = strained(ew, strain_matrix(k, sgn * h))
            vals.append(np.array([[float(t) for t in e.energy(torch.as_tensor((xb @ F).reshape(-1)))] for xb in x]))   # (B, 3)
        d = (vals[0] - vals[1]) / (2 * h) / (1.0 if a == c else 2.0)
        out[:, :, a, c] = out[:, :, c, a] = d.T
    return out[0], out[1], out[2][0]


# ------------------------------------------------------------------------------------------------ the strain derivative of log psi
def generators():
    """(6, 3, 3): E_k with eps = h E_k, the off-diagonal entries h / 2 each (estimator.strain_generators, restated)."""
    E = np.zeros((6, 3, 3))
    for k, (a, b) in enumerate(VOIGT):
        E[k, a, b] += 0.5
        E[k, b, a] += 0.5
    return E


def oracle_log_derivative(cell, klist, net_kw, params, x, h):
    """O (B, 6) complex: [log psi_{+h}(x (1 + h E_k)) - log psi_{-h}(x (1 - h E_k))] / 2h with the ORACLE network on the cells of
    `supercell.strained`, the imaginary part (the phase difference) taken modulo 2 pi.  -> (O, largest |log psi| met)."""
    from common import oracle_net, tt
    from deepsolid_amd import supercell
    from oracle import network as onet
    p = onet.params_to_torch(params)
    x = np.asarray(x, np.float64)
    B = len(x)
    O = np.zeros((B, 6), complex)
    big = 0.0
    for k, E in enumerate(generators()):
        vals = []
        for sgn in (+1.0, -1.0):
            c2, k2 = supercell.strained(cell, klist, sgn * h * E)
            net = oracle_net(c2, k2, net_kw, 'eval_logdet')
            F = np.eye(3) + sgn * h * E
            vals.append(np.array([complex(net.apply(p, tt((xb.reshape(-1, 3) @ F).reshape(-1)))) for xb in x]))
        d = vals[0] - vals[1]
        O[:, k] = (d.real + 1j * np.angle(np.exp(1j * d.imag))) / (2 * h)
        big = max(big, np.abs(vals[0].real).max(), np.abs(vals[1].real).max())
    return O, big


# ------------------------------------------------------------------------------------------------ the order of `sums`
def sums_model(sums, parts):
    """`sums` (49,) after a call whose walker output is parts (B, 4, 6; NaN rows = bad walkers), bit for bit: per group of GROUP walkers
    the tree of force_helpers over (t, t * t) of the good ones (0 for the others and for the padding), the groups added in order."""
    sums = np.array(sums, dtype=np.float64)
    B = parts.shape[0]
    p = parts.reshape(B, 24)
    good = ~np.isnan(p[:, 18])
    for g0 in range(0, B, GROUP):
        sl = slice(g0, min(B, g0 + GROUP))
        ok = np.zeros(GROUP, bool)
        ok[:sl.stop - g0] = good[sl]
        for j in range(24):
            t = np.zeros(GROUP)
            t[:sl.stop - g0] = np.where(good[sl], p[sl, j], 0.0)
            sums[2 * j] += fh.tree(t)
            sums[2 * j + 1] += fh.tree(t * t)
        sums[48] += fh.tree(ok.astype(np.float64))
    return sums
