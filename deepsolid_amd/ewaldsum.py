"""Ewald sums: host-side table setup + device energy (reference DeepSolid/ewaldsum.py).

``EwaldSum(cell)`` mirrors the reference class: the constructor builds, once and
on the host, everything that depends on the cell only (alpha, the half-space G
mesh and its weights, the ion structure factor, the constants), and
``energy(configs)`` evaluates (ee, ei, ii) for a batch of walkers with the HIP
kernel ``k_ewald`` through the C ABI (``ds_ewald``).
"""
import numpy as np

from . import distance

EWALD_GMAX = 200          # reference ewaldsum.py:34
WEIGHT_CUTOFF = 1e-12     # reference ewaldsum.py:199


def _half_space_mesh(recvec, cellvolume, alpha, gmax, latvec=None):
    """G vectors with x>0, or x=0,y>0, or x=y=0,z>0 and weight above the cutoff
    (reference ewaldsum.py:67-89,194-200).  Order = the reference's: the three
    groups concatenated, each in C order of its integer mesh.

    The reference scans all (2 gmax + 1)^3 / 2 = 3.2e7 integer triples; the weight falls monotonically with |G|^2, so only
    triples inside the sphere w(|G|^2) = cutoff can pass, and n_j = G . a_j / 2 pi bounds each integer by |G|max |a_j| / 2 pi:
    the scan runs over that box only (same points, same order: a sub-box of a C-ordered mesh keeps the order of what it keeps)."""
    lo, hi = 0.0, 1.0
    wfun = lambda g2: 4 * np.pi * np.exp(-g2 / (4 * alpha ** 2)) / (cellvolume * g2)
    while wfun(hi) > WEIGHT_CUTOFF:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if wfun(mid) > WEIGHT_CUTOFF else (lo, mid)
    gm = np.sqrt(hi) * (1 + 1e-9)
    if latvec is None:
        latvec = np.linalg.inv(recvec).T
    nmax = [int(min(gmax, np.floor(gm * np.linalg.norm(latvec[j]) / (2 * np.pi)) + 1)) for j in range(3)]
    fy, fz = np.arange(-nmax[1], nmax[1] + 1), np.arange(-nmax[2], nmax[2] + 1)
    pts, wts = [], []

    def scan(ix, iy, iz):
        X, Y, Z = np.meshgrid(ix, iy, iz, indexing='ij')
        n = np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(np.float64)
        g = (n @ recvec) * (2 * np.pi)
        g2 = np.einsum('ik,ik->i', g, g)
        w = 4 * np.pi * np.exp(-g2 / (4 * alpha ** 2)) / (cellvolume * g2)
        keep = w > WEIGHT_CUTOFF
        if keep.any():
            pts.append(g[keep])
            wts.append(w[keep])

    for x0 in range(1, nmax[0] + 1, 8):
        scan(np.arange(x0, min(x0 + 8, nmax[0] + 1)), fy, fz)
    scan(np.array([0]), np.arange(1, nmax[1] + 1), fz)
    scan(np.array([0]), np.array([0]), np.arange(1, nmax[2] + 1))
    return np.concatenate(pts, axis=0), np.concatenate(wts, axis=0)


class EwaldTables:
    """Cell-only quantities of the Ewald sum (reference ewaldsum.py:34-136)."""

    def __init__(self, cell, ewald_gmax=EWALD_GMAX):
        self.nelec = tuple(int(n) for n in cell.nelec)
        self.atom_coords = np.asarray(cell.atom_coords(), dtype=np.float64)
        self.atom_charges = np.asarray(cell.atom_charges(), dtype=np.float64)
        self.latvec = np.asarray(cell.lattice_vectors(), dtype=np.float64)
        self.dist_mode = distance.minimal_image_mode(self.latvec)
        volume = np.linalg.det(self.latvec)
        recvec = np.linalg.inv(self.latvec).T
        self.alpha = 5.0 / np.amin(1.0 / np.linalg.norm(recvec, axis=1))          # :63-64
        self.gpoints, self.gweight = _half_space_mesh(recvec, volume, self.alpha, ewald_gmax, self.latvec)
        q = self.atom_charges
        self.i_sum = q.sum()
        ii_sum2 = (q ** 2).sum()
        ii_sum = (self.i_sum ** 2 - ii_sum2) / 2
        self.ijconst = -np.pi / (volume * self.alpha ** 2)                         # :97
        self.squareconst = -self.alpha / np.sqrt(np.pi) + self.ijconst / 2         # :98
        self.ii_const = ii_sum * self.ijconst + ii_sum2 * self.squareconst          # :100
        self.ion_exp = np.exp(1j * (self.gpoints @ self.atom_coords.T)) @ q         # :131-132
        self.ion_ion = self._ion_ion_real() + float(self.gweight @ np.abs(self.ion_exp) ** 2)

    def _ion_ion_real(self):
        """Real-space ion-ion sum over pairs a<b and the 27 neighbour cells (:122-129)."""
        from scipy.special import erfc
        n = len(self.atom_charges)
        if n == 1:
            return 0.0
        shifts = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing='ij'), -1).reshape(-1, 3) @ self.latvec
        tot = 0.0
        for a in range(n):
            for b in range(a + 1, n):
                d = distance.minimal_image_host(self.latvec, self.dist_mode,
                                                self.atom_coords[a] - self.atom_coords[b])
                r = np.linalg.norm(d[None, :] + shifts, axis=1)
                tot += self.atom_charges[a] * self.atom_charges[b] * np.sum(erfc(self.alpha * r) / r)
        return float(tot)

    def ee_const(self, ne):
        return ne * (ne - 1) / 2 * self.ijconst + ne * self.squareconst             # :109-110

    def ei_const(self, ne):
        return -ne * self.i_sum * self.ijconst                                      # :112-113


def ion_ion_forces(cell, ewald_gmax=EWALD_GMAX, tables=None):
    """(A, 3) float64: -d E_ii / d R_a of the ion-ion Ewald energy `EwaldTables.ion_ion` (reference `_ewald_ion`), the minimal-image
    choice of every pair held fixed.  A constant of the geometry: the ion-ion part of the Hellmann-Feynman force
    (`DeviceSystem.ion_forces`).
      real space:  pair a < b, v = mi(R_a - R_b) + D_s over the 27 cells:  F_a += Z_a Z_b [erfc(alpha r)/r^2 + (2 alpha/sqrt pi)
                   exp(-alpha^2 r^2)/r] v/r,  F_b -= the same
      reciprocal:  F_a = 2 Z_a sum_G w_G G (Re S sin(G.R_a) - Im S cos(G.R_a)),  S = sum_b Z_b exp(i G.R_b)
    The constants of the energy do not depend on the positions."""
    from scipy.special import erfc
    t = tables if tables is not None else EwaldTables(cell, ewald_gmax)
    q, R, al = t.atom_charges, t.atom_coords, t.alpha
    n = len(q)
    F = np.zeros((n, 3))
    shifts = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing='ij'), -1).reshape(-1, 3) @ t.latvec
    for a in range(n):
        for b in range(a + 1, n):
            d = distance.minimal_image_host(t.latvec, t.dist_mode, R[a] - R[b])
            v = d[None, :] + shifts
            r = np.linalg.norm(v, axis=1)
            f = (erfc(al * r) / r ** 2 + 2 * al / np.sqrt(np.pi) * np.exp(-(al * r) ** 2) / r) / r
            pair = q[a] * q[b] * (f[:, None] * v).sum(axis=0)
            F[a] += pair
            F[b] -= pair
    gr = t.gpoints @ R.T                                                           # (NG, A)
    m = t.gweight[:, None] * (t.ion_exp.real[:, None] * np.sin(gr) - t.ion_exp.imag[:, None] * np.cos(gr))
    F += 2 * q[:, None] * (m.T @ t.gpoints)
    return F


VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))      # the component order xx, yy, zz, yz, xz, xy of `ds_stress`


def reciprocal_strain_weights(gpoints, gweight, alpha):
    """(NG, 3, 3): d w_G / d eps_ab = w_G [-delta_ab + 2 G_a G_b (1 / G^2 + 1 / (4 alpha^2))] under G -> G (1 + eps)^-1,
    V -> V (1 + tr eps) at fixed alpha."""
    g2 = np.einsum('gk,gk->g', gpoints, gpoints)
    f = 2.0 * (1.0 / g2 + 0.25 / alpha ** 2)
    return gweight[:, None, None] * (f[:, None, None] * gpoints[:, :, None] * gpoints[:, None, :] - np.eye(3)[None])


def ion_ion_stress(cell, ewald_gmax=EWALD_GMAX, tables=None):
    """(3, 3) float64, symmetric, in Hartree: d E_ii / d eps_ab of the ion-ion Ewald energy `EwaldTables.ion_ion + ii_const` under a
    homogeneous strain of the cell, with alpha, the integer G list and the minimal-image choice of every pair held fixed (DESIGN.md
    section 23).  A constant of the geometry: the ion-ion part of the stress (`DeviceSystem.stress`), which is this over the volume.
      real space:  pair a < b, v = mi(R_a - R_b) + D_s over the 27 cells:  Z_a Z_b f'(r) v_a v_b / r,
                   f'(r) = -[erfc(alpha r)/r^2 + (2 alpha/sqrt pi) exp(-alpha^2 r^2)/r]
      reciprocal:  sum_G dw_G |S_ion(G)|^2  (`reciprocal_strain_weights`; the phases G.R do not change)
      constants:   d(ii_const) = -[(sum Z)^2 / 2] ijconst delta_ab  (the -alpha / sqrt pi of squareconst has no derivative)"""
    from scipy.special import erfc
    t = tables if tables is not None else EwaldTables(cell, ewald_gmax)
    q, R, al = t.atom_charges, t.atom_coords, t.alpha
    n = len(q)
    out = np.zeros((3, 3))
    shifts = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing='ij'), -1).reshape(-1, 3) @ t.latvec
    for a in range(n):
        for b in range(a + 1, n):
            d = distance.minimal_image_host(t.latvec, t.dist_mode, R[a] - R[b])
            v = d[None, :] + shifts
            r = np.linalg.norm(v, axis=1)
            h = -(erfc(al * r) / r ** 2 + 2 * al / np.sqrt(np.pi) * np.exp(-(al * r) ** 2) / r) / r
            out += q[a] * q[b] * np.einsum('s,sa,sb->ab', h, v, v)
    out += np.einsum('g,gab->ab', np.abs(t.ion_exp) ** 2, reciprocal_strain_weights(t.gpoints, t.gweight, al))
    out -= 0.5 * t.i_sum ** 2 * t.ijconst * np.eye(3)
    return 0.5 * (out + out.T)                     # (symmetric to the last bit, whatever order the contractions summed in)


class EwaldSum(EwaldTables):
    """Reference-shaped class: ``energy(configs)`` -> (ee, ei, ii) on the GPU.

    ``configs`` is a torch tensor on the device, (3N,) or (B, 3N)."""

    def __init__(self, cell, ewald_gmax=EWALD_GMAX, nlatvec=1, dtype=None):
        if nlatvec != 1:
            raise ValueError('the device kernel sums the 27 neighbour cells (nlatvec=1), like every reference caller')
        super().__init__(cell, ewald_gmax)
        self._cell = cell
        self._dtype = dtype
        self._system = None

    def _sys(self, like):
        from .device import DeviceSystem
        if self._system is None:
            self._system = DeviceSystem.for_ewald(self._cell, tables=self, dtype=self._dtype or like.dtype)
        return self._system

    def energy(self, configs):
        single = configs.dim() == 1
        out = self._sys(configs).ewald(configs.reshape(1, -1) if single else configs)
        if single:
            return out[0, 0], out[0, 1], out[0, 2]
        return out[:, 0], out[:, 1], out[:, 2]
