"""Hartree-Fock crystalline orbitals from plain arrays (reference DeepSolid/hf.py:84-165 without PySCF at run time).

`GaussianOrbitals` holds what the reference's `hf.SCF` knows after `init_scf()` -- the primitive cell, a contracted Gaussian
basis, the k points and the occupied MO coefficients per spin and k point -- and evaluates the occupied crystalline orbitals
at a batch of walkers on the GPU (`ds_hf_orbitals`, csrc/ds_hf.h).  PySCF is needed once, offline, to dump the arrays
(INTEGRATION.md); `save` / `load` keep them in one `.npz` of numbers only.

Conventions: those of PySCF's `PBCGTOval_sph`, restated here.  This package has never been run next to PySCF -- the machines
it is developed and tested on have none -- so compatibility with a real export holds by these stated conventions only; the
tests pin them against an independent reciprocal-space sum (tests/hf_helpers.py), not against PySCF.

    ao_k,mu(r) = sum_L exp(i k.L) R_mu(|d|) S_lm(d),      d = r - R_atom(mu) - L,      R(|d|) = sum_p c_p exp(-alpha_p |d|^2)

  * S_lm are the real solid harmonics that are orthonormal on the sphere:
      l = 0:  1 / (2 sqrt(pi))
      l = 1:  sqrt(3/4pi) (x, y, z), in this order
      l = 2:  sqrt(15/4pi) xy, sqrt(15/4pi) yz, sqrt(5/16pi) (3z^2 - r^2), sqrt(15/4pi) xz, sqrt(15/16pi) (x^2 - y^2), in this order
  * the coefficients c_p are the ones APPLIED, normalisation included (`normalize_shell` makes them from basis-set tables);
  * AO index: shells in the order given, m inside a shell in the order above;
  * the walker is first wrapped into the primitive cell and the AO multiplied by exp(i k.(wrap a))             (hf.py:113-120);
  * the orbital matrix of spin s is [walker, electron of that spin, orbital], orbitals ordered by k point and then by band
    within k (hf.py:131-134, :148-152) -- the order of `klist` (hf.py:102-104).

Not provided: `kinetic`, `laplacian` and `eval_inverse` of the reference's class.  They need second-derivative AOs, and nothing
in the drivers uses them.
"""
import math

import numpy as np
import torch

MAX_L = 2
MAX_AO = 128
MAX_K = 64
MAX_ELEC_PER_SPIN = 64

_S0 = 0.5 / math.sqrt(math.pi)
_S1 = math.sqrt(3.0 / (4.0 * math.pi))
_D_XY = math.sqrt(15.0 / (4.0 * math.pi))
_D_Z2 = math.sqrt(5.0 / (16.0 * math.pi))
_D_X2Y2 = math.sqrt(15.0 / (16.0 * math.pi))


def _radial_norm2(l, exps, coefs):
    """int_0^inf r^(2l+2) (sum_p c_p exp(-alpha_p r^2))^2 dr, with int r^(2l+2) e^(-s r^2) dr = Gamma(l+3/2) / (2 s^(l+3/2))."""
    s = exps[:, None] + exps[None, :]
    return float(np.sum(coefs[:, None] * coefs[None, :] * math.gamma(l + 1.5) / (2.0 * s ** (l + 1.5))))


def normalize_shell(l, exps, coefs):
    """Raw basis-set table -> applied coefficients with int |chi|^2 d^3r = 1 in free space.  As basis-set tables mean it (and as
    PySCF applies it): `coefs` multiply primitives that are normalised each on its own, and the contraction is then normalised
    as a whole.  The angular factors S_lm are orthonormal on the sphere, so the norm is the radial integral alone."""
    exps = np.asarray(exps, dtype=np.float64).reshape(-1)
    coefs = np.asarray(coefs, dtype=np.float64).reshape(-1)
    if exps.shape != coefs.shape or exps.size == 0 or np.any(exps <= 0):
        raise ValueError('normalize_shell: exponents must be positive, one coefficient each')
    prim = np.array([1.0 / math.sqrt(_radial_norm2(l, exps[i:i + 1], np.ones(1))) for i in range(exps.size)])
    c = coefs * prim
    return c / math.sqrt(_radial_norm2(l, exps, c))


def default_images(a, exps, precision=1e-12):
    """Every lattice vector L = n a with |L| <= sqrt(ln(1/precision) / alpha_min) + D, D the longest body diagonal of the cell:
    for r and the atom inside the cell |r - R - L| >= |L| - D, so an image left out contributes less than `precision` times the
    coefficient.  Sorted by |L| (then by n), so that the far images, which the kernel may skip in chunks, come last."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    amin = float(np.min(np.asarray(exps, dtype=np.float64)))
    diag = max(np.linalg.norm(s @ a) for s in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1)))
    rcut = math.sqrt(math.log(1.0 / precision) / amin) + diag
    # |n_j| = |L . ainv[:, j]| <= |L| |ainv[:, j]|
    nmax = np.floor(rcut * np.linalg.norm(np.linalg.inv(a), axis=0) + 1e-9).astype(int)
    grids = np.meshgrid(*[np.arange(-m, m + 1) for m in nmax], indexing='ij')
    n = np.stack([g.reshape(-1) for g in grids], axis=1)
    L = n @ a
    norm = np.linalg.norm(L, axis=1)
    keep = norm <= rcut
    n, L, norm = n[keep], L[keep], norm[keep]
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], np.round(norm, 9)))
    return np.ascontiguousarray(L[order])


class GaussianOrbitals:
    """PySCF-free stand-in for the reference's `hf.SCF` after `init_scf()`; see the module docstring for the conventions.

    a (3, 3): primitive cell, rows = lattice vectors, Bohr.  atoms (A, 3): coordinates, Bohr.
    shells: one `(atom index, l, exponents, applied coefficients)` per shell, l in {0, 1, 2}.
    kpts (n_k, 3).  mo_coeff: `mo_coeff[spin][k]` is the (nao, n_occ[spin][k]) complex block of OCCUPIED orbitals.
    nelec: (n_up, n_dn) of the simulation cell; the occupations must sum to it.
    images (n_L, 3), optional: the lattice translations to sum over (e.g. PySCF's `cell.get_lattice_Ls()` verbatim); else
    `default_images(a, exponents, precision)`.

    Refused at construction: l > 2, more than 128 AOs, more than 64 k points, more than 64 electrons per spin, occupations
    that do not sum to `nelec`."""

    on_device = True        # the pretraining loops hand it the walkers where they are (no host round trip)

    def __init__(self, a, atoms, shells, kpts, mo_coeff, nelec, images=None, precision=1e-12):
        self.a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(3, 3))
        self.atoms = np.ascontiguousarray(np.asarray(atoms, dtype=np.float64).reshape(-1, 3))
        if self.atoms.shape[0] < 1:
            raise ValueError('GaussianOrbitals: no atoms')
        if abs(np.linalg.det(self.a)) < 1e-12:
            raise ValueError('GaussianOrbitals: the lattice vectors are linearly dependent')
        self.shells = []
        for i, (at, l, ex, co) in enumerate(shells):
            at, l = int(at), int(l)
            ex = np.asarray(ex, dtype=np.float64).reshape(-1)
            co = np.asarray(co, dtype=np.float64).reshape(-1)
            if not 0 <= l <= MAX_L:
                raise ValueError(f'GaussianOrbitals: shell {i} has l = {l}; only s, p and d shells (l <= {MAX_L}) are provided')
            if not 0 <= at < self.atoms.shape[0]:
                raise ValueError(f'GaussianOrbitals: shell {i} names atom {at} of {self.atoms.shape[0]}')
            if ex.size == 0 or ex.shape != co.shape or np.any(ex <= 0) or not (np.all(np.isfinite(ex)) and np.all(np.isfinite(co))):
                raise ValueError(f'GaussianOrbitals: shell {i} needs positive exponents with one finite coefficient each')
            self.shells.append((at, l, ex, co))
        if not self.shells:
            raise ValueError('GaussianOrbitals: no shells')
        self.nao = sum(2 * l + 1 for _, l, _, _ in self.shells)
        if self.nao > MAX_AO:
            raise ValueError(f'GaussianOrbitals: {self.nao} atomic orbitals; at most {MAX_AO} are provided')
        self.kpts = np.ascontiguousarray(np.asarray(kpts, dtype=np.float64).reshape(-1, 3))
        n_k = self.kpts.shape[0]
        if not 1 <= n_k <= MAX_K:
            raise ValueError(f'GaussianOrbitals: {n_k} k points; 1..{MAX_K} are provided')
        self.nelec = (int(nelec[0]), int(nelec[1]))
        if max(self.nelec) > MAX_ELEC_PER_SPIN or min(self.nelec) < 0 or sum(self.nelec) < 1:
            raise ValueError(f'GaussianOrbitals: nelec = {self.nelec}; 0..{MAX_ELEC_PER_SPIN} electrons per spin (one at least) are provided')
        if len(mo_coeff) != 2 or any(len(m) != n_k for m in mo_coeff):
            raise ValueError('GaussianOrbitals: mo_coeff must be [spin][k] with 2 spins and one block per k point')
        self.mo_coeff = []
        for s in range(2):
            blocks = [np.asarray(m, dtype=np.complex128).reshape(self.nao, -1) if np.size(m) else np.zeros((self.nao, 0), np.complex128)
                      for m in mo_coeff[s]]
            self.mo_coeff.append(blocks)
        self.nocc = np.array([[m.shape[1] for m in blocks] for blocks in self.mo_coeff], dtype=np.int32)
        for s in range(2):
            if int(self.nocc[s].sum()) != self.nelec[s]:
                raise ValueError(f'GaussianOrbitals: spin {s} has {int(self.nocc[s].sum())} occupied orbitals over the k points '
                                 f'but nelec[{s}] = {self.nelec[s]}')
        exps_all = np.concatenate([ex for _, _, ex, _ in self.shells])
        self.images = np.ascontiguousarray(default_images(self.a, exps_all, precision) if images is None
                                           else np.asarray(images, dtype=np.float64).reshape(-1, 3))
        if self.images.shape[0] < 1:
            raise ValueError('GaussianOrbitals: no lattice images')
        for name, v in (('a', self.a), ('atoms', self.atoms), ('kpts', self.kpts), ('images', self.images)):
            if not np.all(np.isfinite(v)):
                raise ValueError(f'GaussianOrbitals: `{name}` holds a value that is not finite')
        if not all(np.all(np.isfinite(m)) for blocks in self.mo_coeff for m in blocks):
            raise ValueError('GaussianOrbitals: `mo_coeff` holds a value that is not finite')
        # hf.py:99-104: per spin, the k point of every orbital
        self.klist = [np.concatenate([np.tile(k[None, :], (int(n), 1)) for k, n in zip(self.kpts, self.nocc[s])]).reshape(-1, 3)
                      for s in range(2)]
        self._tables = {}

    # ---- file format: one .npz of numbers only ------------------------------------------------------------------------
    def _arrays(self):
        return {
            'a': self.a, 'atoms': self.atoms,
            'shell_atom': np.array([s[0] for s in self.shells], dtype=np.int32),
            'shell_l': np.array([s[1] for s in self.shells], dtype=np.int32),
            'shell_nprim': np.array([s[2].size for s in self.shells], dtype=np.int32),
            'exps': np.concatenate([s[2] for s in self.shells]), 'coefs': np.concatenate([s[3] for s in self.shells]),
            'kpts': self.kpts, 'nelec': np.array(self.nelec, dtype=np.int32), 'nocc': self.nocc,
            'mo_up': np.concatenate(self.mo_coeff[0], axis=1), 'mo_dn': np.concatenate(self.mo_coeff[1], axis=1),
            'images': self.images,
        }

    def save(self, path):
        """One `.npz` holding the arrays of `ds_hf_desc` (include/deepsolid_hip.h) under their names there, plus `nelec` and
        `nocc` (2, n_k); `mo_up` / `mo_dn` are (nao, n_s) complex128 with the columns ordered by k point, then band."""
        with open(path, 'wb') as f:
            np.savez(f, **self._arrays())

    @classmethod
    def load(cls, path):
        """Inverse of `save`.  A file without `images` gets `default_images`."""
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        off = np.concatenate([[0], np.cumsum(d['shell_nprim'])])
        shells = [(int(at), int(l), d['exps'][off[i]:off[i + 1]], d['coefs'][off[i]:off[i + 1]])
                  for i, (at, l) in enumerate(zip(d['shell_atom'], d['shell_l']))]
        mo = []
        for s, key in enumerate(('mo_up', 'mo_dn')):
            split = np.cumsum(d['nocc'][s])[:-1]
            mo.append(np.split(d[key].reshape(d[key].shape[0], -1), split, axis=1))      # (nao, n_s); n_s may be 0
        return cls(d['a'], d['atoms'], shells, d['kpts'], mo, tuple(int(n) for n in d['nelec']), images=d.get('images'))

    # ---- evaluation ---------------------------------------------------------------------------------------------------
    def _device_tables(self, device):
        from .device import HfOrbitalTables
        key = (device.type, device.index)
        if key not in self._tables:
            t = self._arrays()
            self._tables[key] = HfOrbitalTables(t['a'], t['atoms'], t['shell_atom'], t['shell_l'], t['shell_nprim'], t['exps'],
                                                t['coefs'], t['kpts'], t['images'], t['nocc'], (t['mo_up'], t['mo_dn']), device=device)
        return self._tables[key]

    def eval_aos_host(self, r):
        """Host restatement of the AOs: r (P, 3) float64 -> (n_k, P, nao) complex128, wrap phase included."""
        r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
        frac = r @ np.linalg.inv(self.a)
        wrap = np.floor(frac)
        rp = (frac - wrap) @ self.a
        bloch = np.exp(1j * self.images @ self.kpts.T)                                     # (n_L, n_k)
        ao = np.empty((self.kpts.shape[0], r.shape[0], self.nao), dtype=np.complex128)
        step = max(1, (1 << 21) // max(1, self.images.shape[0]))
        for p0 in range(0, r.shape[0], step):
            q = rp[p0:p0 + step, None, :] - self.images[None, :, :]                        # (p, n_L, 3)
            col = 0
            for at, l, ex, co in self.shells:
                d = q - self.atoms[at]
                x, y, z = d[..., 0], d[..., 1], d[..., 2]
                r2 = x * x + y * y + z * z
                rad = np.zeros_like(r2)
                for al, c in zip(ex, co):
                    rad += c * np.exp(-al * r2)
                if l == 0:
                    ang = [_S0 * rad]
                elif l == 1:
                    ang = [_S1 * rad * x, _S1 * rad * y, _S1 * rad * z]
                else:
                    ang = [_D_XY * rad * x * y, _D_XY * rad * y * z, _D_Z2 * rad * (3 * z * z - r2), _D_XY * rad * x * z,
                           _D_X2Y2 * rad * (x * x - y * y)]
                for m, chi in enumerate(ang):
                    ao[:, p0:p0 + step, col + m] = (chi @ bloch).T
                col += len(ang)
        wrap_phase = np.exp(1j * np.einsum('kc,pc->kp', self.kpts, wrap @ self.a))
        return ao * wrap_phase[:, :, None]

    def _orb_mat_host(self, x):
        B, N, _ = x.shape
        ao = self.eval_aos_host(x.reshape(-1, 3)).reshape(self.kpts.shape[0], B, N, self.nao)
        out, i0 = [], 0
        for s in range(2):
            ne = self.nelec[s]
            mo = [ao[k, :, i0:i0 + ne] @ c for k, c in enumerate(self.mo_coeff[s])]
            out.append(np.concatenate(mo, axis=-1).reshape(B, ne, ne))
            i0 += ne
        return out

    def eval_orb_mat(self, x):
        """hf.py:136-153.  x (B, N, 3) -> [up (B, n_up, n_up), dn (B, n_dn, n_dn)] complex128, [walker, electron, orbital].
        A device tensor (float64 or float32) is evaluated by the HIP kernel and stays on the device; a numpy array (or a host
        tensor) gives the host restatement, as numpy arrays (host tensors).  A channel without electrons is kept as (B, 0, 0),
        as the reference does; callers drop it."""
        n = sum(self.nelec)
        if len(x.shape) != 3 or x.shape[1] != n or x.shape[2] != 3:
            raise ValueError(f'walkers must be (B, {n}, 3), got {tuple(x.shape)}')
        if isinstance(x, torch.Tensor) and x.is_cuda:
            if x.dtype not in (torch.float64, torch.float32):
                x = x.to(torch.float64)
            return self._device_tables(x.device).orbitals(x.reshape(x.shape[0], 3 * n))
        if isinstance(x, torch.Tensor):
            return [torch.from_numpy(m) for m in self._orb_mat_host(x.detach().to(torch.float64).numpy())]
        return self._orb_mat_host(np.asarray(x, dtype=np.float64))

    def eval_orbitals_at(self, points, spin):
        """The orbitals of ONE spin at arbitrary points: points (P, 3) -> (P, M_spin) complex128, [point, orbital], columns in
        the order of `eval_orb_mat`.  A device tensor (float64 or float32) is evaluated by the HIP kernel (`ds_hf_orbitals_at`)
        and stays on the device; a numpy array (or a host tensor) gives `eval_aos_host @ mo_coeff`, as a numpy array (host
        tensor)."""
        spin = int(spin)
        if spin not in (0, 1):
            raise ValueError(f'spin must be 0 or 1, got {spin}')
        if len(points.shape) != 2 or points.shape[1] != 3:
            raise ValueError(f'points must be (P, 3), got {tuple(points.shape)}')
        if isinstance(points, torch.Tensor) and points.is_cuda:
            if points.dtype not in (torch.float64, torch.float32):
                points = points.to(torch.float64)
            return self._device_tables(points.device).orbitals_at(points, spin)
        host = isinstance(points, torch.Tensor)
        r = points.detach().to(torch.float64).numpy() if host else np.asarray(points, dtype=np.float64)
        ao = self.eval_aos_host(r)                                                         # (n_k, P, nao)
        out = np.concatenate([ao[k] @ c for k, c in enumerate(self.mo_coeff[spin])], axis=-1).reshape(r.shape[0], self.nelec[spin])
        return torch.from_numpy(out) if host else out

    def eval_slogdet(self, x):
        """hf.py:155-165: (phase, log|det|) of the product of the spin determinants, where `x` lives."""
        mats = [m for m in self.eval_orb_mat(x) if m.shape[-1] > 0]
        if isinstance(mats[0], torch.Tensor):
            phase, logabs = torch.linalg.slogdet(mats[0])
            for m in mats[1:]:
                p, l = torch.linalg.slogdet(m)
                phase, logabs = phase * p, logabs + l
            return phase, logabs
        phase, logabs = np.linalg.slogdet(mats[0])
        for m in mats[1:]:
            p, l = np.linalg.slogdet(m)
            phase, logabs = phase * p, logabs + l
        return phase, logabs

    def __call__(self, x):
        """hf.py:215-218: the value of the Slater determinant."""
        phase, logabs = self.eval_slogdet(x)
        return (torch.exp(logabs) if isinstance(logabs, torch.Tensor) else np.exp(logabs)) * phase
