"""Shared by test_hf_cpu.py, test_gpu_hf.py and tools/find_hf_sampler_seed.py: an independent numpy restatement of the
Hartree-Fock crystalline orbitals of deepsolid_amd/hf.py (reference hf.py:106-153 with PySCF's `PBCGTOval_sph` conventions), the
made-up test systems, and the replay of the HF-density sampler.

The machines this is tested on have no PySCF, so nothing here is a reference-executed number.  The restatement is pinned by
evaluating every AO in two ways that share no algorithm: the direct sum over lattice images (`ao_direct`), primitive by primitive,
and the Poisson / Hecke-Bochner form in reciprocal space (`ao_recip`),

    ao_k(r) = (1/V) sum_G (-i/2 alpha)^l S_lm(G + k) (pi/alpha)^(3/2) exp(-|G + k|^2 / 4 alpha) exp(i (G + k).(r - R_atom))

per primitive: the Fourier transform of S_lm(d) exp(-alpha d^2) is (-i/2 alpha)^l S_lm(q) (pi/alpha)^(3/2) exp(-q^2/4 alpha) for a
solid harmonic S_lm, and the Bloch sum over L of a function is the sum over G of its transform at G + k, over the cell volume.
The basis tables are made up, with exponents in 0.12 .. 2.0, so that the reciprocal sum converges with a few thousand G vectors.
"""
import functools
import math

import numpy as np

PI = math.pi


def solid_harmonics(l, v):
    """Real solid harmonics, orthonormal on the sphere, at vectors v (..., 3) -> (..., 2l + 1); l = 1: x, y, z;
    l = 2: xy, yz, z^2, xz, x^2 - y^2."""
    v = np.asarray(v, dtype=np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    if l == 0:
        return np.full(v.shape[:-1] + (1,), 1.0 / (2.0 * math.sqrt(PI)))
    if l == 1:
        return math.sqrt(3.0 / (4.0 * PI)) * np.stack([x, y, z], axis=-1)
    if l == 2:
        c = math.sqrt(15.0 / (4.0 * PI))
        return np.stack([c * x * y, c * y * z, math.sqrt(5.0 / (16.0 * PI)) * (2 * z * z - x * x - y * y), c * x * z,
                         0.5 * c * (x * x - y * y)], axis=-1)
    raise ValueError(l)


def lattice_points(a, rcut):
    """Every integer combination n a with |n a| <= rcut, by brute force over the bounding box of the sphere."""
    a = np.asarray(a, dtype=np.float64)
    b = np.linalg.inv(a)                                   # n_j = L . b[:, j]
    nmax = np.ceil(rcut * np.linalg.norm(b, axis=0)).astype(int) + 1
    rng = [np.arange(-m, m + 1) for m in nmax]
    n = np.array(np.meshgrid(*rng, indexing='ij')).reshape(3, -1).T
    L = n @ a
    d = np.sqrt((L * L).sum(-1))
    keep = d <= rcut
    order = np.argsort(d[keep], kind='stable')
    return L[keep][order]


def body_diagonal(a):
    a = np.asarray(a, dtype=np.float64)
    return max(np.linalg.norm(np.array(s) @ a) for s in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1)))


class System:
    """A made-up HF solution: primitive cell a, atoms, shells [(atom, l, exps, applied coefs)], kpts, mo[spin][k] (nao, n_occ)."""

    def __init__(self, a, atoms, shells, kpts, nocc, seed, precision=1e-16):
        self.a = np.asarray(a, dtype=np.float64)
        self.atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
        self.shells = [(int(at), int(l), np.asarray(e, dtype=np.float64), np.asarray(c, dtype=np.float64)) for at, l, e, c in shells]
        self.kpts = np.asarray(kpts, dtype=np.float64).reshape(-1, 3)
        self.nocc = np.asarray(nocc, dtype=int)
        self.nelec = tuple(int(v) for v in self.nocc.sum(axis=1))
        self.nao = sum(2 * l + 1 for _, l, _, _ in self.shells)
        self.alpha_min = min(float(e.min()) for _, _, e, _ in self.shells)
        self.alpha_max = max(float(e.max()) for _, _, e, _ in self.shells)
        self.images = lattice_points(self.a, math.sqrt(math.log(1.0 / precision) / self.alpha_min) + body_diagonal(self.a))
        # random complex MO coefficients, scaled so that the orbital values are O(1): unit rms over points spread over the cell
        rng = np.random.default_rng(seed)
        pts = rng.uniform(size=(40, 3)) @ self.a
        ao = ao_direct(self, pts)
        self.mo = []
        for s in range(2):
            blocks = []
            for k in range(self.kpts.shape[0]):
                c = rng.normal(size=(self.nao, self.nocc[s, k])) + 1j * rng.normal(size=(self.nao, self.nocc[s, k]))
                if c.shape[1]:
                    c = c / np.sqrt((np.abs(ao[k] @ c) ** 2).mean(axis=0))[None, :]
                blocks.append(c)
            self.mo.append(blocks)

    def gaussian_orbitals(self, images='own', **kw):
        """The object under test.  images='own': this helper's translations; None: the package's default_images."""
        from deepsolid_amd import hf
        return hf.GaussianOrbitals(self.a, self.atoms, self.shells, self.kpts, self.mo, self.nelec,
                                   images=self.images if isinstance(images, str) else images, **kw)


def ao_direct(sysm, r, kpts=None, images=None):
    """Direct image sum at points r (P, 3) that lie INSIDE the primitive cell (no wrap) -> (n_k, P, nao) complex128."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    kpts = sysm.kpts if kpts is None else np.asarray(kpts, dtype=np.float64).reshape(-1, 3)
    L = sysm.images if images is None else images
    bloch = np.exp(1j * kpts @ L.T)                        # (n_k, n_L)
    out = np.zeros((kpts.shape[0], r.shape[0], sysm.nao), dtype=np.complex128)
    col = 0
    for at, l, exps, coefs in sysm.shells:
        for p0 in range(0, r.shape[0], 128):
            d = r[p0:p0 + 128, None, :] - sysm.atoms[at][None, None, :] - L[None, :, :]
            d2 = (d * d).sum(-1)
            ylm = solid_harmonics(l, d)                    # (p, n_L, m)
            for al, c in zip(exps, coefs):                 # primitive by primitive
                g = c * np.exp(-al * d2)[..., None] * ylm
                out[:, p0:p0 + 128, col:col + 2 * l + 1] += np.einsum('kl,plm->kpm', bloch, g)
        col += 2 * l + 1
    return out


def ao_recip(sysm, r, kpts=None, tol=1e-16):
    """The same AOs from the reciprocal-space sum, every primitive truncated where exp(-|G + k|^2 / 4 alpha) < tol."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    kpts = sysm.kpts if kpts is None else np.asarray(kpts, dtype=np.float64).reshape(-1, 3)
    recip = 2 * PI * np.linalg.inv(sysm.a).T               # rows b_j
    vol = abs(np.linalg.det(sysm.a))
    kmax = float(np.linalg.norm(kpts, axis=1).max())
    G = lattice_points(recip, math.sqrt(4 * sysm.alpha_max * math.log(1.0 / tol)) + kmax)
    out = np.zeros((kpts.shape[0], r.shape[0], sysm.nao), dtype=np.complex128)
    for ik, k in enumerate(kpts):
        q = G + k
        q2 = (q * q).sum(-1)
        col = 0
        for at, l, exps, coefs in sysm.shells:
            ylm = solid_harmonics(l, q)                    # (n_G, m)
            wave = np.exp(1j * (r - sysm.atoms[at]) @ q.T)  # (P, n_G)
            for al, c in zip(exps, coefs):
                w = c * (-1j / (2 * al)) ** l * (PI / al) ** 1.5 * np.exp(-q2 / (4 * al)) / vol
                out[ik, :, col:col + 2 * l + 1] += wave @ (w[:, None] * ylm)
            col += 2 * l + 1
    return out, G.shape[0]


def wrap(a, r):
    """r (P, 3) -> (r inside the cell, integer cell index n) with r = inside + n a."""
    n = np.floor(np.linalg.solve(np.asarray(a).T, np.asarray(r, dtype=np.float64).T).T)
    return r - n @ a, n


def orb_mats(sysm, x):
    """hf.py:136-153 with the helper's AOs: x (B, 3N) or (B, N, 3) -> [up (B, n_up, n_up), dn (B, n_dn, n_dn)] complex128."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    N = sum(sysm.nelec)
    r = x.reshape(B * N, 3)
    inside, n = wrap(sysm.a, r)
    ao = ao_direct(sysm, inside) * np.exp(1j * sysm.kpts @ (n @ sysm.a).T)[:, :, None]
    ao = ao.reshape(sysm.kpts.shape[0], B, N, sysm.nao)
    out, i0 = [], 0
    for s in range(2):
        ne = sysm.nelec[s]
        cols = [ao[k, :, i0:i0 + ne, :] @ sysm.mo[s][k] for k in range(sysm.kpts.shape[0])]
        out.append(np.concatenate(cols, axis=-1).reshape(B, ne, ne))
        i0 += ne
    return out


def slogdet(sysm, x):
    """-> (phase (B,), log|det| (B,)) of the product of the spin determinants."""
    phase, logabs = 1.0, 0.0
    for m in orb_mats(sysm, x):
        if m.shape[-1]:
            p, l = np.linalg.slogdet(m)
            phase, logabs = phase * p, logabs + l
    return phase, logabs


# ------------------------------------------------------------------------------------------------------------ the test systems
def _norm(l, exps, coefs):
    from deepsolid_amd import hf
    return hf.normalize_shell(l, exps, coefs)


def _shell(at, l, exps, coefs=None):
    return (at, l, np.asarray(exps, dtype=np.float64), _norm(l, exps, np.ones(len(exps)) if coefs is None else coefs))


@functools.lru_cache(maxsize=None)
def lih_cell():
    """The simulation cell of the LiH-like system: rock-salt primitive fcc cell, 2 x 1 x 1 supercell, nelec = (4, 4)."""
    from deepsolid_amd import systems
    return systems.build('lih', S=np.diag([2, 1, 1]))[0]


@functools.lru_cache(maxsize=None)
def lih_system():
    """LiH-like: Li s, s (3 primitives), p; H s -> 6 AOs; the two k points of the 2 x 1 x 1 supercell, two bands each per spin."""
    from deepsolid_amd.supercell import get_supercell_kpts
    cell = lih_cell()
    prim = cell.original_cell
    shells = [_shell(0, 0, [0.6]), _shell(0, 0, [1.8, 0.45, 0.13], [0.3, 0.5, 0.4]), _shell(0, 1, [0.35]), _shell(1, 0, [0.25])]
    return System(prim.lattice_vectors(), prim.atom_coords(), shells, get_supercell_kpts(cell), [[2, 2], [2, 2]], seed=11)


def hex_cell_vectors(L=4.65, z=20.0):
    return np.array([[L * math.cos(PI / 6), -0.5 * L, 0.0], [L * math.cos(PI / 6), 0.5 * L, 0.0], [0.0, 0.0, z]])


@functools.lru_cache(maxsize=None)
def hex_system(nelec=(5, 4), wide_images=False):
    """Hexagonal two-atom cell with 20 Bohr of vacuum; s, p, d on either atom -> 18 AOs; the three k points of a 3 x 1 x 1
    supercell shifted by a twist; nelec (5, 4) or (3, 0).  wide_images: translations out to 1.6 x the radius needed, sorted by
    length -- the far chunks of such a list are the ones the kernel's screening skips."""
    a = hex_cell_vectors()
    atoms = np.array([[3 ** -0.5 * 4.65, 0.0, 0.0], [2 * 3 ** -0.5 * 4.65, 0.0, 0.0]])
    shells = []
    for at in (0, 1):
        shells += [_shell(at, 0, [1.2, 0.3], [0.4, 0.7]), _shell(at, 1, [0.5]), _shell(at, 2, [0.8 - 0.3 * at])]
    recip = 2 * PI * np.linalg.inv(a).T
    twist = np.array([0.13, 0.29, 0.41])
    kpts = np.array([(j / 3.0) * recip[0] for j in range(3)]) + (twist / np.array([3.0, 1.0, 1.0])) @ recip
    nocc = {(5, 4): [[2, 2, 1], [2, 1, 1]], (3, 0): [[1, 1, 1], [0, 0, 0]]}[tuple(nelec)]
    s = System(a, atoms, shells, kpts, nocc, seed=23)
    if wide_images:
        s.images = lattice_points(a, 1.6 * (math.sqrt(math.log(1e16) / s.alpha_min) + body_diagonal(a)))
    return s


@functools.lru_cache(maxsize=None)
def pin_system(kind):
    """The two cells of the direct-against-reciprocal pin, each with s (contracted), p and d shells on two atoms:
    'triclinic' (no symmetry at all) and 'fcc' (the rock-salt primitive cell)."""
    if kind == 'triclinic':
        a = np.array([[5.0, 0.3, 0.2], [1.1, 4.6, -0.4], [0.7, -0.9, 5.2]])
        atoms = np.array([[0.4, 0.3, 0.2], [2.9, 2.2, 3.1]])
    else:
        prim = lih_cell().original_cell
        a, atoms = prim.lattice_vectors(), prim.atom_coords()
    shells = [_shell(0, 0, [1.6, 0.5, 0.14], [0.2, 0.6, 0.3]), _shell(0, 1, [0.9, 0.2], [0.5, 0.5]), _shell(0, 2, [0.6]),
              _shell(1, 0, [0.33]), _shell(1, 1, [0.45]), _shell(1, 2, [1.3, 0.25], [0.4, 0.6])]
    return System(a, atoms, shells, np.zeros((1, 3)), [[1], [1]], seed=3)


def walkers(sysm, B, seed, spread=0.0, sim_a=None):
    """(B, 3N) walkers uniform in the cell `sim_a` (default: the primitive cell), shifted by integer cells up to +-spread."""
    rng = np.random.default_rng(seed)
    a = sysm.a if sim_a is None else np.asarray(sim_a, dtype=np.float64)
    N = sum(sysm.nelec)
    f = rng.uniform(size=(B, N, 3))
    if spread:
        f = f + rng.integers(-int(spread), int(spread) + 1, size=(B, N, 3))
    return (f @ a).reshape(B, 3 * N)


# ------------------------------------------------------------------------------------------------- replay of the HF-density sampler
SAMPLER_BATCH, SAMPLER_NSTEPS, SAMPLER_ITERATIONS, SAMPLER_WIDTH = 32, 3, 2, 0.02
SAMPLER_MARGIN = 1e-6
SAMPLER_SEED = 1          # tools/find_hf_sampler_seed.py


def sampler_noise(seed, N):
    rng = np.random.default_rng(seed)
    normals = rng.normal(size=(SAMPLER_ITERATIONS, SAMPLER_NSTEPS, SAMPLER_BATCH, 3 * N))
    uniforms = rng.uniform(size=(SAMPLER_ITERATIONS, SAMPLER_NSTEPS, SAMPLER_BATCH))
    return normals, uniforms


def sampler_start(sysm, sim_a):
    return walkers(sysm, SAMPLER_BATCH, seed=5, sim_a=sim_a)


def replay_sampler(sysm, sim_a, x0, normals, uniforms, width=SAMPLER_WIDTH, trace=None):
    """qmc.mh_update's symmetric branch (qmc.py:190-196, 217-222) on lp = 2 log|det_HF|, move after move, in float64 numpy.
    -> (final walkers, decisions (iterations, nsteps, B) bool, margins lp2 - lp1 - log u of the same shape); `trace`: a list that
    receives the walkers after every move."""
    sim_a = np.asarray(sim_a, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    lp = 2.0 * slogdet(sysm, x)[1]
    dec = np.zeros(uniforms.shape, dtype=bool)
    margin = np.zeros(uniforms.shape)
    for t in range(normals.shape[0]):
        for i in range(normals.shape[1]):
            prop = (x + width * normals[t, i]).reshape(-1, 3)
            x2 = wrap(sim_a, prop)[0].reshape(x.shape)
            lp2 = 2.0 * slogdet(sysm, x2)[1]
            margin[t, i] = lp2 - lp - np.log(uniforms[t, i])
            dec[t, i] = margin[t, i] > 0
            x = np.where(dec[t, i][:, None], x2, x)
            lp = np.where(dec[t, i], lp2, lp)
            if trace is not None:
                trace.append(x.copy())
    return x, dec, margin
