"""Walker observables of the reference's estimator.py: the complex polarization (:15-42) and the structure factor S(k)
(:44-84), the two quantities the driver logs when ``cfg.log.complex_polarization`` / ``cfg.log.structure_factor`` are set
(process.py:277-283, 337-342, 361-362).

The batch sums come from one HIP call (``device.observable_sums``, csrc/ds_obs.h); what is left here is host algebra on a few
hundred numbers: per-rank means, ONE packed all-reduce of them (``constants.pmean_vector``), and
S(k) = (pmean<|rho|^2> - |pmean<rho>|^2) / N -- the reference takes the pmeans of <rho> and <|rho|^2> separately and only
then forms S(k) (:73-81), it never averages per-rank S(k).
"""
import numpy as np
import torch

from . import constants

_COMPLEX = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def structure_factor_grid(nq):
    """(nq^3, 3) integer points in the order of estimator.py:55-56: ``jnp.meshgrid`` indexes 'xy', so point
    p = i nq^2 + j nq + k is (n1, n2, n3) = (j, i, k)."""
    mesh = np.meshgrid(*[np.arange(nq) for _ in range(3)])
    return np.stack([m.ravel() for m in mesh], axis=0).T.astype(np.int32)


def combine_sums(sums, batch, n_q, polarization, nelec, dtype=torch.float64):
    """Packed batch sums of one rank (the layout of ``ds_observables``) -> (polarization or None, S(k) or None).
    Only the requested observables travel in the all-reduce; with world size 1 nothing is reduced."""
    sums = sums.to(torch.float64)
    parts = []
    if polarization:
        parts.append(sums[:2])
    if n_q:
        parts.append(sums[2:2 + 3 * n_q])
    if not parts:
        return None, None
    means = constants.pmean_vector(torch.cat(parts) / batch)
    pol = sk = None
    if polarization:
        pol = torch.complex(means[0], means[1]).to(_COMPLEX[dtype])
        means = means[2:]
    if n_q:
        one_re, one_im, two = means[:n_q], means[n_q:2 * n_q], means[2 * n_q:3 * n_q]
        sk = ((two - (one_re * one_re + one_im * one_im)) / nelec).to(dtype)
    return pol, sk


def make_observables(simulation_cell, polarization_direction=None, nq=None, ndim=3):
    """Both observables from one kernel call and one all-reduce: f(data) -> (polarization or None, S(k) or None).
    `polarization_direction` None / `nq` None switches the one off."""
    if ndim != 3:
        raise ValueError(f'ndim = {ndim}: only three-dimensional walkers are supported')
    if polarization_direction is not None and polarization_direction not in (0, 1, 2):
        raise ValueError(f'polarization direction must be 0, 1 or 2, got {polarization_direction}')
    if nq is not None and not 1 <= int(nq) <= 8:
        raise ValueError(f'nq = {nq}: the structure factor supports 1 <= nq <= 8')
    recvec = np.asarray(simulation_cell.reciprocal_vectors(), dtype=np.float64)
    nelec = int(simulation_cell.nelectron) if hasattr(simulation_cell, 'nelectron') else int(sum(simulation_cell.nelec))
    grid = structure_factor_grid(int(nq)) if nq is not None else np.zeros((0, 3), np.int32)
    pol_dir = -1 if polarization_direction is None else int(polarization_direction)

    def observables(data):
        from . import device
        if data.shape[-1] != 3 * nelec:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {nelec} electrons')
        x = data.reshape(-1, 3 * nelec)
        sums = device.observable_sums(recvec, x, grid, pol_dir)
        return combine_sums(sums, x.shape[0], grid.shape[0], pol_dir >= 0, nelec, x.dtype)

    return observables


def make_complex_polarization(simulation_cell, direction=0, ndim=3):
    """estimator.py:15-42: f(data (B, 3N)) -> complex scalar tensor, the batch (and rank) mean of exp(i g_dir . sum_e r_e)."""
    f = make_observables(simulation_cell, polarization_direction=direction, ndim=ndim)
    return lambda data: f(data)[0]


def make_structure_factor(simulation_cell, nq=4, ndim=3):
    """estimator.py:44-84: f(data (B, 3N)) -> real (nq^3,) tensor S(k) = (<|rho_k|^2> - |<rho_k>|^2) / N on the
    grid of ``structure_factor_grid(nq)``, in the dtype of the walkers."""
    f = make_observables(simulation_cell, nq=nq, ndim=ndim)
    return lambda data: f(data)[1]


def _csv_value(v):
    """One value as pandas' DataFrame.to_csv writes it (default float_format, na_rep='')."""
    if np.isnan(v):
        return ''
    return repr(float(v)) if v.dtype == np.float64 else str(v)


def append_structure_factor_row(path, sk):
    """Append S(k) to `path` exactly as process.py:339-342 does with
    ``pd.DataFrame(sk[None, :]).to_csv(path, mode='a', sep=',', header=False)``: the row index 0, then the nq^3 values."""
    sk = np.asarray(sk.detach().cpu() if isinstance(sk, torch.Tensor) else sk).reshape(-1)
    with open(path, 'a') as f:
        f.write(','.join(['0'] + [_csv_value(v) for v in sk]) + '\n')


# ------------------------------------------------------------------ real-space observables (csrc/ds_realspace.h)
# The reference has no real-space estimator; the conventions of this section are this project's own.
PAIR_CHANNELS = ('up-up', 'up-down', 'down-down')


def wigner_seitz_radius(a):
    """Half the length of the shortest non-zero lattice vector of `a` (3, 3; rows = lattice vectors), from the vectors with
    coefficients in -3..3."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    n = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(-3, 4)] * 3, indexing='ij')], axis=1)
    n = n[np.any(n != 0, axis=1)]
    return 0.5 * float(np.sqrt(((n @ a) ** 2).sum(axis=1)).min())


def plane_spacings(a):
    """The three distances between neighbouring lattice planes of `a`: spacing j = 1 / |column j of inv(a)|."""
    return 1.0 / np.sqrt((np.linalg.inv(np.asarray(a, dtype=np.float64).reshape(3, 3)) ** 2).sum(axis=0))


class _Lattices:
    """What `RealSpaceAccumulator` reads of a simulation cell, rebuilt from a saved state."""

    def __init__(self, a, nelec):
        self.a, self.nelec = np.asarray(a, dtype=np.float64), tuple(int(n) for n in nelec)
        self.original_cell = self


class RealSpaceAccumulator:
    """Spin-resolved electron density and radial pair-correlation function g(r), accumulated as integer counts on the device over
    any number of walker batches (`update`), summed over the ranks once (`reduce`) and normalised on the host.

    `density_grid`: G or (g0, g1, g2), the grid on the folding lattice `density_cell`: 'primitive'
    (``simulation_cell.original_cell.a``), 'simulation', or a 3x3 array of any lattice whose translations are symmetries; None: no
    density.  `pair_bins`: number of radial bins on [0, pair_rmax); None: no g(r).  `pair_rmax` None: the Wigner-Seitz radius
    r_ws (half the shortest lattice vector of the simulation cell).  pair_rmax > r_ws, or pair_rmax >= 1.5 x the smallest plane
    spacing (the kernel looks at the 27 nearest images only), is a ValueError."""

    def __init__(self, simulation_cell, density_grid=None, density_cell='primitive', pair_bins=None, pair_rmax=None):
        self.a = np.array(simulation_cell.a, dtype=np.float64).reshape(3, 3)
        self.nelec = (int(simulation_cell.nelec[0]), int(simulation_cell.nelec[1]))
        n = sum(self.nelec)
        if not 1 <= n <= 128 or min(self.nelec) < 0:
            raise ValueError(f'nelec = {self.nelec}: between 1 and 128 electrons are supported')
        if density_grid is None and pair_bins is None:
            raise ValueError('RealSpaceAccumulator: neither density_grid nor pair_bins was given')
        self.grid = self.fold = None
        if density_grid is not None:
            g = np.asarray(density_grid)
            if g.ndim > 1 or g.size not in (1, 3) or not np.all(g == np.floor(g)):
                raise ValueError(f'density_grid must be an integer or three integers, got {density_grid!r}')
            g = tuple(int(v) for v in (np.repeat(g.reshape(-1), 3) if g.size == 1 else g))
            if min(g) < 1 or max(g) > 256 or g[0] * g[1] * g[2] > 1 << 22:
                raise ValueError(f'density_grid = {g}: 1 <= g_j <= 256 and g0 g1 g2 <= 2^22 are supported')
            self.grid = g
            if isinstance(density_cell, str):
                if density_cell == 'primitive':
                    fold = simulation_cell.original_cell.a
                elif density_cell == 'simulation':
                    fold = simulation_cell.a
                else:
                    raise ValueError(f"density_cell must be 'primitive', 'simulation' or a 3x3 array, got {density_cell!r}")
            else:
                fold = density_cell
            fold = np.array(fold, dtype=np.float64)
            if fold.shape != (3, 3) or not np.all(np.isfinite(fold)) or abs(np.linalg.det(fold)) < 1e-12:
                raise ValueError('density_cell must be a non-singular 3x3 lattice')
            self.fold = fold
        self.n_r = self.r_max = None
        self.r_ws, self.spacings = wigner_seitz_radius(self.a), plane_spacings(self.a)
        if pair_bins is not None:
            if int(pair_bins) != pair_bins or not 1 <= int(pair_bins) <= 1024:
                raise ValueError(f'pair_bins = {pair_bins!r}: 1 <= pair_bins <= 1024 is supported')
            r_max = self.r_ws if pair_rmax is None else float(pair_rmax)
            if not (r_max > 0 and np.isfinite(r_max)):
                raise ValueError(f'pair_rmax = {pair_rmax!r} must be positive')
            if r_max > self.r_ws:
                raise ValueError(f'pair_rmax = {r_max} is beyond the Wigner-Seitz radius {self.r_ws} of the simulation cell: '
                                 'more than one image of a pair could be counted')
            if not r_max < 1.5 * self.spacings.min():
                raise ValueError(f'pair_rmax = {r_max} is not below 1.5 x the smallest plane spacing {self.spacings.min()}: '
                                 'the nearest image may lie outside the 27 shifts the kernel searches')
            self.n_r, self.r_max = int(pair_bins), r_max
        elif pair_rmax is not None:
            raise ValueError('pair_rmax without pair_bins')
        self.dens = self.pair = None        # int64 tensors (2, g0, g1, g2) / (3, n_r), made on the walkers' device by the first update
        self.n_walkers = 0
        self.reduced = False

    # ---- accumulation
    def _buffers(self, device):
        if self.grid is not None:
            self.dens = torch.zeros((2,) + self.grid, dtype=torch.int64, device=device) if self.dens is None \
                else self.dens.to(device)
        if self.n_r is not None:
            self.pair = torch.zeros((3, self.n_r), dtype=torch.int64, device=device) if self.pair is None else self.pair.to(device)

    def update(self, data):
        """Add the walkers `data` (B, 3N) to the counts: one kernel call, no device -> host copy."""
        from . import device
        if self.reduced:
            raise RuntimeError('RealSpaceAccumulator.update after reduce(): the counts are already summed over the ranks')
        n = sum(self.nelec)
        if data.shape[-1] != 3 * n:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {n} electrons')
        x = data.reshape(-1, 3 * n)
        if not x.is_cuda:
            raise RuntimeError('RealSpaceAccumulator.update: walkers must live on the ROCm device (no CPU path)')
        self._buffers(x.device)
        device.realspace_counts(x, self.nelec[0], dens=self.dens, fold_lattice=self.fold, pair=self.pair, latvec=self.a,
                                r_max=self.r_max)
        self.n_walkers += int(x.shape[0])

    def _same_setup(self, other):
        same = lambda p, q: (p is None) == (q is None) and (p is None or np.array_equal(np.asarray(p), np.asarray(q)))
        return all(same(getattr(self, k), getattr(other, k)) for k in ('a', 'nelec', 'grid', 'fold', 'n_r', 'r_max'))

    def merge(self, other):
        """Add the counts and the walker number of another accumulator of the same setup (a continued run, another seed).
        The counts are added as they are, so both sides must be in the same state: both rank-local (before `reduce`) or both
        summed over the ranks.  With more than one rank a mixed pair is refused, since a later `reduce` would count one side
        once per rank.  A loaded file counts as rank-local (see `load`)."""
        if not self._same_setup(other):
            raise ValueError('RealSpaceAccumulator.merge: the two accumulators differ in cell, grid or bins')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('RealSpaceAccumulator.merge: one side is summed over the ranks and the other is rank-local')
        for k in ('dens', 'pair'):
            mine, theirs = getattr(self, k), getattr(other, k)
            if theirs is not None:
                setattr(self, k, theirs.clone() if mine is None else mine + theirs.to(mine.device))
        self.n_walkers += other.n_walkers
        return self

    def reduce(self):
        """Sum the counts and the walker number over the ranks in ONE all-reduce (`constants.psum_if_pmap`; the identity at
        world size 1).  Once per accumulator: a second call raises."""
        if self.reduced:
            raise RuntimeError('RealSpaceAccumulator.reduce was already called: reducing twice would count every rank again')
        if constants.world_size() == 1:
            self.reduced = True
            return self
        if (self.grid is not None and self.dens is None) or (self.n_r is not None and self.pair is None):
            self._buffers('cuda' if torch.cuda.is_available() else 'cpu')
        parts = [t.reshape(-1) for t in (self.dens, self.pair) if t is not None]
        packed = torch.cat(parts + [torch.tensor([self.n_walkers], dtype=torch.int64, device=parts[0].device)])
        packed = constants.psum_if_pmap(packed)
        off = 0
        for k in ('dens', 'pair'):
            t = getattr(self, k)
            if t is not None:
                setattr(self, k, packed[off:off + t.numel()].reshape(t.shape).clone())
                off += t.numel()
        self.n_walkers = int(packed[-1])
        self.reduced = True                 # only now: a collective that raised leaves the accumulator as it was
        return self

    # ---- normalisation (host)
    def _counts(self, t, shape):
        return np.zeros(shape, np.int64) if t is None else t.detach().cpu().numpy()

    def density_counts(self):
        if self.grid is None:
            raise ValueError('this accumulator holds no density (density_grid=None)')
        return self._counts(self.dens, (2,) + self.grid)

    def pair_counts(self):
        if self.n_r is None:
            raise ValueError('this accumulator holds no pair counts (pair_bins=None)')
        return self._counts(self.pair, (3, self.n_r))

    def r_edges(self):
        return np.arange(self.n_r + 1, dtype=np.float64) * (self.r_max / self.n_r)

    def density(self):
        """(2, g0, g1, g2) float64, electrons / Bohr^3: counts / (n_walkers dV V_sim / V_fold), dV = V_fold / (g0 g1 g2); each
        spin integrates over the folding cell to the electrons of that spin per folding cell."""
        counts = self.density_counts()
        v_sim, v_fold = abs(np.linalg.det(self.a)), abs(np.linalg.det(self.fold))
        dv = v_fold / float(np.prod(self.grid))
        return counts / (self.n_walkers * dv * v_sim / v_fold) if self.n_walkers else np.full(counts.shape, np.nan)

    def pair_correlation(self):
        """-> (r_mid (n_r,), g (3, n_r)): g_c[k] = counts_c[k] V_sim / (n_walkers P_c V_shell_k) with
        V_shell_k = 4 pi / 3 (r_{k+1}^3 - r_k^3), P_c = N_s (N_s - 1) / 2 for up-up and down-down and N_up N_down for up-down;
        a channel without pairs is NaN.  Independent uniform walkers give g = 1 in expectation for any N."""
        counts = self.pair_counts()
        edges = self.r_edges()
        shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
        nu, nd = self.nelec
        g = np.full((3, self.n_r), np.nan)
        for c, p in enumerate((nu * (nu - 1) // 2, nu * nd, nd * (nd - 1) // 2)):
            if p > 0 and self.n_walkers:
                g[c] = counts[c] * abs(np.linalg.det(self.a)) / (self.n_walkers * p * shell)
        return 0.5 * (edges[1:] + edges[:-1]), g

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the counts, the walker number and the setup they belong to ('reduced' records whether the counts
        were summed over the ranks when they were written; loading does not restore it, see `load`)."""
        sd = {'n_walkers': np.int64(self.n_walkers), 'simulation_lattice': self.a.copy(), 'nelec': np.asarray(self.nelec, np.int64),
              'reduced': np.bool_(self.reduced)}
        if self.grid is not None:
            sd.update(density_counts=self.density_counts(), fold_lattice=self.fold.copy(), grid=np.asarray(self.grid, np.int64))
        if self.n_r is not None:
            sd.update(pair_counts=self.pair_counts(), r_edges=self.r_edges(), pair_rmax=np.float64(self.r_max))
        return sd

    def load_state_dict(self, sd):
        """Replace the counts by those of `sd` (of an accumulator of the same setup); the accumulator is rank-local and open
        for `update` afterwards, as after `load`."""
        other = RealSpaceAccumulator.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('RealSpaceAccumulator.load_state_dict: the state belongs to another cell, grid or bins')
        self.dens, self.pair, self.n_walkers, self.reduced = other.dens, other.pair, other.n_walkers, other.reduced
        return self

    @classmethod
    def from_state_dict(cls, sd):
        has_d, has_p = 'density_counts' in sd, 'pair_counts' in sd
        acc = cls(_Lattices(sd['simulation_lattice'], sd['nelec']),
                  density_grid=tuple(int(v) for v in sd['grid']) if has_d else None,
                  density_cell=np.asarray(sd['fold_lattice']) if has_d else 'primitive',
                  pair_bins=len(sd['r_edges']) - 1 if has_p else None, pair_rmax=float(sd['pair_rmax']) if has_p else None)
        if has_d:
            acc.dens = torch.as_tensor(np.array(sd['density_counts'], dtype=np.int64).reshape((2,) + acc.grid))
        if has_p:
            acc.pair = torch.as_tensor(np.array(sd['pair_counts'], dtype=np.int64).reshape(3, acc.n_r))
        acc.n_walkers = int(sd['n_walkers'])
        return acc                          # reduced stays False: the loaded counts are this rank's contribution from here on

    def save(self, path, results=False):
        """One .npz of `state_dict()`; `results`: also the normalised density and g(r) (what `run_inference` writes)."""
        sd = self.state_dict()
        if results:
            if self.grid is not None:
                sd['density'] = self.density()
            if self.n_r is not None:
                sd['r_mid'], sd['g'] = self.pair_correlation()
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path`, as a fresh rank-local one: `update` or `merge` go on adding to its counts and
        `reduce` may be called once more, whether or not the file was written after a `reduce` (`run_inference` always writes
        after one).  The loaded counts then are this rank's contribution, so in a run of several ranks load the file on ONE
        rank only and start the others empty, or the old counts are summed once per rank."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})


# ------------------------------------------------------------------ momentum distribution (csrc/ds_onebody.h)
# The reference has no off-diagonal estimator; the conventions of this section are this project's own.
def momentum_kpoints(simulation_cell, klist, shells=1):
    """The Bloch-allowed wave vectors k = k_t + n . G_S of a network with the k list `klist` in the simulation cell, for
    |n_j| <= shells: k_t is the first entry of `klist` (all entries differ by supercell reciprocal vectors, so any entry spans
    the same set), G_S are the rows of 2 pi inv(a)^T.  -> (k (n_k, 3) float64, n (n_k, 3) int64), n = 0 first, the others in
    lexicographic order.  At most 512 points (shells <= 3): the limit of one `ds_one_body_ratios` call."""
    shells = int(shells)
    if not 0 <= shells <= 3:
        raise ValueError(f'shells = {shells}: 0 <= shells <= 3 is supported ((2 shells + 1)^3 <= 512 points per call)')
    kl = [np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in klist]
    kt = np.concatenate(kl, axis=0)[0]
    g = 2.0 * np.pi * np.linalg.inv(np.asarray(simulation_cell.a, dtype=np.float64).reshape(3, 3)).T
    r = np.arange(-shells, shells + 1)
    n = np.stack([m.ravel() for m in np.meshgrid(r, r, r, indexing='ij')], axis=1).astype(np.int64)
    zero = np.all(n == 0, axis=1)
    n = np.concatenate([n[zero], n[~zero]], axis=0)
    return kt[None, :] + n @ g, n


class MomentumDistribution:
    """Spin-resolved momentum distribution n_s(k) of a network's wavefunction, accumulated on the device over any number of walker
    batches: an accumulator for `run_inference(accumulators=...)`.  Every `update` is ONE `ds_one_body_ratios` call that moves,
    per walker, `samples_per_walker` electrons in turn (default N: one shift per electron) by shifts uniform in the simulation
    cell and adds q exp(-i k.s) to float64 sums; nothing is read back.  `net`: the object `make_solid_fermi_net` returns (or its
    `.apply`); `kpoints`: (k (n_k, 3), n (n_k, 3)) as `momentum_kpoints` returns them, None: that function with `shells`.
    The in-kernel noise is the Philox stream (seed, offset): the offset advances by 1 per update, the seed is decorrelated over
    the ranks the way `inference._rank_generator` does it."""

    def __init__(self, net, params, kpoints=None, shells=1, samples_per_walker=None, seed=0):
        self.apply = getattr(net, 'apply', net)
        self.params = params
        cell = self.apply.simulation_cell
        self.nelec = (int(cell.nelec[0]), int(cell.nelec[1]))
        k, n = momentum_kpoints(cell, self.apply.klist, shells) if kpoints is None else kpoints
        self._setup(k, n, samples_per_walker)
        self.seed = (int(seed) * max(1, constants.world_size()) + constants.rank()) % (1 << 63)

    def _setup(self, k, n, samples_per_walker):
        self.kpoints = np.ascontiguousarray(np.asarray(k, dtype=np.float64).reshape(-1, 3))
        self.k_int = np.ascontiguousarray(np.asarray(n, dtype=np.int64).reshape(-1, 3))
        if not 1 <= len(self.kpoints) <= 512 or len(self.k_int) != len(self.kpoints):
            raise ValueError(f'MomentumDistribution: between 1 and 512 k points (with one integer triple each) are supported, '
                             f'got {len(self.kpoints)} / {len(self.k_int)}')
        n_el = sum(self.nelec)
        self.samples_per_walker = n_el if samples_per_walker is None else int(samples_per_walker)
        if self.samples_per_walker < 1:
            raise ValueError(f'samples_per_walker = {samples_per_walker} must be >= 1')
        self.sums = torch.zeros(2, len(self.kpoints), 2, dtype=torch.float64)      # moved to the walkers' device by the first update
        self.n_bad = torch.zeros(2, dtype=torch.int64)
        self.samples = np.zeros(2, dtype=np.int64)
        self.offset = 0
        self.first_electron = 0
        self.seed = 0
        self.reduced = False
        self._kdev = None

    # ---- accumulation
    def update(self, data):
        """Add `samples_per_walker` ratios of every walker of `data` (B, 3N) to the sums: one library call, no device -> host
        copy.  The samples per spin are counted on the host: they follow from first_electron alone."""
        if self.apply is None:
            raise RuntimeError('MomentumDistribution.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('MomentumDistribution.update after reduce(): the sums are already summed over the ranks')
        n_el, m = sum(self.nelec), self.samples_per_walker
        if data.shape[-1] != 3 * n_el:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {n_el} electrons')
        x = data.reshape(-1, 3 * n_el)
        sysd = self.apply.system
        if self.sums.device != x.device:
            self.sums, self.n_bad = self.sums.to(x.device), self.n_bad.to(x.device)
        if self._kdev is None or self._kdev.device != x.device:
            self._kdev = torch.as_tensor(self.kpoints).to(x.device)
        out = sysd.one_body_ratios(self.params, x, m, kvec=self._kdev, first_electron=self.first_electron, seed=self.seed,
                                   offset=self.offset, nk_sums=self.sums)
        self.n_bad += out['n_bad']
        up = int(np.count_nonzero((self.first_electron + np.arange(m)) % n_el < self.nelec[0]))
        self.samples += np.asarray([up, m - up], dtype=np.int64) * int(x.shape[0])
        self.offset += 1
        self.first_electron = (self.first_electron + m) % n_el

    def _same_setup(self, other):
        return self.nelec == other.nelec and np.array_equal(self.kpoints, other.kpoints) and np.array_equal(self.k_int, other.k_int)

    def merge(self, other):
        """Add the sums, sample counts and bad counts of another accumulator with the same electrons and k list.  Both sides must
        be in the same state (rank-local or summed over the ranks), as for `RealSpaceAccumulator.merge`."""
        if not self._same_setup(other):
            raise ValueError('MomentumDistribution.merge: the two accumulators differ in electron numbers or k points')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('MomentumDistribution.merge: one side is summed over the ranks and the other is rank-local')
        self.sums = self.sums + other.sums.to(self.sums.device)
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        self.samples = self.samples + other.samples
        return self

    def reduce(self):
        """Sum the sums, the bad counts and the sample counts over the ranks in ONE packed float64 all-reduce (counts below 2^53
        are exact; the identity at world size 1).  Once per accumulator: a second call raises."""
        if self.reduced:
            raise RuntimeError('MomentumDistribution.reduce was already called: reducing twice would count every rank again')
        if constants.world_size() > 1:
            dev = self.sums.device if self.sums.is_cuda else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
            n = self.sums.numel()
            packed = torch.cat([self.sums.reshape(-1).to(dev), self.n_bad.to(dev, torch.float64),
                                torch.as_tensor(self.samples, dtype=torch.float64, device=dev)])
            packed = constants.psum_if_pmap(packed)
            self.sums = packed[:n].reshape(self.sums.shape).clone()
            self.n_bad = packed[n:n + 2].round().to(torch.int64)
            self.samples = packed[n + 2:n + 4].round().cpu().numpy().astype(np.int64)
        self.reduced = True
        return self

    # ---- normalisation (host)
    def momentum_distribution(self):
        """(2, n_k) complex128: n_s(k) = N_s sums_s(k) / (samples on spin s - bad samples on spin s); the real part is the
        estimate, the imaginary part vanishes in expectation.  A spin without electrons is 0, one without good samples NaN."""
        s = self.sums.detach().cpu().numpy()
        good = self.samples - self.n_bad.detach().cpu().numpy()
        out = np.zeros((2, len(self.kpoints)), dtype=np.complex128)
        for sp in range(2):
            if self.nelec[sp] > 0:
                out[sp] = self.nelec[sp] * (s[sp, :, 0] + 1j * s[sp, :, 1]) / good[sp] if good[sp] > 0 else np.nan
        return out

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the sums and counts, the k list they belong to and where the noise stream stands."""
        return {'sums': self.sums.detach().cpu().numpy().copy(), 'samples': self.samples.copy(),
                'n_bad': self.n_bad.detach().cpu().numpy().copy(), 'kpoints': self.kpoints.copy(), 'k_int': self.k_int.copy(),
                'nelec': np.asarray(self.nelec, np.int64), 'samples_per_walker': np.int64(self.samples_per_walker),
                'offset': np.int64(self.offset), 'first_electron': np.int64(self.first_electron), 'reduced': np.bool_(self.reduced)}

    def load_state_dict(self, sd):
        """Replace the sums, counts and stream position by those of `sd` (same electrons and k list); the accumulator is
        rank-local and open for `update` afterwards."""
        other = MomentumDistribution.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('MomentumDistribution.load_state_dict: the state belongs to other electron numbers or k points')
        self.sums, self.n_bad, self.samples = other.sums.to(self.sums.device), other.n_bad.to(self.n_bad.device), other.samples
        self.offset, self.first_electron, self.reduced = other.offset, other.first_electron, False
        return self

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = None
        acc.nelec = tuple(int(v) for v in sd['nelec'])
        acc._setup(sd['kpoints'], sd['k_int'], int(sd['samples_per_walker']) if 'samples_per_walker' in sd else None)
        acc.sums = torch.as_tensor(np.array(sd['sums'], dtype=np.float64).reshape(2, -1, 2))
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(2))
        acc.samples = np.array(sd['samples'], dtype=np.int64).reshape(2)
        acc.offset = int(sd['offset']) if 'offset' in sd else 0
        acc.first_electron = int(sd['first_electron']) if 'first_electron' in sd else 0
        return acc                          # reduced stays False: the loaded sums are this rank's contribution from here on

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also `n_k`, the normalised complex (2, n_k) distribution."""
        sd = self.state_dict()
        if results:
            sd['n_k'] = self.momentum_distribution()
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path` as a fresh rank-local one without a network (see `from_state_dict`)."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})


# ------------------------------------------------------------------ total spin <S^2> (csrc/ds_spin.h)
# The reference has no such estimator; the conventions of this section are this project's own.
class SpinSquared:
    """Total spin <S^2> of a network's wavefunction from spin-exchange ratios, accumulated on the device over any number of walker
    batches: an accumulator for `run_inference(accumulators=...)`.  With P = n_up n_dn pairs (i, j) of an up and a down electron and
    q_p(R) = psi(P_p R) / psi(R), P_p exchanging the two positions,

        <S^2> = S_z (S_z + 1) + n_dn - < sum_p q_p(R) >_{|psi|^2},   S_z = (n_up - n_dn) / 2.

    Every `update` is ONE `ds_spin_exchange_ratios` call that takes, per walker, `pairs_per_walker` = M pairs in turn (default P:
    every pair) and adds the walker sums t_w = sum_m q_{w,m} to four float64 numbers; nothing is read back.  psi is antisymmetric
    within a spin channel, so every pair has the same expectation and M pairs scaled by P / M are unbiased; `first_pair` advances by
    M mod P per update, so that all pairs are visited in turn.  No random numbers are drawn.  `net`: the object
    `make_solid_fermi_net` returns (or its `.apply`).  A cell without a pair of opposite spins (P = 0) makes no library call."""

    def __init__(self, net, params, pairs_per_walker=None):
        self.apply = getattr(net, 'apply', net)
        self.params = params
        cell = self.apply.simulation_cell
        self._setup((int(cell.nelec[0]), int(cell.nelec[1])), pairs_per_walker)

    def _setup(self, nelec, pairs_per_walker):
        self.nelec = (int(nelec[0]), int(nelec[1]))
        self.n_pairs_total = self.nelec[0] * self.nelec[1]
        self.pairs_per_walker = self.n_pairs_total if pairs_per_walker is None else int(pairs_per_walker)
        if self.pairs_per_walker < 1 and self.n_pairs_total > 0:
            raise ValueError(f'pairs_per_walker = {pairs_per_walker} must be >= 1')
        self.sums = torch.zeros(4, dtype=torch.float64)          # moved to the walkers' device by the first update
        self.n_bad = torch.zeros(1, dtype=torch.int64)
        self.n_walkers = 0
        self.first_pair = 0
        self.reduced = False

    # ---- accumulation
    def update(self, data):
        """Add `pairs_per_walker` exchange ratios of every walker of `data` (B, 3N) to the sums: one library call, no device -> host
        copy.  With P = 0 the walkers are only counted."""
        if self.apply is None:
            raise RuntimeError('SpinSquared.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('SpinSquared.update after reduce(): the sums are already summed over the ranks')
        n_el = sum(self.nelec)
        if data.shape[-1] != 3 * n_el:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {n_el} electrons')
        x = data.reshape(-1, 3 * n_el)
        self.n_walkers += int(x.shape[0])
        if self.n_pairs_total == 0:
            return
        if self.sums.device != x.device:
            self.sums, self.n_bad = self.sums.to(x.device), self.n_bad.to(x.device)
        out = self.apply.system.spin_exchange_ratios(self.params, x, self.pairs_per_walker, first_pair=self.first_pair, sums=self.sums)
        self.n_bad += out['n_bad']
        self.first_pair = (self.first_pair + self.pairs_per_walker) % self.n_pairs_total

    def _same_setup(self, other):
        return self.nelec == other.nelec and self.pairs_per_walker == other.pairs_per_walker

    def merge(self, other):
        """Add the sums, the bad count and the walker number of another accumulator with the same electrons and pairs per walker.
        Both sides must be in the same state (rank-local or summed over the ranks), as for `RealSpaceAccumulator.merge`."""
        if not self._same_setup(other):
            raise ValueError('SpinSquared.merge: the two accumulators differ in electron numbers or pairs per walker')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('SpinSquared.merge: one side is summed over the ranks and the other is rank-local')
        self.sums = self.sums + other.sums.to(self.sums.device)
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        self.n_walkers += other.n_walkers
        return self

    def reduce(self):
        """Sum the four sums, the bad count and the walker number over the ranks in ONE packed float64 all-reduce (counts below
        2^53 are exact; the identity at world size 1).  Once per accumulator: a second call raises."""
        if self.reduced:
            raise RuntimeError('SpinSquared.reduce was already called: reducing twice would count every rank again')
        if constants.world_size() > 1:
            dev = self.sums.device if self.sums.is_cuda else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
            packed = torch.cat([self.sums.to(dev), self.n_bad.to(dev, torch.float64),
                                torch.tensor([self.n_walkers], dtype=torch.float64, device=dev)])
            packed = constants.psum_if_pmap(packed)
            self.sums = packed[:4].clone()
            self.n_bad = packed[4:5].round().to(torch.int64)
            self.n_walkers = int(packed[5].round())
        self.reduced = True                 # only now: a collective that raised leaves the accumulator as it was
        return self

    # ---- normalisation (host)
    def spin_squared(self):
        """-> dict(value, error, imag, n_walkers, n_bad, sz):
        value = S_z (S_z + 1) + n_dn - (P / M) sum_w Re t_w / n_good over the n_good walkers whose ratios were all finite;
        error = (P / M) sqrt((sum_w (Re t_w)^2 / n_good - mean^2) / (n_good - 1)): a NAIVE standard error over walkers -- it takes
        them as independent and ignores the autocorrelation of the Markov chain, so it is a lower bound on a real run (NaN below
        two good walkers); imag = -(P / M) sum_w Im t_w / n_good (vanishes in expectation); n_walkers: all walkers seen; n_bad:
        those left out.  With P = 0 there is nothing to sample: value = S_z (S_z + 1) + n_dn = s (s + 1), s = |S_z|, exactly
        (which is S_z (S_z + 1) for the cell without down electrons), error = 0."""
        nu, nd = self.nelec
        sz = 0.5 * (nu - nd)
        base = sz * (sz + 1.0) + nd
        n_bad = int(self.n_bad.sum())
        if self.n_pairs_total == 0:
            return dict(value=base, error=0.0, imag=0.0, n_walkers=self.n_walkers, n_bad=n_bad, sz=sz)
        s = self.sums.detach().cpu().numpy()
        scale = self.n_pairs_total / self.pairs_per_walker
        n = float(s[3])
        if n < 1:
            return dict(value=float('nan'), error=float('nan'), imag=float('nan'), n_walkers=self.n_walkers, n_bad=n_bad, sz=sz)
        mean = s[0] / n
        var = max(s[2] / n - mean * mean, 0.0)
        error = scale * float(np.sqrt(var / (n - 1))) if n > 1 else float('nan')
        return dict(value=float(base - scale * mean), error=error, imag=float(-scale * s[1] / n), n_walkers=self.n_walkers,
                    n_bad=n_bad, sz=sz)

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the sums and counts, the setup they belong to and the pair the next update starts from."""
        return {'sums': self.sums.detach().cpu().numpy().copy(), 'n_bad': self.n_bad.detach().cpu().numpy().copy(),
                'n_walkers': np.int64(self.n_walkers), 'nelec': np.asarray(self.nelec, np.int64),
                'pairs_per_walker': np.int64(self.pairs_per_walker), 'first_pair': np.int64(self.first_pair),
                'reduced': np.bool_(self.reduced)}

    def load_state_dict(self, sd):
        """Replace the sums, counts and the next pair by those of `sd` (same electrons and pairs per walker); the accumulator is
        rank-local and open for `update` afterwards."""
        other = SpinSquared.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('SpinSquared.load_state_dict: the state belongs to other electron numbers or pairs per walker')
        self.sums, self.n_bad = other.sums.to(self.sums.device), other.n_bad.to(self.n_bad.device)
        self.n_walkers, self.first_pair, self.reduced = other.n_walkers, other.first_pair, False
        return self

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = None
        acc._setup(tuple(int(v) for v in sd['nelec']), int(sd['pairs_per_walker']))
        acc.sums = torch.as_tensor(np.array(sd['sums'], dtype=np.float64).reshape(4))
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(1))
        acc.n_walkers = int(sd['n_walkers'])
        acc.first_pair = int(sd['first_pair']) if 'first_pair' in sd else 0
        return acc                          # reduced stays False: the loaded sums are this rank's contribution from here on

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also `value`, `error` and `imag` of `spin_squared()`."""
        sd = self.state_dict()
        if results:
            r = self.spin_squared()
            sd.update(value=np.float64(r['value']), error=np.float64(r['error']), imag=np.float64(r['imag']))
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path` as a fresh rank-local one without a network (see `from_state_dict`)."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})


# ------------------------------------------------------------------ ionic forces (csrc/ds_force.h)
# The reference has no force estimator; the conventions of this section are this project's own.
def force_cutoff(a, cutoff=None):
    """The cutoff r_c of the zero-variance force term for the lattice `a`: `cutoff` in bohr, by default `wigner_seitz_radius(a)`, which
    is also the largest value accepted; anything <= 0, not finite or larger raises ValueError.  So does a cutoff that is not below
    the smallest plane spacing (lattice vectors far from reduced: the kernel looks for the nearest image one cell around the
    wrapped one; no shipped cell comes close)."""
    r_ws = wigner_seitz_radius(a)
    cutoff = r_ws if cutoff is None else float(cutoff)
    if not (np.isfinite(cutoff) and 0.0 < cutoff <= r_ws * (1.0 + 1e-12)):
        raise ValueError(f'cutoff = {cutoff} must be positive and at most the Wigner-Seitz radius {r_ws} of the simulation cell')
    if not cutoff < plane_spacings(a).min():
        raise ValueError(f'cutoff = {cutoff} is not below the smallest plane spacing {plane_spacings(a).min()} of the simulation '
                         'cell: the lattice vectors are too skewed for the nearest-image search (use a reduced cell)')
    return cutoff


class IonForces:
    """Forces on the ions of the simulation cell, accumulated on the device over any number of walker batches: an accumulator for
    `run_inference(accumulators=...)` (VMC) and `run_dmc(accumulators=...)` (the mixed estimate, on comb blocks).  Per ion a:

        hf = < -d(E_ei + E_ii)/dR_a >                 the Hellmann-Feynman force of the Ewald energy (infinite variance at an
                                                      all-electron nucleus: the integrand goes as 1/r^2)
        zv = < hf + (H - E_L)(Q_a psi)/psi >          the zero-variance force of Assaraf and Caffarel,
             Q_a = -Z_a sum_i c(r_ia) v_ia / r_ia,    c(r) = (1 - r^2/r_c^2)^3 inside the cutoff r_c, 0 beyond,
                                                      v_ia the nearest image of r_i - R_a

    The added term has zero expectation and cancels the 1/r^2 singularity; it needs only the drift Re grad log psi.
    WHAT IS MISSING: the Pulay term 2 <(E_L - E) d log psi / dR_a> is not evaluated (the walker gradient comes from forward jets:
    there is no derivative with respect to an ion position).  hf and zv are therefore the force only for an exact psi, and their
    bias is FIRST ORDER in the error of the wave function.  All-electron ions only: a semi-local pseudopotential has force terms
    of its own, which are not implemented (`pseudopotential` must be None).  `PrimitiveForces` (below) adds the Pulay term for the
    atoms of the primitive cell.

    Every `update` is ONE `ds_logpsi_grad` call and ONE `ds_ion_forces` call that adds to 12 A + 1 float64 numbers; nothing is read
    back.  `cutoff`: r_c, by default (and at most) `wigner_seitz_radius` of the simulation cell.  `net`: the object
    `make_solid_fermi_net` returns (or its `.apply`).
    A pure (forward-walking) DMC estimate of one component goes through `dmc.ForwardWalking` as a callable, for instance
    `scalars={'f_zv': lambda arrays: system.ion_forces(arrays['x'], arrays['drift'])['zv'].reshape(len(arrays['x']), -1)}`."""

    def __init__(self, net, params, cutoff=None, pseudopotential=None):
        if pseudopotential is not None:
            raise NotImplementedError('IonForces: the force terms of a semi-local pseudopotential are not implemented '
                                      '(all-electron ions only)')
        self.apply = getattr(net, 'apply', net)
        self.params = params
        cell = self.apply.simulation_cell
        self._setup(np.asarray(cell.atom_coords(), np.float64), np.asarray(cell.atom_charges(), np.float64),
                    np.asarray(cell.a, np.float64), int(sum(cell.nelec)), cutoff)

    def _setup(self, atoms, charges, latvec, n_elec, cutoff):
        self.atoms = np.asarray(atoms, np.float64).reshape(-1, 3)
        self.charges = np.asarray(charges, np.float64).reshape(-1)
        self.latvec = np.asarray(latvec, np.float64).reshape(3, 3)
        self.n_elec = int(n_elec)
        self.cutoff = force_cutoff(self.latvec, cutoff)
        self.n_atoms = self.atoms.shape[0]
        self.sums = torch.zeros(12 * self.n_atoms + 1, dtype=torch.float64)     # moved to the walkers' device by the first update
        self.n_bad = torch.zeros(1, dtype=torch.int64)
        self.n_walkers = 0
        self.reduced = False

    # ---- accumulation
    def update(self, data):
        """Add the forces of every walker of `data` (B, 3N) to the sums: one `ds_logpsi_grad` and one `ds_ion_forces` call, no
        device -> host copy."""
        if self.apply is None:
            raise RuntimeError('IonForces.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('IonForces.update after reduce(): the sums are already summed over the ranks')
        if data.shape[-1] != 3 * self.n_elec:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {self.n_elec} electrons')
        x = data.reshape(-1, 3 * self.n_elec)
        if x.shape[0] == 0:
            return
        if self.sums.device != x.device:
            self.sums, self.n_bad = self.sums.to(x.device), self.n_bad.to(x.device)
        system = self.apply.system
        drift = system.logpsi_grad(self.params, x)[1].real.contiguous()
        out = system.ion_forces(x, drift, cutoff=self.cutoff, sums=self.sums, want_walker=False)
        self.n_bad += out['n_bad']
        self.n_walkers += int(x.shape[0])           # only now: a call that raised leaves the count with the sums

    def _same_setup(self, other):
        return (self.atoms.shape == other.atoms.shape and np.array_equal(self.atoms, other.atoms) and
                np.array_equal(self.charges, other.charges) and np.array_equal(self.latvec, other.latvec) and
                self.n_elec == other.n_elec and self.cutoff == other.cutoff)

    def merge(self, other):
        """Add the sums, the bad count and the walker number of another accumulator of the same ions, lattice and cutoff.  Both sides
        must be in the same state (rank-local or summed over the ranks), as for `SpinSquared.merge`."""
        if not self._same_setup(other):
            raise ValueError('IonForces.merge: the two accumulators differ in ions, lattice, electron number or cutoff')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('IonForces.merge: one side is summed over the ranks and the other is rank-local')
        self.sums = self.sums + other.sums.to(self.sums.device)
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        self.n_walkers += other.n_walkers
        return self

    def reduce(self):
        """Sum the sums, the bad count and the walker number over the ranks in ONE packed float64 all-reduce (counts below 2^53 are
        exact; the identity at world size 1).  Once per accumulator: a second call raises."""
        if self.reduced:
            raise RuntimeError('IonForces.reduce was already called: reducing twice would count every rank again')
        if constants.world_size() > 1:
            dev = self.sums.device if self.sums.is_cuda else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
            k = self.sums.numel()
            packed = torch.cat([self.sums.to(dev), self.n_bad.to(dev, torch.float64),
                                torch.tensor([self.n_walkers], dtype=torch.float64, device=dev)])
            packed = constants.psum_if_pmap(packed)
            self.sums = packed[:k].clone()
            self.n_bad = packed[k:k + 1].round().to(torch.int64)
            self.n_walkers = int(packed[k + 1].round())
        self.reduced = True                 # only now: a collective that raised leaves the accumulator as it was
        return self

    # ---- normalisation (host)
    def forces(self):
        """-> dict(hf, hf_error, zv, zv_error (each (A, 3) float64, Ha/bohr), n_walkers, n_bad, atoms (A, 3), cutoff):
        the means over the n_good walkers whose forces were finite, and error = sqrt((sum f^2 / n_good - mean^2) / (n_good - 1)): a
        NAIVE standard error over walkers -- it takes them as independent and ignores the autocorrelation of the Markov chain, so
        it is a lower bound on a real run (NaN below two good walkers; of hf it does not even exist in the limit: the variance of
        the bare Hellmann-Feynman force of an all-electron ion is infinite).  NaN everywhere without a good walker.  The Pulay
        term is not part of either force (see the class)."""
        s = self.sums.detach().cpu().numpy()
        A = self.n_atoms
        n = float(s[12 * A])
        q = s[:12 * A].reshape(A, 3, 4)
        out = dict(n_walkers=self.n_walkers, n_bad=int(self.n_bad.sum()), atoms=self.atoms.copy(), cutoff=self.cutoff)
        for name, k in (('hf', 0), ('zv', 2)):
            if n < 1:
                out[name] = np.full((A, 3), np.nan)
                out[name + '_error'] = np.full((A, 3), np.nan)
                continue
            mean = q[:, :, k] / n
            var = np.maximum(q[:, :, k + 1] / n - mean * mean, 0.0)
            out[name] = mean
            out[name + '_error'] = np.sqrt(var / (n - 1)) if n > 1 else np.full((A, 3), np.nan)
        return out

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the sums and counts and the setup they belong to."""
        return {'sums': self.sums.detach().cpu().numpy().copy(), 'n_bad': self.n_bad.detach().cpu().numpy().copy(),
                'n_walkers': np.int64(self.n_walkers), 'atoms': self.atoms.copy(), 'charges': self.charges.copy(),
                'latvec': self.latvec.copy(), 'n_elec': np.int64(self.n_elec), 'cutoff': np.float64(self.cutoff),
                'reduced': np.bool_(self.reduced)}

    def load_state_dict(self, sd):
        """Replace the sums and counts by those of `sd` (same ions, lattice and cutoff); the accumulator is rank-local and open for
        `update` afterwards."""
        other = IonForces.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('IonForces.load_state_dict: the state belongs to other ions, another lattice or another cutoff')
        self.sums, self.n_bad = other.sums.to(self.sums.device), other.n_bad.to(self.n_bad.device)
        self.n_walkers, self.reduced = other.n_walkers, False
        return self

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = None
        acc._setup(sd['atoms'], sd['charges'], sd['latvec'], int(sd['n_elec']), float(sd['cutoff']))
        acc.sums = torch.as_tensor(np.array(sd['sums'], dtype=np.float64).reshape(12 * acc.n_atoms + 1))
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(1))
        acc.n_walkers = int(sd['n_walkers'])
        return acc                          # reduced stays False: the loaded sums are this rank's contribution from here on

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also hf, hf_error, zv and zv_error of `forces()`."""
        sd = self.state_dict()
        if results:
            r = self.forces()
            sd.update({k: r[k] for k in ('hf', 'hf_error', 'zv', 'zv_error')})
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path` as a fresh rank-local one without a network (see `from_state_dict`)."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})


# ------------------------------------------------------------------ pseudopotential forces (csrc/ds_ecp_force.h)
# The reference has neither pseudopotentials nor forces; the conventions are this project's own.
_ECP_KEYS = ('atom_species', 'n_l', 'r_cut_loc', 'r_cut_nl', 'n_quad', 'term_offset', 'term_n', 'term_zeta', 'term_c')


def _ecp_signature(ecp):
    """The arrays that define a `pseudopotential.SemiLocalECP` beyond cell and atoms, as plain numpy (what `merge` compares)."""
    sig = dict(atom_species=np.asarray(ecp.atom_species, np.int32), n_l=np.asarray(ecp.n_l, np.int32),
               r_cut_loc=np.asarray(ecp.r_cut_loc, np.float64), r_cut_nl=np.asarray(ecp.r_cut_nl, np.float64),
               n_quad=np.asarray(ecp.n_quad, np.int32))
    sig.update(ecp.tables())
    return sig


class PseudopotentialForces(IonForces):
    """Forces on the ions of a simulation cell with a semi-local pseudopotential, accumulated on the device over any number of walker
    batches: an accumulator with the interface of `IonForces`, for `run_inference(accumulators=...)` (VMC) and
    `run_dmc(accumulators=...)`.  Per ion a:

        pp    = < F^loc_a + Re F^nl_a >        minus the derivative of E_loc + E_nl of `ds_ecp_energy` in R_a, with psi held fixed
                                               as a function of the electron coordinates (`ds_ecp_forces`)
        total = < pp + hf >                    hf = -d(E_ei + E_ii)/dR_a of the Ewald energy with Z_eff (`ds_ion_forces`' out_hf)

    No zero-variance term is added: inside the core the 1/r^2 of the Z_eff Ewald force is cancelled by v'_loc of any published
    potential, so the variance of the total is finite without one.
    LIMITS, read them before using a number:
      - Hellmann-Feynman part only.  The Pulay term 2 <(E_L - E) d log psi / dR_a> with E_pp inside E_L is not evaluated, so the
        bias is FIRST ORDER in the error of psi, as `IonForces` is without `PrimitiveForces`.
      - The radial functions are exactly 0 outside their cutoffs.  The jump at a cutoff is a delta term of the exact derivative and
        is left out; its size is that of the function at its cutoff, `find_cutoff`'s `tol`.
      - A walker with an electron exactly on a pseudo-ion (r = 0: no direction) is bad: it is left out and counted in n_bad, like a
        walker with a non-finite coordinate or result.
      - Under `run_dmc` the numbers are MIXED estimates (psi_T psi_0), taken on comb blocks; not the pure estimate.
      - Cost: one forward-Laplacian chain evaluation per quadrature configuration, N_q per (electron, ion) pair inside r_cut_nl.

    Every `update` is ONE `ds_ion_forces` call for out_hf (no drift needed) and ONE `ds_ecp_forces` call with that as `base`, which
    adds to 12 A + 1 float64 numbers in the library's fixed order; the rotation offset advances by one per update (`key` is the
    Philox seed).  The `ds_ecp_forces` call synchronises the stream once (the pair total)."""

    def __init__(self, net, params, pseudopotential, key=0):
        if pseudopotential is None:
            raise ValueError('PseudopotentialForces needs a pseudopotential (all-electron ions: IonForces)')
        self.apply = getattr(net, 'apply', net)
        self.params = params
        self.pseudopotential = pseudopotential
        cell = self.apply.simulation_cell
        atoms, latvec = np.asarray(cell.atom_coords(), np.float64).reshape(-1, 3), np.asarray(cell.a, np.float64).reshape(3, 3)
        if atoms.shape != pseudopotential.atoms.shape or not (np.allclose(atoms, pseudopotential.atoms, rtol=0, atol=1e-10) and
                                                              np.allclose(latvec, pseudopotential.a, rtol=0, atol=1e-10)):
            raise ValueError('PseudopotentialForces: the pseudopotential was built for another simulation cell')
        self._setup(atoms, np.asarray(cell.atom_charges(), np.float64), latvec, int(sum(cell.nelec)),
                    _ecp_signature(pseudopotential), key)

    def _setup(self, atoms, charges, latvec, n_elec, ecp, key):
        self.atoms = np.asarray(atoms, np.float64).reshape(-1, 3)
        self.charges = np.asarray(charges, np.float64).reshape(-1)
        self.latvec = np.asarray(latvec, np.float64).reshape(3, 3)
        self.n_elec = int(n_elec)
        self.ecp = {k: np.asarray(ecp[k]) for k in _ECP_KEYS}
        self.seed, self.offset = int(key), 0
        self.n_atoms = self.atoms.shape[0]
        self.sums = torch.zeros(12 * self.n_atoms + 1, dtype=torch.float64)     # moved to the walkers' device by the first update
        self.n_bad = torch.zeros(1, dtype=torch.int64)
        self.n_walkers = 0
        self.reduced = False

    def update(self, data):
        """Add the forces of every walker of `data` (B, 3N) to the sums: one `ds_ion_forces` and one `ds_ecp_forces` call."""
        if self.apply is None:
            raise RuntimeError('PseudopotentialForces.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('PseudopotentialForces.update after reduce(): the sums are already summed over the ranks')
        if data.shape[-1] != 3 * self.n_elec:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {self.n_elec} electrons')
        x = data.reshape(-1, 3 * self.n_elec)
        if x.shape[0] == 0:
            return
        if self.sums.device != x.device:
            self.sums, self.n_bad = self.sums.to(x.device), self.n_bad.to(x.device)
        system = self.apply.system
        hf = system.ion_forces(x)['hf']
        out = system.ecp_forces(self.params, x, self.pseudopotential, seed=self.seed, offset=self.offset, base=hf, sums=self.sums,
                                want_walker=False)
        self.offset += 1
        self.n_bad += out['n_bad']
        self.n_walkers += int(x.shape[0])           # only now: a call that raised leaves the count with the sums

    def _same_setup(self, other):
        return (isinstance(other, PseudopotentialForces) and self.atoms.shape == other.atoms.shape and
                np.array_equal(self.atoms, other.atoms) and np.array_equal(self.charges, other.charges) and
                np.array_equal(self.latvec, other.latvec) and self.n_elec == other.n_elec and
                all(np.array_equal(self.ecp[k], other.ecp[k]) for k in _ECP_KEYS))

    def merge(self, other):
        """Add the sums, the bad count and the walker number of another accumulator of the same ions, lattice and pseudopotential.
        Both sides must be in the same state (rank-local or summed over the ranks)."""
        if not self._same_setup(other):
            raise ValueError('PseudopotentialForces.merge: the two accumulators differ in ions, lattice, electron number or pseudopotential')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('PseudopotentialForces.merge: one side is summed over the ranks and the other is rank-local')
        self.sums = self.sums + other.sums.to(self.sums.device)
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        self.n_walkers += other.n_walkers
        return self

    def forces(self):
        """-> dict(pp, pp_error, total, total_error (each (A, 3) float64, Ha/bohr), n_walkers, n_bad, atoms (A, 3)): the means over the
        n_good walkers whose forces were finite, and error = sqrt((sum f^2 / n_good - mean^2) / (n_good - 1)): the NAIVE standard
        error of `IonForces.forces` (walkers taken as independent; NaN below two good walkers).  NaN everywhere without a good
        walker.  The limits of the class apply: Hellmann-Feynman only, no cutoff delta term, mixed estimate under DMC."""
        s = self.sums.detach().cpu().numpy()
        A = self.n_atoms
        n = float(s[12 * A])
        q = s[:12 * A].reshape(A, 3, 4)
        out = dict(n_walkers=self.n_walkers, n_bad=int(self.n_bad.sum()), atoms=self.atoms.copy())
        for name, k in (('pp', 0), ('total', 2)):
            if n < 1:
                out[name] = np.full((A, 3), np.nan)
                out[name + '_error'] = np.full((A, 3), np.nan)
                continue
            mean = q[:, :, k] / n
            var = np.maximum(q[:, :, k + 1] / n - mean * mean, 0.0)
            out[name] = mean
            out[name + '_error'] = np.sqrt(var / (n - 1)) if n > 1 else np.full((A, 3), np.nan)
        return out

    def state_dict(self):
        """Plain numpy arrays: the sums and counts and the setup they belong to (the pseudopotential's tables as `ecp_<name>`)."""
        sd = {'sums': self.sums.detach().cpu().numpy().copy(), 'n_bad': self.n_bad.detach().cpu().numpy().copy(),
              'n_walkers': np.int64(self.n_walkers), 'atoms': self.atoms.copy(), 'charges': self.charges.copy(),
              'latvec': self.latvec.copy(), 'n_elec': np.int64(self.n_elec), 'seed': np.int64(self.seed),
              'offset': np.int64(self.offset), 'reduced': np.bool_(self.reduced)}
        sd.update({'ecp_' + k: self.ecp[k].copy() for k in _ECP_KEYS})
        return sd

    def load_state_dict(self, sd):
        """Replace the sums and counts by those of `sd` (same ions, lattice and pseudopotential); the rotation offset continues
        behind the larger of the two, and the accumulator is rank-local and open for `update` afterwards."""
        other = PseudopotentialForces.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('PseudopotentialForces.load_state_dict: the state belongs to other ions, another lattice or another pseudopotential')
        self.sums, self.n_bad = other.sums.to(self.sums.device), other.n_bad.to(self.n_bad.device)
        self.n_walkers, self.reduced, self.offset = other.n_walkers, False, max(self.offset, other.offset)
        return self

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = acc.pseudopotential = None
        acc._setup(sd['atoms'], sd['charges'], sd['latvec'], int(sd['n_elec']), {k: sd['ecp_' + k] for k in _ECP_KEYS}, int(sd['seed']))
        acc.offset = int(sd['offset'])
        acc.sums = torch.as_tensor(np.array(sd['sums'], dtype=np.float64).reshape(12 * acc.n_atoms + 1))
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(1))
        acc.n_walkers = int(sd['n_walkers'])
        return acc                          # reduced stays False: the loaded sums are this rank's contribution from here on

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also pp, pp_error, total and total_error of `forces()`."""
        sd = self.state_dict()
        if results:
            r = self.forces()
            sd.update({k: r[k] for k in ('pp', 'pp_error', 'total', 'total_error')})
        with open(path, 'wb') as f:
            np.savez(f, **sd)


# ------------------------------------------------------------------ stress tensor and pressure (csrc/ds_stress.h)
# The reference has no stress estimator; the conventions of this section are this project's own.
STRESS_ROWS = ('kin', 'ee', 'ei', 'total')


def voigt_to_matrix(v):
    """(..., 6) in the component order xx, yy, zz, yz, xz, xy of `ds_stress` -> (..., 3, 3) symmetric."""
    from .ewaldsum import VOIGT
    v = np.asarray(v, np.float64)
    out = np.empty(v.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(VOIGT):
        out[..., a, b] = out[..., b, a] = v[..., k]
    return out


def strain_generators():
    """(6, 3, 3): the symmetric matrices E_k with eps = h E_k the strain whose derivative in h is the component k (xx, yy, zz, yz, xz, xy)
    of a strain derivative as `ds_stress` defines it (the two off-diagonal entries count as independent: each is h / 2)."""
    from .ewaldsum import VOIGT
    E = np.zeros((6, 3, 3))
    for k, (a, b) in enumerate(VOIGT):
        E[k, a, b] += 0.5
        E[k, b, a] += 0.5
    return E


class StressTensor:
    """Stress tensor and pressure of the simulation cell, accumulated on the device over any number of walker batches: an accumulator
    for `run_inference(accumulators=...)` (VMC) and, without the wave-function term, `run_dmc(accumulators=...)` (the mixed estimate,
    on comb blocks).

        sigma_ab = < kin_ab + dE_ewald / d eps_ab > / V     (Ha / bohr^3),      P = -tr sigma / 3

    kin_ab = -sum_i Re(d_ia conj d_ib), d = grad log psi, is the integrated-by-parts kinetic tensor (<tr kin> = -2 <T>; valid under
    periodic and twisted boundary conditions) and dE_ewald / d eps the derivative of the Ewald sums of `ds_ewald` under a homogeneous
    strain eps of the cell, electrons and ions scaled along, with alpha, the G list and the minimal images held fixed
    (`DeviceSystem.stress`).  For a pure Coulomb Hamiltonian tr(dE_ewald / d eps) = -E_ewald, so P = (2 <T> + <V>) / (3 V): the virial
    theorem, which the truncated sums obey to their convergence error.
    sigma is the stress only for an exact psi: for a variational psi the energy also changes because psi at fixed parameters changes
    with the cell (its features, envelopes and k points), a bias first order in the error of the wave function.  The variance of
    the kinetic tensor is NOT the zero variance of E_L: kin fluctuates even for an exact psi.  All-electron ions only
    (`pseudopotential` must be None).

    Every `update` is ONE `ds_logpsi_grad` call and ONE `ds_stress` call; nothing is read back.  `net`: the object
    `make_solid_fermi_net` returns (or its `.apply`).

    `wavefunction_term=True` adds the missing term,

        sigma^tot_ab V = < kin + dE_ewald / d eps >_ab + 2 Re < conj(E_L - E)(O_ab - <O_ab>) >,   O_ab = d log psi_eps((1 + eps) x) / d eps_ab

    (the Jacobian of the normalisation is a constant and drops out of the covariance), with O by central differences over
    strained handles: `supercell.strained` and `DeviceSystem.for_network` for +-`strain_step` along each of the six components,
    TWELVE handles built once at the first update, O_k = [log psi_{+h}(x (1 + h E_k)) - log psi_{-h}(x (1 - h E_k))] / 2h with the
    phase difference taken modulo 2 pi.  Every `update` is then ONE BLOCK, as for `PrimitiveForces`: `local_energy` (unless the
    caller passes `energies`), `logpsi_grad`, `ds_stress` and TWELVE `logpsi` forwards, and appends one device row
    [n_good, sum Re E, sum Im E, sum total (6), sum t (6)], t = Re conj(E_b - mean E of the block) O_b.  `stress()` then also gives
    sigma_total and pressure_total with errors from reblocking the block series.  float64 handles only (a float32 forward loses the
    difference); VMC only: `run_dmc` refuses it (`vmc_only`)."""

    ROW_LEN = 15

    def __init__(self, net, params, pseudopotential=None, wavefunction_term=False, strain_step=1e-4):
        if pseudopotential is not None:
            raise NotImplementedError('StressTensor: the strain derivative of a semi-local pseudopotential is not implemented '
                                      '(all-electron ions only)')
        self.apply = getattr(net, 'apply', net)
        self.params = params
        if wavefunction_term:
            if getattr(self.apply, 'dtype', torch.float64) != torch.float64:
                raise ValueError('StressTensor(wavefunction_term=True) needs a float64 network: the central difference of log psi over '
                                 'a strain step of 1e-4 is below the resolution of a float32 forward')
            if not (np.isfinite(strain_step) and 0.0 < float(strain_step) < 0.1):
                raise ValueError(f'strain_step = {strain_step} must be positive and small')
        cell = self.apply.simulation_cell
        self._setup(np.asarray(cell.atom_coords(), np.float64), np.asarray(cell.atom_charges(), np.float64),
                    np.asarray(cell.a, np.float64), int(sum(cell.nelec)), wavefunction_term, strain_step)

    def _setup(self, atoms, charges, latvec, n_elec, wavefunction_term=False, strain_step=1e-4):
        self.atoms = np.asarray(atoms, np.float64).reshape(-1, 3)
        self.charges = np.asarray(charges, np.float64).reshape(-1)
        self.latvec = np.asarray(latvec, np.float64).reshape(3, 3)
        self.n_elec = int(n_elec)
        self.volume = float(abs(np.linalg.det(self.latvec)))
        self.wavefunction_term = bool(wavefunction_term)
        self.vmc_only = self.wavefunction_term                  # (read by `run_dmc`)
        self.strain_step = float(strain_step)
        self._strained = None                                   # [(system +h, F +h, system -h, F -h)] per component, on first use
        self.sums = torch.zeros(49, dtype=torch.float64)        # of `ds_stress`; moved to the walkers' device by the first update
        self.trace_sums = torch.zeros(2, dtype=torch.float64)   # sum and sum of squares of tr(total) over the good walkers (for P)
        self.blocks = []                                        # device rows, one per update (wavefunction_term)
        self.n_bad = torch.zeros(1, dtype=torch.int64)
        self.n_walkers = 0
        self.n_means = 1                    # block means subtracted per row: the ranks whose rows were added by reduce()
        self.reduced = False

    @property
    def rows(self):
        """(blocks, 15) float64 tensor of the block rows of the wave-function term (on the device of the walkers)."""
        if not self.blocks:
            return torch.zeros(0, self.ROW_LEN, dtype=torch.float64)
        return torch.stack(self.blocks)

    # ---- the strain derivative of log psi
    def strained_systems(self):
        """The twelve handles of the wave-function term, built once: per component k the `DeviceSystem` of the cell strained by
        +h E_k and by -h E_k (`strain_generators`), each with its deformation matrix 1 +- h E_k as a device tensor."""
        if self._strained is None:
            from .device import DeviceSystem
            from .supercell import strained
            base = self.apply.system
            out = []
            for E in strain_generators():
                pair = []
                for sgn in (+1.0, -1.0):
                    cell, klist = strained(self.apply.simulation_cell, self.apply.klist, sgn * self.strain_step * E)
                    sysd = DeviceSystem.for_network(cell, klist, self.apply.net_kw, torch.float64)
                    pair += [sysd, torch.as_tensor(np.eye(3) + sgn * self.strain_step * E, dtype=torch.float64, device=base.device)]
                out.append(tuple(pair))
            self._strained = out
        return self._strained

    def strain_log_derivative(self, x):
        """O (B, 6) complex128: d log psi_eps((1 + eps) x) / d eps_k at eps = 0 by central differences over the strained handles,
        twelve `logpsi` forwards; Re = d log|psi|, Im = d arg psi (the phase difference modulo 2 pi)."""
        B = x.shape[0]
        O = torch.empty(B, 6, dtype=torch.complex128, device=x.device)
        for k, (sp, Fp, sm, Fm) in enumerate(self.strained_systems()):
            lap, php = sp.logpsi(self.params, (x.reshape(B, -1, 3) @ Fp).reshape(B, -1))
            lam, phm = sm.logpsi(self.params, (x.reshape(B, -1, 3) @ Fm).reshape(B, -1))
            dph = torch.angle(torch.view_as_complex(php.contiguous()) * torch.view_as_complex(phm.contiguous()).conj())
            O[:, k] = torch.complex(lap - lam, dph) / (2.0 * self.strain_step)
        return O

    # ---- accumulation
    def update(self, data, energies=None):
        """Add the tensors of every walker of `data` (B, 3N) to the sums: one `ds_logpsi_grad` and one `ds_stress` call, no device ->
        host copy.  With the wave-function term the call is one block (see the class); `energies` (B,) complex: the walkers'
        local energies when the caller has them (used by the wave-function term only)."""
        if self.apply is None:
            raise RuntimeError('StressTensor.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('StressTensor.update after reduce(): the sums are already summed over the ranks')
        if data.shape[-1] != 3 * self.n_elec:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {self.n_elec} electrons')
        x = data.reshape(-1, 3 * self.n_elec)
        B = x.shape[0]
        if B == 0:
            return
        if self.sums.device != x.device:
            self.sums, self.trace_sums, self.n_bad = self.sums.to(x.device), self.trace_sums.to(x.device), self.n_bad.to(x.device)
        system = self.apply.system
        if self.wavefunction_term:
            self.strained_systems()             # (before anything is added: a failure leaves the accumulator as it was)
            if energies is None:
                ke, ew, _, _ = system.local_energy(self.params, x)
                E = torch.complex(ke[:, 0].double() + ew.double(), ke[:, 1].double())
            else:
                E = torch.as_tensor(energies).to(device=x.device, dtype=torch.complex128).reshape(B)
        grad = system.logpsi_grad(self.params, x)[1]
        out = system.stress(x, grad, sums=self.sums, want_walker=True)
        total = out['parts'][:, 3]
        finite = torch.isfinite(total).all(1)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        tr = torch.where(finite, total[:, :3].sum(dim=1), zero)             # (a bad walker's rows are NaN: left out)
        self.trace_sums += torch.stack([tr.sum(), (tr * tr).sum()])
        self.n_bad += out['n_bad']
        if self.wavefunction_term:
            O = self.strain_log_derivative(x)
            good = finite & torch.isfinite(E.real) & torch.isfinite(E.imag) & torch.isfinite(O.real).all(1) & torch.isfinite(O.imag).all(1)
            n = good.sum().to(torch.float64)
            Er, Ei = torch.where(good, E.real, zero), torch.where(good, E.imag, zero)
            sr, si = Er.sum(), Ei.sum()
            dr, di = torch.where(good, Er - sr / n, zero), torch.where(good, Ei - si / n, zero)
            g2 = good[:, None]
            t = (dr[:, None] * torch.where(g2, O.real, zero) + di[:, None] * torch.where(g2, O.imag, zero)).sum(0)    # Re conj(dE) O
            self.blocks.append(torch.cat([torch.stack([n, sr, si]), torch.where(g2, total, zero).sum(0), t]))
        self.n_walkers += int(B)                    # only now: a call that raised leaves the count with the sums

    def _same_setup(self, other):
        return (self.atoms.shape == other.atoms.shape and np.array_equal(self.atoms, other.atoms) and
                np.array_equal(self.charges, other.charges) and np.array_equal(self.latvec, other.latvec) and
                self.n_elec == other.n_elec and self.wavefunction_term == other.wavefunction_term and
                (not self.wavefunction_term or self.strain_step == other.strain_step))

    def merge(self, other):
        """Add the sums, the bad count and the walker number of another accumulator of the same ions and lattice (and the same
        wave-function term and strain step; its blocks continue this one's series).  Both sides must be in the same state (rank-local
        or summed over the ranks), as for `IonForces.merge`."""
        if not self._same_setup(other):
            raise ValueError('StressTensor.merge: the two accumulators differ in ions, lattice, electron number or wave-function term')
        if self.reduced != other.reduced and constants.world_size() > 1 or self.n_means != other.n_means:
            raise ValueError('StressTensor.merge: one side is summed over the ranks and the other is rank-local')
        self.sums = self.sums + other.sums.to(self.sums.device)
        self.trace_sums = self.trace_sums + other.trace_sums.to(self.trace_sums.device)
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        dev = self.blocks[0].device if self.blocks else (other.blocks[0].device if other.blocks else None)
        self.blocks = self.blocks + [b.to(dev) for b in other.blocks]
        self.n_walkers += other.n_walkers
        return self

    def reduce(self):
        """Sum the sums, the block rows (block by block: every rank must hold the same number), the bad count and the walker number
        over the ranks in ONE packed float64 all-reduce (counts below 2^53 are exact; the identity at world size 1).  Once per
        accumulator: a second call raises."""
        if self.reduced:
            raise RuntimeError('StressTensor.reduce was already called: reducing twice would count every rank again')
        W = constants.world_size()
        if W > 1:
            dev = self.sums.device if self.sums.is_cuda else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
            rows = self.rows.to(dev)
            nb = float(rows.shape[0])
            packed = torch.cat([self.sums.to(dev), self.trace_sums.to(dev), self.n_bad.to(dev, torch.float64),
                                torch.tensor([self.n_walkers, nb, nb * nb], dtype=torch.float64, device=dev)])
            packed = constants.psum_if_pmap(packed)
            if float(packed[53]) != W * nb or float(packed[54]) != W * nb * nb:
                raise RuntimeError('StressTensor.reduce: the ranks hold different numbers of blocks')
            if rows.numel():
                self.blocks = list(constants.psum_if_pmap(rows.reshape(-1)).reshape(rows.shape).clone())
                self.n_means = self.n_means * W
            self.sums = packed[:49].clone()
            self.trace_sums = packed[49:51].clone()
            self.n_bad = packed[51:52].round().to(torch.int64)
            self.n_walkers = int(packed[52].round())
        self.reduced = True                 # only now: a collective that raised leaves the accumulator as it was
        return self

    # ---- normalisation (host)
    def stress(self):
        """-> dict(sigma (3, 3) float64 in Ha / bohr^3 = the mean of the total row over the volume, sigma_error, parts = dict(kin, ee, ei
        (3, 3) means over the volume, ii the ion-ion constant likewise, and kin_error, ee_error, ei_error), pressure = -tr sigma / 3 and
        pressure_error (Ha / bohr^3), pressure_gpa and pressure_gpa_error (`constants.HARTREE_PER_BOHR3_IN_GPA`), volume (bohr^3),
        n_walkers, n_bad).  Means are over the n_good walkers whose tensors were finite; every error is
        sqrt((sum t^2 / n_good - mean^2) / (n_good - 1)), a NAIVE standard error over walkers -- it takes them as independent and
        ignores the autocorrelation of the Markov chain, so it is a lower bound on a real run (NaN below two good walkers).  The
        pressure's error comes from the walkers' own traces, not from the component errors (which are correlated).  NaN everywhere
        without a good walker.  sigma does not hold the wave-function term.
        With `wavefunction_term` also: sigma_total = sigma + wavefunction (3, 3), per block sum total / n / V and
        2 sum t / (n - 1) / V (the block's own mean energy was subtracted: the unbiased covariance), averaged over the blocks weighted
        by n_good; sigma_total_error, wavefunction_error, pressure_total, pressure_total_error and pressure_total_gpa, the errors by
        `dmc.reblock` over the block series (below eight blocks the plain standard error of the series, NaN for a single block);
        n_blocks.  Blocks with n <= 1 good walkers are left out; NaN without a block."""
        s = self.sums.detach().cpu().numpy()
        t = self.trace_sums.detach().cpu().numpy()
        n = float(s[48])
        V = self.volume
        q = s[:48].reshape(4, 6, 2)
        nan33 = np.full((3, 3), np.nan)
        gpa = constants.HARTREE_PER_BOHR3_IN_GPA
        out = dict(volume=V, n_walkers=self.n_walkers, n_bad=int(self.n_bad.sum()))
        if n < 1:
            out.update(sigma=nan33, sigma_error=nan33.copy(), pressure=np.nan, pressure_error=np.nan, pressure_gpa=np.nan,
                       pressure_gpa_error=np.nan,
                       parts={k: nan33.copy() for k in ('kin', 'ee', 'ei', 'ii', 'kin_error', 'ee_error', 'ei_error')})
        else:
            mean = q[:, :, 0] / n
            var = np.maximum(q[:, :, 1] / n - mean * mean, 0.0)
            err = np.sqrt(var / (n - 1)) if n > 1 else np.full((4, 6), np.nan)
            m33, e33 = voigt_to_matrix(mean) / V, voigt_to_matrix(err) / V
            parts = {name: m33[k] for k, name in enumerate(STRESS_ROWS[:3])}
            parts.update({name + '_error': e33[k] for k, name in enumerate(STRESS_ROWS[:3])})
            parts['ii'] = m33[3] - ((m33[0] + m33[1]) + m33[2])
            tr_mean = t[0] / n
            tr_err = np.sqrt(max(t[1] / n - tr_mean * tr_mean, 0.0) / (n - 1)) if n > 1 else np.nan
            pressure = -np.trace(m33[3]) / 3.0
            out.update(sigma=m33[3], sigma_error=e33[3], parts=parts, pressure=pressure, pressure_error=tr_err / (3.0 * V),
                       pressure_gpa=pressure * gpa, pressure_gpa_error=tr_err / (3.0 * V) * gpa)
        if self.wavefunction_term:
            from .dmc import reblock
            rows = self.rows.detach().cpu().numpy().reshape(-1, self.ROW_LEN)
            rows = rows[rows[:, 0] > self.n_means]
            out['n_blocks'] = int(rows.shape[0])
            if rows.shape[0] == 0:
                out.update(sigma_total=nan33.copy(), sigma_total_error=nan33.copy(), wavefunction=nan33.copy(),
                           wavefunction_error=nan33.copy(), pressure_total=np.nan, pressure_total_error=np.nan, pressure_total_gpa=np.nan)
                return out
            nb = rows[:, 0]
            series = {'wavefunction': 2.0 * rows[:, 9:15] / (nb - self.n_means)[:, None] / V}
            series['sigma_total'] = rows[:, 3:9] / nb[:, None] / V + series['wavefunction']
            lvl = min(8, max(2, len(nb)))
            for k, v in series.items():
                out[k] = voigt_to_matrix((v * nb[:, None]).sum(0) / nb.sum())
                out[k + '_error'] = voigt_to_matrix(np.array([reblock(v[:, c], min_blocks=lvl)[1] for c in range(6)]))
            p = -series['sigma_total'][:, :3].sum(1) / 3.0
            out['pressure_total'] = float((p * nb).sum() / nb.sum())
            out['pressure_total_error'] = float(reblock(p, min_blocks=lvl)[1])
            out['pressure_total_gpa'] = out['pressure_total'] * gpa
        return out

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the sums, block rows and counts and the setup they belong to."""
        return {'sums': self.sums.detach().cpu().numpy().copy(), 'trace_sums': self.trace_sums.detach().cpu().numpy().copy(),
                'rows': self.rows.detach().cpu().numpy().copy(), 'n_means': np.int64(self.n_means),
                'n_bad': self.n_bad.detach().cpu().numpy().copy(), 'n_walkers': np.int64(self.n_walkers), 'atoms': self.atoms.copy(),
                'charges': self.charges.copy(), 'latvec': self.latvec.copy(), 'n_elec': np.int64(self.n_elec),
                'wavefunction_term': np.bool_(self.wavefunction_term), 'strain_step': np.float64(self.strain_step),
                'reduced': np.bool_(self.reduced)}

    def load_state_dict(self, sd):
        """Replace the sums, rows and counts by those of `sd` (same ions, lattice and wave-function term); the accumulator is
        rank-local and open for `update` afterwards."""
        other = StressTensor.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('StressTensor.load_state_dict: the state belongs to other ions, another lattice or another wave-function term')
        self.sums, self.trace_sums = other.sums.to(self.sums.device), other.trace_sums.to(self.trace_sums.device)
        self.n_bad = other.n_bad.to(self.n_bad.device)
        self.blocks, self.n_means = other.blocks, other.n_means
        self.n_walkers, self.reduced = other.n_walkers, False
        return self

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = None
        acc._setup(sd['atoms'], sd['charges'], sd['latvec'], int(sd['n_elec']),
                   bool(sd['wavefunction_term']) if 'wavefunction_term' in sd else False,
                   float(sd['strain_step']) if 'strain_step' in sd else 1e-4)
        acc.sums = torch.as_tensor(np.array(sd['sums'], dtype=np.float64).reshape(49))
        acc.trace_sums = torch.as_tensor(np.array(sd['trace_sums'], dtype=np.float64).reshape(2))
        if 'rows' in sd:
            acc.blocks = list(torch.as_tensor(np.array(sd['rows'], dtype=np.float64).reshape(-1, cls.ROW_LEN)))
        acc.n_means = int(sd['n_means']) if 'n_means' in sd else 1
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(1))
        acc.n_walkers = int(sd['n_walkers'])
        return acc                          # reduced stays False: the loaded sums are this rank's contribution from here on

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also the arrays and numbers of `stress()` (but its `parts`)."""
        sd = self.state_dict()
        if results:
            r = self.stress()
            sd.update({k: np.asarray(v, np.float64) for k, v in r.items() if k not in ('parts', 'n_walkers', 'n_bad')})
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path` as a fresh rank-local one without a network (see `from_state_dict`)."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})


# ------------------------------------------------------------------ total force on the primitive-cell atoms (csrc/ds_iongrad.h)
def primitive_fold(sim_atoms, prim_atoms, prim_latvec):
    """-> (owner (As,) int: the primitive atom each ion of the simulation cell is an image of, scale = As / A).  `get_supercell`
    orders the ions atom-major, so image s belongs to atom s // scale; that is ASSERTED here: sim_atoms[s] - prim_atoms[s // scale]
    must be a lattice vector of the primitive cell, otherwise ValueError (a cell built in another order would fold forces onto
    the wrong atoms without any other symptom)."""
    sim_atoms = np.asarray(sim_atoms, np.float64).reshape(-1, 3)
    prim_atoms = np.asarray(prim_atoms, np.float64).reshape(-1, 3)
    As, A = sim_atoms.shape[0], prim_atoms.shape[0]
    if A < 1 or As % A:
        raise ValueError(f'{As} ions in the simulation cell are not a multiple of the {A} atoms of the primitive cell')
    scale = As // A
    owner = np.arange(As) // scale
    frac = (sim_atoms - prim_atoms[owner]) @ np.linalg.inv(np.asarray(prim_latvec, np.float64).reshape(3, 3))
    off = np.abs(frac - np.round(frac)).max(axis=1)
    if off.max() > 1e-8:
        s = int(off.argmax())
        raise ValueError(f'ion {s} of the simulation cell is not a lattice translate of primitive atom {s // scale}: the ions are not '
                         'ordered atom-major (get_supercell), the fold onto the primitive atoms would be wrong')
    return owner, scale


class PrimitiveForces:
    """The total force on each atom of the PRIMITIVE cell per simulation cell, zero-variance force plus Pulay term, accumulated on
    the device over walker batches: an accumulator for `run_inference(accumulators=...)`.

        F_a = sum_{s image of a} F^zv_s  -  2 Re < conj(E_L - E) (O_a - <O_a>) >,     O_a = d log psi / d R_a (complex)

    F^zv is `IonForces`' zero-variance force on the ions of the simulation cell, E_L = ke + ewald the complex local energy and O_a
    `DeviceSystem.logpsi_ion_grad`.  For a complex psi the piece 2 <Im E_L d arg psi> belongs to <Re d E_L / dR> and is kept: the
    formula is the parameter gradient of `train.make_loss` with theta = R.
    WHICH ATOMS: the network's atoms are the A atoms of the primitive cell and its features are periodic in the primitive lattice,
    so moving atom a moves all `scale` images of it in the simulation cell together; the derivative of psi in a single ion of a
    supercell does not exist in this ansatz.  The result is the q = 0 force that internal-coordinate relaxation needs.  The ions
    of the simulation cell are atom-major (`primitive_fold` asserts it at construction).  All-electron ions only.

    Every `update` is ONE BLOCK and runs four calls: `local_energy` (unless the caller passes its complex `energies`),
    `logpsi_grad`, `ion_forces(want_walker=True)` and one `logpsi_ion_vjp` with cot_b = E_b - mean E of the block, whose batch sum
    is the covariance numerator sum_b Re conj(E_b - E) O_b (the mean of O drops out: sum_b (E_b - E) = 0), so no second sweep is
    needed.  Walkers that `ion_forces` marks bad (or whose energy is not finite) are left out of every sum of the block.  The
    block appends one device row [n_good, sum Re E, sum Im E, per (a, c): sum zv, sum hf, sum t]; nothing is read back.
    VMC ONLY: the Pulay term is a covariance under |psi|^2.  The accumulators of `run_dmc` deliver mixed estimates of plain
    averages; a mixed estimate of a covariance term is not the DMC force, and this class does not pretend to give one."""

    def __init__(self, net, params, cutoff=None):
        self.apply = getattr(net, 'apply', net)
        self.params = params
        cell = self.apply.simulation_cell
        prim = cell.original_cell
        self._setup(np.asarray(cell.atom_coords(), np.float64), np.asarray(cell.atom_charges(), np.float64), np.asarray(cell.a, np.float64),
                    np.asarray(prim.atom_coords(), np.float64), np.asarray(prim.a, np.float64), int(sum(cell.nelec)), cutoff)

    def _setup(self, sim_atoms, charges, latvec, prim_atoms, prim_latvec, n_elec, cutoff):
        self.sim_atoms = np.asarray(sim_atoms, np.float64).reshape(-1, 3)
        self.charges = np.asarray(charges, np.float64).reshape(-1)
        self.latvec = np.asarray(latvec, np.float64).reshape(3, 3)
        self.atoms = np.asarray(prim_atoms, np.float64).reshape(-1, 3)
        self.prim_latvec = np.asarray(prim_latvec, np.float64).reshape(3, 3)
        self.owner, self.scale = primitive_fold(self.sim_atoms, self.atoms, self.prim_latvec)
        self.n_elec = int(n_elec)
        self.cutoff = force_cutoff(self.latvec, cutoff)
        self.n_atoms = self.atoms.shape[0]
        self.row_len = 3 + 9 * self.n_atoms
        self.blocks = []                    # device rows, one per update
        self.n_bad = torch.zeros(1, dtype=torch.int64)
        self.n_walkers = 0
        self.n_means = 1                    # block means subtracted per row: the ranks whose rows were added by reduce()
        self.reduced = False

    @property
    def rows(self):
        """(blocks, 3 + 9 A) float64 tensor of the block rows (on the device of the walkers)."""
        if not self.blocks:
            return torch.zeros(0, self.row_len, dtype=torch.float64)
        return torch.stack(self.blocks)

    # ---- accumulation
    def update(self, data, energies=None):
        """One block from the walkers `data` (B, 3N); `energies` (B,) complex: their local energies when the caller has them."""
        if self.apply is None:
            raise RuntimeError('PrimitiveForces.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('PrimitiveForces.update after reduce(): the rows are already summed over the ranks')
        if data.shape[-1] != 3 * self.n_elec:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {self.n_elec} electrons')
        x = data.reshape(-1, 3 * self.n_elec)
        B = x.shape[0]
        if B == 0:
            return
        system = self.apply.system
        if energies is None:
            ke, ew, _, _ = system.local_energy(self.params, x)
            E = torch.complex(ke[:, 0].double() + ew.double(), ke[:, 1].double())
        else:
            E = torch.as_tensor(energies).to(device=x.device, dtype=torch.complex128).reshape(B)
        drift = system.logpsi_grad(self.params, x)[1].real.contiguous()
        f = system.ion_forces(x, drift, cutoff=self.cutoff, want_walker=True)
        A, sc = self.n_atoms, self.scale
        good = torch.isfinite(f['zv']).all(2).all(1) & torch.isfinite(f['hf']).all(2).all(1) & torch.isfinite(E.real) & torch.isfinite(E.imag)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        w3 = good[:, None, None]
        zv = torch.where(w3, f['zv'].reshape(B, A, sc, 3).sum(2), zero).sum(0)          # atom-major: image s of atom s // scale
        hf = torch.where(w3, f['hf'].reshape(B, A, sc, 3).sum(2), zero).sum(0)
        n = good.sum().to(torch.float64)
        Er, Ei = torch.where(good, E.real, zero), torch.where(good, E.imag, zero)
        sr, si = Er.sum(), Ei.sum()
        cot = torch.stack([torch.where(good, Er - sr / n, zero), torch.where(good, Ei - si / n, zero)], 1)
        O = system.logpsi_ion_vjp(self.params, x, cot)[0]
        t = torch.where(w3, O, zero).sum(0)
        row = torch.cat([torch.stack([n, sr, si]), torch.stack([zv, hf, t], 2).reshape(-1)])
        self.blocks.append(row)
        if self.n_bad.device != x.device:
            self.n_bad = self.n_bad.to(x.device)
        self.n_bad += (B - good.sum()).reshape(1)
        self.n_walkers += int(B)

    def _same_setup(self, other):
        return (self.sim_atoms.shape == other.sim_atoms.shape and np.array_equal(self.sim_atoms, other.sim_atoms) and
                self.atoms.shape == other.atoms.shape and np.array_equal(self.atoms, other.atoms) and
                np.array_equal(self.charges, other.charges) and np.array_equal(self.latvec, other.latvec) and
                np.array_equal(self.prim_latvec, other.prim_latvec) and self.n_elec == other.n_elec and self.cutoff == other.cutoff)

    def merge(self, other):
        """Append the blocks of another accumulator of the same cell and cutoff (its series continues this one's), add its counts."""
        if not self._same_setup(other):
            raise ValueError('PrimitiveForces.merge: the two accumulators differ in atoms, lattice, electron number or cutoff')
        if self.reduced != other.reduced and constants.world_size() > 1 or self.n_means != other.n_means:
            raise ValueError('PrimitiveForces.merge: one side is summed over the ranks and the other is rank-local')
        dev = self.blocks[0].device if self.blocks else (other.blocks[0].device if other.blocks else None)
        self.blocks = self.blocks + [b.to(dev) for b in other.blocks]
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        self.n_walkers += other.n_walkers
        return self

    def reduce(self):
        """Add the rows of all ranks block by block (every rank must hold the same number of blocks), the bad count and the walker
        number, in one packed float64 all-reduce.  A summed row holds one subtracted mean per rank: `forces()` divides the Pulay
        sums by n - ranks.  Once per accumulator: a second call raises; so does `update` afterwards."""
        if self.reduced:
            raise RuntimeError('PrimitiveForces.reduce was already called: reducing twice would count every rank again')
        W = constants.world_size()
        if W > 1:
            rows = self.rows
            dev = rows.device if rows.is_cuda else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
            nb = float(rows.shape[0])
            head = constants.psum_if_pmap(torch.tensor([nb, nb * nb], dtype=torch.float64, device=dev))
            if float(head[0]) != W * nb or float(head[1]) != W * nb * nb:
                raise RuntimeError('PrimitiveForces.reduce: the ranks hold different numbers of blocks')
            packed = torch.cat([rows.to(dev).reshape(-1), self.n_bad.to(dev, torch.float64),
                                torch.tensor([self.n_walkers], dtype=torch.float64, device=dev)])
            packed = constants.psum_if_pmap(packed)
            k = rows.numel()
            self.blocks = list(packed[:k].reshape(rows.shape).clone())
            self.n_bad = packed[k:k + 1].round().to(torch.int64)
            self.n_walkers = int(packed[k + 1].round())
            self.n_means = self.n_means * W
        self.reduced = True
        return self

    # ---- normalisation (host)
    def forces(self):
        """-> dict(total, zv, hf, pulay and their *_error (each (A, 3) float64, Ha/bohr, per primitive atom and simulation cell),
        energy (complex block-weighted mean), n_blocks, n_walkers, n_bad, atoms (A, 3) of the primitive cell, cutoff).
        Per block zv = sum zv / n, hf = sum hf / n, pulay = -2 sum t / (n - 1) (the block's own mean energy was subtracted: the
        unbiased covariance), total = zv + pulay; each is averaged over the blocks weighted by n_good.  The error is `dmc.reblock`
        over the block series: the blocks of a Markov chain are correlated and a covariance estimator has no per-walker variance
        to fall back on (below eight blocks there is no level to halve to: the error is then the plain standard error of the block
        series, NaN for a single block).  Blocks with too few good walkers for a covariance (n <= 1) are left out; NaN without a block."""
        from .dmc import reblock
        rows = self.rows.detach().cpu().numpy().reshape(-1, self.row_len)
        A = self.n_atoms
        rows = rows[rows[:, 0] > self.n_means]
        out = dict(n_blocks=int(rows.shape[0]), n_walkers=self.n_walkers, n_bad=int(self.n_bad.sum()), atoms=self.atoms.copy(),
                   cutoff=self.cutoff)
        names = ('total', 'zv', 'hf', 'pulay')
        if rows.shape[0] == 0:
            for k in names:
                out[k] = np.full((A, 3), np.nan)
                out[k + '_error'] = np.full((A, 3), np.nan)
            out['energy'] = complex(np.nan, np.nan)
            return out
        n = rows[:, 0]
        body = rows[:, 3:].reshape(-1, A, 3, 3)
        series = {'zv': body[..., 0] / n[:, None, None], 'hf': body[..., 1] / n[:, None, None],
                  'pulay': -2.0 * body[..., 2] / (n - self.n_means)[:, None, None]}
        series['total'] = series['zv'] + series['pulay']
        for k in names:
            v = series[k]
            out[k] = (v * n[:, None, None]).sum(0) / n.sum()
            out[k + '_error'] = np.array([[reblock(v[:, a, c], min_blocks=min(8, max(2, len(v))))[1] for c in range(3)] for a in range(A)])
        out['energy'] = complex(rows[:, 1].sum() / n.sum(), rows[:, 2].sum() / n.sum())
        return out

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the block rows and counts and the setup they belong to."""
        return {'rows': self.rows.detach().cpu().numpy().copy(), 'n_bad': self.n_bad.detach().cpu().numpy().copy(),
                'n_walkers': np.int64(self.n_walkers), 'n_means': np.int64(self.n_means), 'atoms': self.atoms.copy(),
                'sim_atoms': self.sim_atoms.copy(), 'charges': self.charges.copy(), 'latvec': self.latvec.copy(),
                'prim_latvec': self.prim_latvec.copy(), 'n_elec': np.int64(self.n_elec), 'cutoff': np.float64(self.cutoff),
                'reduced': np.bool_(self.reduced)}

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = None
        acc._setup(sd['sim_atoms'], sd['charges'], sd['latvec'], sd['atoms'], sd['prim_latvec'], int(sd['n_elec']), float(sd['cutoff']))
        acc.blocks = list(torch.as_tensor(np.array(sd['rows'], dtype=np.float64).reshape(-1, acc.row_len)))
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(1))
        acc.n_walkers = int(sd['n_walkers'])
        acc.n_means = int(sd['n_means'])
        return acc

    def load_state_dict(self, sd):
        """Replace the rows and counts by those of `sd` (same cell and cutoff); the accumulator is open for `update` afterwards."""
        other = PrimitiveForces.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('PrimitiveForces.load_state_dict: the state belongs to other atoms, another lattice or another cutoff')
        self.blocks, self.n_bad = other.blocks, other.n_bad
        self.n_walkers, self.n_means, self.reduced = other.n_walkers, other.n_means, False
        return self

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also the arrays of `forces()`."""
        sd = self.state_dict()
        if results:
            r = self.forces()
            sd.update({k: r[k] for k in r if k not in ('atoms', 'cutoff', 'n_walkers', 'n_bad')})
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path` as a fresh one without a network (see `from_state_dict`)."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})


# ------------------------------------------------------------------ one-body density matrix (csrc/ds_obdm.h)
# The reference has no such estimator; the conventions of this section are this project's own.
def _integer_matrix(m, what, tol=1e-8):
    r = np.rint(m)
    if not np.all(np.abs(m - r) <= tol):
        raise ValueError(f'OneBodyDensityMatrix: {what} (largest distance from an integer {float(np.abs(m - r).max()):.3e})')
    return r


class OneBodyDensityMatrix:
    """Spin-resolved one-body reduced density matrix of a network's wavefunction in a basis of crystalline orbitals, accumulated on
    the device over any number of walker batches: an accumulator for `run_inference(accumulators=...)`.

    `basis`: a `hf.GaussianOrbitals`; its columns per spin are the basis functions phi^s_i (M_s <= 64 of them, `basis.nelec` =
    (M_up, M_dn)), not necessarily occupied or orthonormal and independent of the network's electron numbers.  With
    chi = phi / sqrt(Omega_S / Omega_p), Omega_p = |det basis.a| (PySCF normalises an orbital over that cell),

        n^s_ij = < sum_{e in s} int_{Omega_S} dr' chi_i*(r') chi_j(r_e) psi(.., r_e -> r', ..) / psi(R) >,
        S^s_ij = int_{Omega_S} dr' chi_i*(r') chi_j(r').

    Every `update` is ONE `ds_one_body_ratios` call that moves, per walker, `samples_per_walker` = M electrons in turn (default N)
    by shifts uniform in the simulation cell and exports (q, s), and ONE `ds_obdm_accumulate` call that folds them with the basis
    at r_e and r' into float64 sums; nothing is read back.  The Philox offset advances by 1 per update, `first_electron` by M mod
    N, the seed is decorrelated over the ranks as in `MomentumDistribution`.  `net`: the object `make_solid_fermi_net` returns
    (or its `.apply`).

    Refused at construction (ValueError), since the integrand is periodic over the simulation cell only then: a simulation cell
    that is not a superlattice of the basis's cell (`sim.a @ inv(basis.a)` integer to 1e-8), a basis k point that is not
    Bloch-allowed ((k - k_t) . a_S / 2 pi integer to 1e-8, k_t the first `klist` entry), more than 64 basis functions per spin.

    Limits: uniform r' has a large variance for core orbitals of all-electron ions (of order Omega_S over the orbital's volume) --
    valence bands and pseudopotential cells are the use case; importance-sampled r' enters through `update(data, shifts=...,
    weights=...)`.  No error bars (merge several accumulators).  Under `run_dmc` the result is the mixed estimate."""

    MAX_ORB = 64

    def __init__(self, net, params, basis, samples_per_walker=None, seed=0):
        self.apply = getattr(net, 'apply', net)
        self.params = params
        self.basis = basis
        cell = self.apply.simulation_cell
        self._setup((int(cell.nelec[0]), int(cell.nelec[1])), cell.a, basis.a, basis.kpts, basis.nelec, samples_per_walker)
        ratio = self.sim_a @ np.linalg.inv(self.basis_a)
        _integer_matrix(ratio, 'the simulation cell is not a superlattice of the basis cell: sim.a @ inv(basis.a) is not an integer matrix')
        kl = [np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in self.apply.klist]
        kt = np.concatenate(kl, axis=0)[0]
        _integer_matrix((self.basis_kpts - kt[None, :]) @ self.sim_a.T / (2.0 * np.pi),
                        'a basis k point is not Bloch-allowed: (k - k_t) . a_S / 2 pi is not an integer vector')
        self.seed = (int(seed) * max(1, constants.world_size()) + constants.rank()) % (1 << 63)

    def _setup(self, nelec, sim_a, basis_a, basis_kpts, norb, samples_per_walker):
        self.nelec = (int(nelec[0]), int(nelec[1]))
        self.sim_a = np.array(sim_a, dtype=np.float64).reshape(3, 3)
        self.basis_a = np.array(basis_a, dtype=np.float64).reshape(3, 3)
        self.basis_kpts = np.ascontiguousarray(np.asarray(basis_kpts, dtype=np.float64).reshape(-1, 3))
        self.norb = (int(norb[0]), int(norb[1]))
        if min(self.norb) < 0 or max(self.norb) < 1 or max(self.norb) > self.MAX_ORB:
            raise ValueError(f'OneBodyDensityMatrix: {self.norb} basis functions per spin; 0..{self.MAX_ORB} (one at least) are supported')
        n_el = sum(self.nelec)
        self.samples_per_walker = n_el if samples_per_walker is None else int(samples_per_walker)
        if self.samples_per_walker < 1:
            raise ValueError(f'samples_per_walker = {samples_per_walker} must be >= 1')
        mb = max(self.norb)
        self.dm_sums = torch.zeros(2, mb, mb, 2, dtype=torch.float64)      # moved to the walkers' device by the first update
        self.ov_sums = torch.zeros(2, mb, mb, 2, dtype=torch.float64)
        self.n_bad = torch.zeros(2, dtype=torch.int64)
        self.samples = np.zeros(2, dtype=np.int64)
        self.offset = 0
        self.first_electron = 0
        self.seed = 0
        self.reduced = False

    # ---- accumulation
    def update(self, data, shifts=None, weights=None):
        """Add `samples_per_walker` samples of every walker of `data` (B, 3N) to the sums: two library calls, no device -> host
        copy.  `shifts` (B, M, 3) replaces the uniform shifts by the caller's, drawn from a density p(s); `weights` (B, M) float64
        then holds 1 / (Omega_S p(s)).  The samples per spin are counted on the host: they follow from first_electron alone."""
        if self.apply is None:
            raise RuntimeError('OneBodyDensityMatrix.update: a loaded accumulator has no network; merge it into one that has')
        if self.reduced:
            raise RuntimeError('OneBodyDensityMatrix.update after reduce(): the sums are already summed over the ranks')
        n_el, m = sum(self.nelec), self.samples_per_walker
        if data.shape[-1] != 3 * n_el:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {n_el} electrons')
        x = data.reshape(-1, 3 * n_el)
        sysd = self.apply.system
        if self.dm_sums.device != x.device:
            self.dm_sums, self.ov_sums, self.n_bad = self.dm_sums.to(x.device), self.ov_sums.to(x.device), self.n_bad.to(x.device)
        out = sysd.one_body_ratios(self.params, x, m, first_electron=self.first_electron, seed=self.seed, offset=self.offset,
                                   shifts=shifts, want_ratios=True, want_shifts=True)
        if weights is not None:
            weights = weights.to(device=x.device, dtype=torch.float64)
        res = self.basis._device_tables(x.device).obdm_accumulate(x, self.nelec, m, self.first_electron, out['ratios'], out['shifts'],
                                                                  weights=weights, dm_sums=self.dm_sums, ov_sums=self.ov_sums)
        self.n_bad += res['n_bad']
        up = int(np.count_nonzero((self.first_electron + np.arange(m)) % n_el < self.nelec[0]))
        self.samples += np.asarray([up, m - up], dtype=np.int64) * int(x.shape[0])
        self.offset += 1
        self.first_electron = (self.first_electron + m) % n_el

    def _same_setup(self, other):
        """Electron numbers, both lattices, the basis's k points and its functions per spin.  (The orbital coefficients are not
        part of the state: merging sums of two different bases on the same k points is the caller's error.)"""
        return self.nelec == other.nelec and self.norb == other.norb and np.array_equal(self.sim_a, other.sim_a) and \
            np.array_equal(self.basis_a, other.basis_a) and np.array_equal(self.basis_kpts, other.basis_kpts)

    def merge(self, other):
        """Add the sums, sample counts and bad counts of another accumulator of the same setup.  Both sides must be in the same
        state (rank-local or summed over the ranks), as for `RealSpaceAccumulator.merge`."""
        if not self._same_setup(other):
            raise ValueError('OneBodyDensityMatrix.merge: the two accumulators differ in electron numbers, cells or basis')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('OneBodyDensityMatrix.merge: one side is summed over the ranks and the other is rank-local')
        self.dm_sums = self.dm_sums + other.dm_sums.to(self.dm_sums.device)
        self.ov_sums = self.ov_sums + other.ov_sums.to(self.ov_sums.device)
        self.n_bad = self.n_bad + other.n_bad.to(self.n_bad.device)
        self.samples = self.samples + other.samples
        return self

    def reduce(self):
        """Sum both sums, the bad counts and the sample counts over the ranks in ONE packed float64 all-reduce (counts below 2^53
        are exact; the identity at world size 1).  Once per accumulator: a second call raises."""
        if self.reduced:
            raise RuntimeError('OneBodyDensityMatrix.reduce was already called: reducing twice would count every rank again')
        if constants.world_size() > 1:
            dev = self.dm_sums.device if self.dm_sums.is_cuda else torch.device('cuda' if torch.cuda.is_available() else 'cpu')
            n = self.dm_sums.numel()
            packed = torch.cat([self.dm_sums.reshape(-1).to(dev), self.ov_sums.reshape(-1).to(dev), self.n_bad.to(dev, torch.float64),
                                torch.as_tensor(self.samples, dtype=torch.float64, device=dev)])
            packed = constants.psum_if_pmap(packed)
            self.dm_sums = packed[:n].reshape(self.dm_sums.shape).clone()
            self.ov_sums = packed[n:2 * n].reshape(self.ov_sums.shape).clone()
            self.n_bad = packed[2 * n:2 * n + 2].round().to(torch.int64)
            self.samples = packed[2 * n + 2:2 * n + 4].round().cpu().numpy().astype(np.int64)
        self.reduced = True                 # only now: a collective that raised leaves the accumulator as it was
        return self

    # ---- normalisation (host)
    def _normalised(self, sums, electrons):
        s = sums.detach().cpu().numpy()
        good = self.samples - self.n_bad.detach().cpu().numpy()
        omega_p = abs(np.linalg.det(self.basis_a))
        out = []
        for sp in range(2):
            m = self.norb[sp]
            z = s[sp, :m, :m, 0] + 1j * s[sp, :m, :m, 1]
            scale = (self.nelec[sp] if electrons else 1.0) * omega_p
            out.append(scale * z / good[sp] if good[sp] > 0 else (np.zeros((m, m), np.complex128) if electrons and self.nelec[sp] == 0
                                                                   else np.full((m, m), np.nan, np.complex128)))
        return tuple(out)

    def density_matrix(self):
        """(n^up (M_up, M_up), n^dn (M_dn, M_dn)) complex128: n^s = N_s Omega_p dm_sums[s] / (samples on s - bad samples on s).
        A spin without electrons is 0, one without good samples NaN."""
        return self._normalised(self.dm_sums, True)

    def overlap(self):
        """(S^up, S^dn) complex128: S^s = Omega_p ov_sums[s] / (samples on s - bad samples on s), the sampled overlap of the basis
        over the simulation cell in the normalisation of `density_matrix`; NaN for a spin without good samples."""
        return self._normalised(self.ov_sums, False)

    def natural_orbitals(self, spin, overlap='sampled'):
        """-> (occupations (M,) descending, c (M, M)): the generalised Hermitian eigenproblem D c = S c diag(occ) with
        D = (n + n^dagger) / 2 and S = (S + S^dagger) / 2 of `overlap()` ('sampled') or the unit matrix ('identity': for a basis
        known to be orthonormal over its cell).  Column a of c holds the coefficients of natural orbital a in the basis functions;
        c^dagger S c = 1."""
        if overlap not in ('sampled', 'identity'):
            raise ValueError(f"overlap must be 'sampled' or 'identity', got {overlap!r}")
        n = self.density_matrix()[int(spin)]
        d = 0.5 * (n + n.conj().T)
        if overlap == 'identity':
            s = np.eye(d.shape[0], dtype=np.complex128)
        else:
            s = self.overlap()[int(spin)]
            s = 0.5 * (s + s.conj().T)
        low = np.linalg.cholesky(s)                                       # S = L L^dagger (raises if S is not positive definite)
        linv = np.linalg.inv(low)
        occ, v = np.linalg.eigh(linv @ d @ linv.conj().T)
        order = np.argsort(occ)[::-1]
        return occ[order], (linv.conj().T @ v)[:, order]

    # ---- persistence
    def state_dict(self):
        """Plain numpy arrays: the sums and counts, the setup they belong to and where the noise stream stands."""
        return {'dm_sums': self.dm_sums.detach().cpu().numpy().copy(), 'ov_sums': self.ov_sums.detach().cpu().numpy().copy(),
                'samples': self.samples.copy(), 'n_bad': self.n_bad.detach().cpu().numpy().copy(),
                'nelec': np.asarray(self.nelec, np.int64), 'simulation_lattice': self.sim_a.copy(), 'basis_lattice': self.basis_a.copy(),
                'basis_kpts': self.basis_kpts.copy(), 'basis_norb': np.asarray(self.norb, np.int64),
                'samples_per_walker': np.int64(self.samples_per_walker), 'offset': np.int64(self.offset),
                'first_electron': np.int64(self.first_electron), 'reduced': np.bool_(self.reduced)}

    def load_state_dict(self, sd):
        """Replace the sums, counts and stream position by those of `sd` (same setup); the accumulator is rank-local and open for
        `update` afterwards."""
        other = OneBodyDensityMatrix.from_state_dict(sd)
        if not self._same_setup(other):
            raise ValueError('OneBodyDensityMatrix.load_state_dict: the state belongs to other electron numbers, cells or basis')
        dev = self.dm_sums.device
        self.dm_sums, self.ov_sums, self.n_bad = other.dm_sums.to(dev), other.ov_sums.to(dev), other.n_bad.to(dev)
        self.samples = other.samples
        self.offset, self.first_electron, self.reduced = other.offset, other.first_electron, False
        return self

    @classmethod
    def from_state_dict(cls, sd):
        """An accumulator without a network or basis: it can be merged, normalised and saved, not updated."""
        acc = cls.__new__(cls)
        acc.apply = acc.params = acc.basis = None
        acc._setup(sd['nelec'], sd['simulation_lattice'], sd['basis_lattice'], sd['basis_kpts'], sd['basis_norb'],
                   int(sd['samples_per_walker']) if 'samples_per_walker' in sd else None)
        mb = max(acc.norb)
        acc.dm_sums = torch.as_tensor(np.array(sd['dm_sums'], dtype=np.float64).reshape(2, mb, mb, 2))
        acc.ov_sums = torch.as_tensor(np.array(sd['ov_sums'], dtype=np.float64).reshape(2, mb, mb, 2))
        acc.n_bad = torch.as_tensor(np.array(sd['n_bad'], dtype=np.int64).reshape(2))
        acc.samples = np.array(sd['samples'], dtype=np.int64).reshape(2)
        acc.offset = int(sd['offset']) if 'offset' in sd else 0
        acc.first_electron = int(sd['first_electron']) if 'first_electron' in sd else 0
        return acc                          # reduced stays False: the loaded sums are this rank's contribution from here on

    def save(self, path, results=True):
        """One .npz of `state_dict()`; `results`: also `dm_up`, `dm_dn`, `overlap_up`, `overlap_dn`, the normalised matrices."""
        sd = self.state_dict()
        if results:
            sd['dm_up'], sd['dm_dn'] = self.density_matrix()
            sd['overlap_up'], sd['overlap_dn'] = self.overlap()
        with open(path, 'wb') as f:
            np.savez(f, **sd)

    @classmethod
    def load(cls, path):
        """The accumulator saved at `path` as a fresh rank-local one without a network (see `from_state_dict`)."""
        with np.load(path) as f:
            return cls.from_state_dict({k: f[k] for k in f.files})
