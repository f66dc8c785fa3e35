"""Fixed-phase diffusion Monte Carlo on the device: host bookkeeping around `ds_dmc_step` (csrc/ds_dmc.h; the algorithm is stated
in include/deepsolid_hip.h and DESIGN.md section 19).  The reference has no DMC; the conventions are this project's own.

`make_dmc_step` returns the block function (one C-ABI call per block of steps; no host synchronisation inside WITHOUT a
pseudopotential -- with one, `ds_dmc_step_ecp` synchronises the stream once per step and once more for the initialisation, to
read the pair total of every pseudopotential evaluation; `ds_dmc_step_tmove`, the same with T-moves, once per step), `DmcState` holds
the six walker arrays (seven with a pseudopotential: 'epp') with the scalars a run carries between blocks (`save` / `load`: one .npz of numbers; a resumed run continues
bit-identically), `reblock` is the blocking error bar of a correlated series.  The driver loop is `inference.run_dmc`.
"""
import numpy as np
import torch

STATS = ('w', 'we', 'we2', 'accepted', 'p', 'clipped', 'nonfinite', 'w2', 'parents')        # columns of a stats row


def default_e_cut(n_elec, tau):
    """The energy cut-off of Zen, Sorella, Gillan, Michaelides and Alfe (Phys. Rev. B 93, 241118): 0.2 sqrt(N / tau)."""
    return 0.2 * float(np.sqrt(n_elec / tau))


class DmcState:
    """Walker state of a DMC run: `arrays` = dict of x, logabs, phase, drift, eloc, weight -- and epp (B, 3) float64 = (E_loc,
    Re E_nl, Im E_nl) in a run with a pseudopotential -- (device tensors, updated in place by every block) and the scalars e_trial, e_ref, tau_eff, offset (the Philox offset of the next step), valid (False until the
    first block has filled logabs .. eloc from x)."""

    def __init__(self, arrays, e_trial=0.0, e_ref=0.0, tau_eff=0.0, offset=0, valid=False, sum_w=0.0, sum_we=0.0):
        self.arrays, self.e_trial, self.e_ref, self.tau_eff, self.offset, self.valid = arrays, float(e_trial), float(e_ref), \
            float(tau_eff), int(offset), bool(valid)
        self.sum_w, self.sum_we = float(sum_w), float(sum_we)        # the running mixed estimate e_ref = sum_we / sum_w

    @classmethod
    def fresh(cls, system, x, tau, e_trial, e_ref=None, weight=None, ecp=False):
        return cls(system.dmc_state(x, weight, ecp=True) if ecp else system.dmc_state(x, weight), e_trial, e_trial if e_ref is None else e_ref, tau, 0, False)

    def save(self, path):
        """One .npz of numbers: the six arrays (and epp when the state has it), e_trial, e_ref (with the two sums behind it), tau_eff and the Philox offset."""
        np.savez(path, **{k: v.cpu().numpy() for k, v in self.arrays.items()}, e_trial=np.float64(self.e_trial),
                 e_ref=np.float64(self.e_ref), tau_eff=np.float64(self.tau_eff), offset=np.uint64(self.offset),
                 valid=np.int64(self.valid), sum_w=np.float64(self.sum_w), sum_we=np.float64(self.sum_we))

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path) as f:
            names = ('x', 'logabs', 'phase', 'drift', 'eloc', 'weight') + (('epp',) if 'epp' in f.files else ())
            arrays = {k: torch.as_tensor(f[k], device=device).contiguous() for k in names}
            return cls(arrays, float(f['e_trial']), float(f['e_ref']), float(f['tau_eff']), int(f['offset']), bool(int(f['valid'])),
                       float(f['sum_w']), float(f['sum_we']))


def make_dmc_step(logdet_net, simulation_cell, tau, steps, e_cut=None, node_mode=0, branch_every=1, seed=0, pseudopotential=None,
                  tmoves=False, want_parents=False):
    """-> block(params, state) -> stats (steps, 9) float64 device tensor: `steps` DMC steps on `state` (a `DmcState`) in place as ONE
    `ds_dmc_step` call, with the state's e_trial, e_ref and tau_eff; the state's Philox offset advances by `steps`.  `e_cut`
    defaults to `default_e_cut`; 0 switches the clip off.  `seed`: the Philox seed (fold the rank into it).
    `pseudopotential` (a `pseudopotential.SemiLocalECP`): the locality approximation, ONE `ds_dmc_step_ecp` call per block, which
    synchronises the stream once per step (and once for the initialisation); the state needs 'epp' (`DmcState.fresh(...,
    ecp=True)`), and the block's `ecp_stats` (steps, 3) = per step sum w E_loc, sum w Re E_nl, sum w Im E_nl stay on
    `block.ecp_stats`.  Any other form of potential is refused.
    `tmoves=True` (needs a `pseudopotential`): Casula's T-moves, ONE `ds_dmc_step_tmove` call per block;
    `block.ecp_stats` is then (steps, 4), the fourth column the number of walkers that made a T-move.
    `want_parents=True`: the call's parents (steps, B) int32 -- the identity for a step without a comb -- stay on `block.parents`
    (what `ForwardWalking.update` takes); with any of the three step entries."""
    from .pseudopotential import SemiLocalECP
    if pseudopotential is not None and not isinstance(pseudopotential, SemiLocalECP):
        raise NotImplementedError('DMC with this form of pseudopotential is not provided: only a pseudopotential.SemiLocalECP in the '
                                  'locality approximation is (no T-moves: DESIGN.md section 19)')
    if tmoves and pseudopotential is None:
        raise ValueError('tmoves=True needs a pseudopotential')
    system = logdet_net.apply.system
    tau = float(tau)
    e_cut = default_e_cut(system.n, tau) if e_cut is None else float(e_cut)
    del simulation_cell                                    # (the handle carries the cell; kept for the signature of the samplers)

    def block(params, state):
        out = system.dmc_step(params, state.arrays, steps, tau, tau_eff=state.tau_eff, e_trial=state.e_trial, e_ref=state.e_ref,
                              e_cut=e_cut, node_mode=node_mode, branch_every=branch_every, seed=seed, offset=state.offset,
                              state_valid=state.valid, **({} if pseudopotential is None else {'ecp': pseudopotential}),
                              **({'tmoves': True} if tmoves else {}), **({'want_parents': True} if want_parents else {}))
        state.valid = True
        state.offset += steps
        block.ecp_stats = out.get('ecp_stats')
        block.parents = out.get('parents') if want_parents else None
        return out['stats']
    block.ecp_stats = block.parents = None
    block.system, block.e_cut, block.steps, block.branch_every = system, e_cut, int(steps), int(branch_every)
    return block


def reblock(series, min_blocks=8):
    """Blocking error bar (Flyvbjerg and Petersen, J. Chem. Phys. 91, 461) of the mean of a correlated series, host numpy.
    -> (mean, error, block length): the series is halved by pair averages while at least `min_blocks` blocks remain; the error
    is the largest standard error of the mean over the levels (the plateau of the blocking curve, from below)."""
    x = np.asarray(series, dtype=np.float64).reshape(-1)
    if len(x) < 2:
        return (float(x.mean()) if len(x) else float('nan')), float('nan'), 1
    mean, best, length, size = float(x.mean()), 0.0, 1, 1
    while len(x) >= max(min_blocks, 2):
        err = float(np.sqrt(x.var(ddof=1) / len(x)))
        if err > best:
            best, length = err, size
        x = 0.5 * (x[0:2 * (len(x) // 2):2] + x[1:2 * (len(x) // 2):2])
        size *= 2
    return mean, best, length


# ------------------------------------------------------------------ forward walking (csrc/ds_fw.h)
BUILTIN_SCALARS = ('energy', 'potential', 'kinetic')


class ForwardWalking:
    """Pure (forward-walking) estimators of a DMC run on the device: density, g(r) and per-walker scalars at several lags at once.

    The estimate of O at lag l is  sum_w w_w(t + l) O(x_anc(w)(t)) / sum_w w_w(t + l): the snapshot taken l blocks ago, weighted
    with what its descendants weigh now.  `lags` are counted in blocks (projection time: lag * steps_per_block * tau_eff), distinct
    integers >= 0.  A ring of max(lags) + 1 slots holds, per slot, a copy of x (B, 3N), the per-walker scalar values (B, K)
    float64 and an int32 ancestor row.  Lag 0 is the properly weighted mixed estimate, valid on every block.  The variance grows
    with the lag and the bias falls with it: convergence in the lag is the user's to check, which is why several lags run at once.

    `density_grid`, `density_cell`, `pair_bins`, `pair_rmax`: as `estimator.RealSpaceAccumulator` (which checks them); both None:
    scalars only.  The counts are integers: a walker enters with q = rint(weight * weight_scale), so a weight is resolved to
    1 / weight_scale (the comb keeps weights near 1) and must stay below 2^24 / weight_scale.
    `scalars`: names of the built-in ones -- 'energy' = eloc (+ epp[:, 0] + epp[:, 1] when the state has 'epp'), 'potential' =
    the Ewald energy (+ the same epp part), 'kinetic' = energy - potential, all in Hartree per simulation cell -- or a dict
    name -> None (built-in) or a callable `arrays -> (B,)` or `(B, k)` float64 tensor for anything else per walker (a per-walker
    S(k) is not built in: it goes through such a callable)."""

    def __init__(self, simulation_cell, lags=(0, 4, 16), density_grid=None, density_cell='primitive', pair_bins=None, pair_rmax=None,
                 scalars=BUILTIN_SCALARS, weight_scale=2.0 ** 16):
        from .estimator import RealSpaceAccumulator
        lags = tuple(lags)
        if not lags or any(int(l) != l or l < 0 for l in lags):
            raise ValueError(f'ForwardWalking: lags must be integers >= 0, got {lags!r}')
        lags = tuple(int(l) for l in lags)
        if len(set(lags)) != len(lags):
            raise ValueError(f'ForwardWalking: lags must be distinct, got {lags!r}')
        if not (np.isfinite(weight_scale) and weight_scale > 0):
            raise ValueError(f'ForwardWalking: weight_scale must be positive and finite, got {weight_scale!r}')
        self.lags, self.n_slots, self.weight_scale = lags, max(lags) + 1, float(weight_scale)
        self.a = np.array(simulation_cell.a, dtype=np.float64).reshape(3, 3)
        self.nelec = (int(simulation_cell.nelec[0]), int(simulation_cell.nelec[1]))
        # (the real-space setup and its refusals are RealSpaceAccumulator's; it holds no counts here)
        if pair_rmax is not None and pair_bins is None:
            raise ValueError('pair_rmax without pair_bins')
        self.rs = None if density_grid is None and pair_bins is None else \
            RealSpaceAccumulator(simulation_cell, density_grid=density_grid, density_cell=density_cell, pair_bins=pair_bins,
                                 pair_rmax=pair_rmax)
        spec = dict(scalars) if isinstance(scalars, dict) else {str(n): None for n in scalars}
        for name, fn in spec.items():
            if fn is None and name not in BUILTIN_SCALARS:
                raise ValueError(f'ForwardWalking: {name!r} is no built-in scalar {BUILTIN_SCALARS}; give a callable for it')
            if fn is not None and not callable(fn):
                raise ValueError(f'ForwardWalking: the scalar {name!r} must be None (built-in) or a callable')
        self.spec = spec
        self.columns = None                   # name -> (first column, number of columns), known after the first update
        self.batch = self.n3 = None
        self.t = 0                            # blocks seen
        self.ring_x = self.ring_v = self.anc = self.dens = self.pair = self.q_sum = self.bad = None
        self.series = [[] for _ in lags]      # per lag: one (K, 2) row per block in which the lag's slot existed
        self.reduced = False

    # ---- accumulation
    def _values(self, system, arrays):
        cols, names = [], {}
        x = arrays['x']
        builtin = {}
        if any(fn is None for fn in self.spec.values()):
            epp = (arrays['epp'][:, 0] + arrays['epp'][:, 1]) if 'epp' in arrays else None
            energy = arrays['eloc'] if epp is None else arrays['eloc'] + epp
            ew = system.ewald(x)
            pot = (ew[:, 0] + ew[:, 1] + ew[:, 2]).double()
            pot = pot if epp is None else pot + epp
            builtin = dict(energy=energy, potential=pot, kinetic=energy - pot)
        k0 = 0
        for name, fn in self.spec.items():
            v = builtin[name] if fn is None else fn(arrays)
            if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.dim() in (1, 2) and v.shape[0] == x.shape[0]):
                raise ValueError(f'ForwardWalking: the scalar {name!r} must be a (B,) or (B, k) float64 tensor')
            v = v.reshape(x.shape[0], -1)
            names[name] = (k0, int(v.shape[1]))
            k0 += int(v.shape[1])
            cols.append(v)
        if self.columns is None:
            self.columns = names
        elif self.columns != names:
            raise ValueError('ForwardWalking: the scalars changed their number of columns between updates')
        return torch.cat(cols, dim=1).contiguous() if cols else None

    def _allocate(self, x):
        dev, L = x.device, len(self.lags)
        B, n3 = self.batch, self.n3
        i64 = dict(dtype=torch.int64, device=dev)
        if self.ring_x is None:
            K = sum(k for _, k in self.columns.values())
            self.ring_x = torch.zeros(self.n_slots, B, n3, dtype=x.dtype, device=dev)
            self.ring_v = torch.zeros(self.n_slots, B, K, dtype=torch.float64, device=dev)
            self.anc = torch.full((self.n_slots, B), -1, dtype=torch.int32, device=dev)
            self.q_sum, self.bad = torch.zeros(L, **i64), torch.zeros(L, 2, 2, **i64)
            if self.rs is not None and self.rs.grid is not None:
                self.dens = torch.zeros((L, 2) + self.rs.grid, **i64)
            if self.rs is not None and self.rs.n_r is not None:
                self.pair = torch.zeros(L, 3, self.rs.n_r, **i64)
        elif self.ring_x.device != dev:       # (after load_state_dict the tensors wait on the host)
            for k in ('ring_x', 'ring_v', 'anc', 'dens', 'pair', 'q_sum', 'bad'):
                if getattr(self, k) is not None:
                    setattr(self, k, getattr(self, k).to(dev).contiguous())
            self.series = [[r.to(dev) for r in rows] for rows in self.series]

    def update(self, system, state, parents):
        """After every block: `state` (a `DmcState` or its dict of arrays) as the block left it, `parents` (steps, B) int32 as
        the block's step entry wrote them (`make_dmc_step(..., want_parents=True)`: `block.parents`).  In this order: 1. the
        ancestor rows of all slots go through the block's parents (`ds_dmc_ancestry`); 2. the slot of this block takes x, the
        scalars and anc = the identity; 3. for every lag whose slot exists, `ds_realspace_counts_w` into that lag's own int64
        buffers and `ds_dmc_fw_sums`, both with the slot's data, index = the slot's ancestor row and weight = the state's
        weights as they stand now; 4. the (K, 2) row is appended to that lag's per-block series."""
        from . import device
        if self.reduced:
            raise RuntimeError('ForwardWalking.update after reduce(): the counts are already summed over the ranks')
        arrays = getattr(state, 'arrays', state)
        x, weight = arrays['x'], arrays['weight']
        if not x.is_cuda:
            raise RuntimeError('ForwardWalking.update: the walkers must live on the ROCm device (no CPU path)')
        if x.shape[1] != 3 * sum(self.nelec):
            raise ValueError(f'ForwardWalking.update: walkers have {x.shape[1]} coordinates, the cell has {sum(self.nelec)} electrons')
        if not np.array_equal(np.asarray(system.cell.a, dtype=np.float64).reshape(3, 3), self.a) or \
                tuple(int(n) for n in system.cell.nelec) != self.nelec:
            raise ValueError('ForwardWalking.update: the system belongs to another cell than the tracker')
        if self.batch is None:
            self.batch, self.n3 = int(x.shape[0]), int(x.shape[1])
        if (int(x.shape[0]), int(x.shape[1])) != (self.batch, self.n3):
            raise ValueError(f'ForwardWalking.update: the batch is {tuple(x.shape)}, the first update had ({self.batch}, {self.n3})')
        if parents is not None and tuple(parents.shape[1:]) != (self.batch,):
            raise ValueError(f'ForwardWalking.update: parents must be (steps, {self.batch}), got {tuple(parents.shape)}')
        values = self._values(system, arrays)
        self._allocate(x)
        device.dmc_ancestry(parents.contiguous() if parents is not None else None, self.anc, B=self.batch)
        slot = self.t % self.n_slots
        self.ring_x[slot].copy_(x)
        if values is not None:
            self.ring_v[slot].copy_(values)
        self.anc[slot].copy_(torch.arange(self.batch, dtype=torch.int32, device=x.device))
        for i, lag in enumerate(self.lags):
            if lag > self.t:
                continue
            s = (self.t - lag) % self.n_slots
            if self.dens is not None or self.pair is not None:
                device.realspace_counts_w(self.ring_x[s], self.nelec[0], self.q_sum[i:i + 1], self.bad[i, 0], index=self.anc[s],
                                          weight=weight, weight_scale=self.weight_scale,
                                          dens=None if self.dens is None else self.dens[i], fold_lattice=self.rs.fold,
                                          pair=None if self.pair is None else self.pair[i], latvec=self.a, r_max=self.rs.r_max)
            if values is not None:
                row, _ = device.dmc_fw_sums(self.ring_v[s], index=self.anc[s], weight=weight, n_bad=self.bad[i, 1])
                self.series[i].append(row)
        self.t += 1

    # ---- results (host)
    def _lag(self, lag):
        if lag not in self.lags:
            raise ValueError(f'ForwardWalking: lag {lag!r} is not one of {self.lags}')
        return self.lags.index(lag)

    def _np(self, t):
        return None if t is None else t.detach().cpu().numpy()

    def series_array(self, lag):
        """(blocks, K, 2) float64: per block in which the lag's slot existed, per column (sum w v, sum w)."""
        rows = self.series[self._lag(lag)]
        K = 0 if self.columns is None else sum(k for _, k in self.columns.values())
        return np.stack([self._np(r) for r in rows]) if rows else np.zeros((0, K, 2))

    def _realspace(self, lag):
        """A RealSpaceAccumulator of this setup with the lag's counts and n_walkers = q_sum: its normalisation applies as it is."""
        from .estimator import RealSpaceAccumulator
        if self.rs is None:
            raise ValueError('this tracker holds no real-space counts (density_grid = pair_bins = None)')
        i = self._lag(lag)
        acc = RealSpaceAccumulator.from_state_dict(self.rs.state_dict())
        acc.dens = None if self.dens is None else self.dens[i].cpu()
        acc.pair = None if self.pair is None else self.pair[i].cpu()
        acc.n_walkers = 0 if self.q_sum is None else int(self.q_sum[i])
        return acc

    def density_counts(self, lag):
        return self._realspace(lag).density_counts()

    def pair_counts(self, lag):
        return self._realspace(lag).pair_counts()

    def density(self, lag):
        """(2, g0, g1, g2) float64, electrons / Bohr^3, in the conventions of `RealSpaceAccumulator.density`, normalised by q_sum."""
        return self._realspace(lag).density()

    def pair_correlation(self, lag):
        """-> (r_mid, g (3, n_r)) in the conventions of `RealSpaceAccumulator.pair_correlation`, normalised by q_sum."""
        return self._realspace(lag).pair_correlation()

    def scalar(self, name, lag, skip=0):
        """-> (value, error, block length): the ratio of the summed columns sum_t sum w v / sum_t sum w over the blocks from `skip` on,
        and the reblocked error (`reblock`) of the per-block ratios (of fewer than 8 blocks: the standard error of their mean).  A
        scalar of k > 1 columns gives arrays of k entries.  For lag l the first row belongs to the snapshot of block 0, weighted at
        block l: `skip` counts snapshots."""
        if self.columns is None or name not in self.columns:
            raise ValueError(f'ForwardWalking: no scalar {name!r} (have {tuple(self.spec)})')
        k0, k = self.columns[name]
        ser = self.series_array(lag)[skip:, k0:k0 + k]
        with np.errstate(invalid='ignore', divide='ignore'):
            value = ser[:, :, 0].sum(0) / ser[:, :, 1].sum(0) if len(ser) else np.full(k, np.nan)
            per_block = ser[:, :, 0] / ser[:, :, 1]
        # (a series shorter than reblock's 8 blocks gets the plain standard error of its mean instead of no error at all)
        stats = [reblock(per_block[:, j], min_blocks=min(8, max(len(per_block), 2))) for j in range(k)]
        err, length = np.array([st[1] for st in stats]), np.array([st[2] for st in stats])
        return (float(value[0]), float(err[0]), int(length[0])) if k == 1 else (value, err, length)

    def lost(self, lag):
        """Contributions skipped because the ancestor row held no valid walker (a lost lineage): the sum over the blocks."""
        return 0 if self.bad is None else int(self.bad[self._lag(lag), :, 0].max())

    @property
    def n_bad(self):
        """(lags, 2, 2) int64: per lag, for the counts [0] and for the sums [1], the skips for the index and for the weight /
        value, as `ds_realspace_counts_w` and `ds_dmc_fw_sums` count them."""
        return np.zeros((len(self.lags), 2, 2), np.int64) if self.bad is None else self._np(self.bad)

    # ---- ranks, continuation, persistence
    def _same_setup(self, other):
        same = lambda p, q: (p is None) == (q is None) and (p is None or np.array_equal(np.asarray(p), np.asarray(q)))
        rs = (self.rs is None) == (other.rs is None) and (self.rs is None or self.rs._same_setup(other.rs))
        return rs and all(same(getattr(self, k), getattr(other, k)) for k in ('a', 'nelec', 'lags', 'weight_scale')) and \
            tuple(self.spec) == tuple(other.spec)

    def reduce(self):
        """Sum the counts, q_sum, the skip counters and the per-block series over the ranks (`constants.psum_if_pmap`; the
        identity at world size 1): one all-reduce of the int64 arrays and one of the series.  `weight_scale` must be equal on all
        ranks (it is checked).  Once per tracker: a second call raises, as does `update` afterwards."""
        from . import constants
        if self.reduced:
            raise RuntimeError('ForwardWalking.reduce was already called: reducing twice would count every rank again')
        if constants.world_size() > 1:
            if self.q_sum is None:
                raise RuntimeError('ForwardWalking.reduce before the first update')
            dev = self.q_sum.device
            scale = torch.tensor([self.weight_scale, -self.weight_scale], dtype=torch.float64, device=dev)
            lo = constants.psum_if_pmap(scale) / constants.world_size()
            if float(lo[0]) != self.weight_scale or float(lo[1]) != -self.weight_scale:
                raise ValueError('ForwardWalking.reduce: weight_scale differs between the ranks')
            names = [k for k in ('dens', 'pair', 'q_sum', 'bad') if getattr(self, k) is not None]
            packed = constants.psum_if_pmap(torch.cat([getattr(self, k).reshape(-1) for k in names]))
            off = 0
            for k in names:
                t = getattr(self, k)
                setattr(self, k, packed[off:off + t.numel()].reshape(t.shape).clone())
                off += t.numel()
            flat = [r for rows in self.series for r in rows]
            if flat:
                summed = constants.psum_if_pmap(torch.stack(flat))
                it = iter(summed.unbind(0))
                self.series = [[next(it) for _ in rows] for rows in self.series]
        self.reduced = True
        return self

    def merge(self, other):
        """Add the counts of another tracker of the same setup (another seed, another run) and append its series; the ring stays
        this tracker's.  Both rank-local or both reduced, as `RealSpaceAccumulator.merge`."""
        from . import constants
        if not self._same_setup(other):
            raise ValueError('ForwardWalking.merge: the two trackers differ in cell, lags, grid, bins, scalars or weight_scale')
        if self.reduced != other.reduced and constants.world_size() > 1:
            raise ValueError('ForwardWalking.merge: one side is summed over the ranks and the other is rank-local')
        if self.columns is None:
            self.columns = other.columns
        elif other.columns is not None and other.columns != self.columns:
            raise ValueError('ForwardWalking.merge: the scalars have different columns')
        for k in ('dens', 'pair', 'q_sum', 'bad'):
            mine, theirs = getattr(self, k), getattr(other, k)
            if theirs is not None:
                setattr(self, k, theirs.clone() if mine is None else mine + theirs.to(mine.device))
        for rows, more in zip(self.series, other.series):
            rows.extend(r.to(rows[0].device) if rows else r for r in more)
        return self

    def state_dict(self):
        """Plain numpy arrays: the setup, the ring (x, values, ancestor rows, the block counter), the buffers and the series."""
        sd = {'lags': np.asarray(self.lags, np.int64), 'weight_scale': np.float64(self.weight_scale), 'simulation_lattice': self.a.copy(),
              'nelec': np.asarray(self.nelec, np.int64), 'blocks': np.int64(self.t), 'reduced': np.bool_(self.reduced),
              'scalar_names': np.asarray(list(self.spec), dtype=str)}
        if self.rs is not None:
            for k, v in self.rs.state_dict().items():
                if k in ('fold_lattice', 'grid', 'r_edges', 'pair_rmax'):
                    sd['rs_' + k] = v
        if self.columns is not None:
            sd['columns'] = np.asarray([self.columns[n] for n in self.spec], np.int64).reshape(len(self.spec), 2)
        for k in ('ring_x', 'ring_v', 'anc', 'dens', 'pair', 'q_sum', 'bad'):
            if getattr(self, k) is not None:
                sd[k] = self._np(getattr(self, k))
        for i, lag in enumerate(self.lags):
            sd[f'series_{lag}'] = self.series_array(lag)
        return sd

    def load_state_dict(self, sd):
        """Replace ring, buffers and series by those of `sd` (written by a tracker of the same setup): the next `update` continues
        with the same bits as the run that was not interrupted.  The tracker is rank-local and open for `update` afterwards."""
        if tuple(int(l) for l in sd['lags']) != self.lags or float(sd['weight_scale']) != self.weight_scale or \
                not np.array_equal(sd['simulation_lattice'], self.a) or tuple(int(n) for n in sd['nelec']) != self.nelec or \
                tuple(str(n) for n in sd['scalar_names']) != tuple(self.spec):
            raise ValueError('ForwardWalking.load_state_dict: the state belongs to another cell, lags, scalars or weight_scale')
        has = lambda k: 'rs_' + k in sd
        if (self.rs is None) != (not (has('grid') or has('r_edges'))) or (self.rs is not None and (
                (self.rs.grid is None) != (not has('grid')) or (self.rs.n_r is None) != (not has('r_edges')) or
                (has('grid') and (tuple(int(v) for v in sd['rs_grid']) != self.rs.grid or not np.array_equal(sd['rs_fold_lattice'], self.rs.fold))) or
                (has('r_edges') and (len(sd['rs_r_edges']) - 1 != self.rs.n_r or float(sd['rs_pair_rmax']) != self.rs.r_max)))):
            raise ValueError('ForwardWalking.load_state_dict: the state belongs to another grid or other bins')
        self.columns = {n: (int(c[0]), int(c[1])) for n, c in zip(self.spec, sd['columns'])} if 'columns' in sd else None
        for k in ('ring_x', 'ring_v', 'anc', 'dens', 'pair', 'q_sum', 'bad'):
            setattr(self, k, torch.as_tensor(np.array(sd[k])).contiguous() if k in sd else None)
        self.batch, self.n3 = (int(self.ring_x.shape[1]), int(self.ring_x.shape[2])) if self.ring_x is not None else (None, None)
        self.t = int(sd['blocks'])
        self.series = [[torch.as_tensor(np.array(r)) for r in sd[f'series_{lag}']] for lag in self.lags]
        self.reduced = False
        return self

    def save(self, path):
        """One .npz of `state_dict()`."""
        with open(path, 'wb') as f:
            np.savez(f, **self.state_dict())

    def load(self, path):
        """`load_state_dict` of the file that `save` wrote; the tracker itself is made by the caller (callables are not stored)."""
        with np.load(path) as f:
            return self.load_state_dict({k: f[k] for k in f.files})
