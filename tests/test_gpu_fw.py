"""GPU tests of forward walking (csrc/ds_fw.h, `dmc.ForwardWalking`): `ds_dmc_ancestry`,
`ds_realspace_counts_w` and `ds_dmc_fw_sums` against the numpy model of tests/fw_helpers.py -- integers equal, sums equal bit for
bit -- the tracker end to end on the device's own snapshots, parents and weights, its reduction to `RealSpaceAccumulator`, and the
physics check that the pure total energy agrees with the mixed one."""
import functools
import types

import numpy as np
import pytest
import torch

import dmc_ecp_helpers as deh
import dmc_helpers as dh
import fw_helpers as fw
import realspace_helpers as rh
import sampler_helpers as sh
from deepsolid_amd import device, dmc, estimator
from test_gpu_dmc import bits, clone, cu, dev_params, same_bits, system

pytestmark = pytest.mark.gpu

I32 = dict(dtype=torch.int32, device='cuda')
I64 = dict(dtype=torch.int64, device='cuda')
EDGE_WEIGHTS = [0.0, 1.0, 2.0 ** -20, 255.9, 256.5, np.nan, np.inf, -1.0]       # 256.5 x 2^16 > 2^24: bad
SCALE = 2.0 ** 16


def ci(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64).astype(np.int32), device='cuda')


# ------------------------------------------------------------------------------------------------------------ 1. ds_dmc_ancestry
def parent_rows(kind, steps, B, rng):
    if kind == 'identity':
        return np.tile(np.arange(B), (steps, 1))
    if kind == 'zero':
        return np.zeros((steps, B), np.int64)
    rows = rng.integers(0, B, size=(steps, B))
    if kind == 'garbage' and steps:
        for k in range(steps):
            bad = rng.integers(0, B, size=max(1, B // 8))
            rows[k, bad] = rng.choice([-1, B, 2 ** 31 - 1, -2 ** 31, B + 7], size=len(bad))
        rows[steps - 1, 0] = -1
        rows[0, B - 1] = B
    return rows


@pytest.mark.parametrize('B', [1, 3, 257, 1025])
def test_ancestry_equals_the_model(B):
    """steps = 0, 1, 3; n_slots = 0, 1, 4; the identity, all walkers pointing to walker 0, a random map, rows with -1, B and the
    int32 extremes; tables that already hold -1; in place, run twice."""
    rng = np.random.default_rng(B)
    for steps in (0, 1, 3):
        for n_slots in (0, 1, 4):
            for kind in ('identity', 'zero', 'random', 'garbage'):
                rows = parent_rows(kind, steps, B, rng)
                anc = rng.integers(0, B, size=(n_slots, B))
                anc[:, rng.integers(0, B, size=max(1, B // 5))] = -1           # lineages that are lost already
                want_P = fw.compose(rows, B)
                want = fw.carry(anc, want_P)
                parents = ci(rows) if steps else None
                anc_d = ci(anc) if n_slots else None
                P = device.dmc_ancestry(parents, anc_d, want_block=True, B=B)
                assert np.array_equal(P.cpu().numpy(), want_P), (steps, n_slots, kind)
                if kind == 'identity':
                    assert np.array_equal(want_P, np.arange(B))
                if kind == 'garbage' and steps:
                    assert (want_P < 0).any()
                if n_slots:
                    assert np.array_equal(anc_d.cpu().numpy(), want), (steps, n_slots, kind)
                    assert device.dmc_ancestry(parents, anc_d, B=B) is None    # a second time, on its own output
                    assert np.array_equal(anc_d.cpu().numpy(), fw.carry(want, want_P)), (steps, n_slots, kind)


def test_ancestry_refuses_a_short_workspace_and_bad_arguments():
    from deepsolid_amd import _lib
    from deepsolid_amd.device import _ptr, _stream
    lib = _lib.load()
    B, steps, n_slots = 300, 2, 3
    parents, anc = ci(np.tile(np.arange(B), (steps, 1))), ci(np.tile(np.arange(B), (n_slots, 1)))
    before = anc.clone()
    need = lib.ds_dmc_ancestry_workspace_bytes(B, n_slots)
    assert need == 4 * B * (1 + n_slots)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    call = lambda *a: (lib.ds_dmc_ancestry(*a, _stream()), lib.ds_last_error().decode())
    rc, msg = call(B, steps, _ptr(parents), n_slots, _ptr(anc), None, _ptr(ws), need - 1)
    assert rc != 0 and 'workspace too small' in msg
    for args, word in (((0, steps, _ptr(parents), n_slots, _ptr(anc), None, _ptr(ws), need), 'B must be'),
                       ((B, -1, _ptr(parents), n_slots, _ptr(anc), None, _ptr(ws), need), 'steps'),
                       ((B, steps, None, n_slots, _ptr(anc), None, _ptr(ws), need), 'null parents'),
                       ((B, steps, _ptr(parents), n_slots, None, None, _ptr(ws), need), 'null anc'),
                       ((B, steps, _ptr(parents), n_slots, _ptr(anc), None, None, need), 'null workspace')):
        rc, msg = call(*args)
        assert rc != 0 and word in msg, (word, msg)
    torch.cuda.synchronize()
    assert torch.equal(anc, before)                                            # refused before any launch
    assert call(B, steps, _ptr(parents), n_slots, _ptr(anc), None, _ptr(ws), need)[0] == 0


# ------------------------------------------------------------------------------------------------------ 2. ds_realspace_counts_w
GRID, N_R = (2, 3, 5), 64


def counts_w(x, n_up, cell, r_max, index=None, weight=None, scale=SCALE, dens=True, pair=True, fold=None):
    d = torch.zeros((2,) + GRID, **I64) if dens is True else dens
    p = torch.zeros(3, N_R, **I64) if pair is True else pair
    q_sum, n_bad = torch.zeros(1, **I64), torch.zeros(2, **I64)
    device.realspace_counts_w(x, n_up, q_sum, n_bad, index=index, weight=weight, weight_scale=scale, dens=d,
                              fold_lattice=cell.a if fold is None else fold, pair=p, latvec=cell.a, r_max=r_max)
    return d, p, int(q_sum), n_bad.cpu().numpy().tolist()


@pytest.mark.parametrize('name', ['lih', 'triclinic'])
def test_counts_w_without_index_and_weight_equal_the_unweighted_counts(name):
    cell, x = rh.case(name)
    r_ws = estimator.wigner_seitz_radius(cell.a)
    xd = torch.as_tensor(x, device='cuda')
    fold = cell.original_cell.a
    d0, p0 = torch.zeros((2,) + GRID, **I64), torch.zeros(3, N_R, **I64)
    device.realspace_counts(xd, cell.nelec[0], dens=d0, fold_lattice=fold, pair=p0, latvec=cell.a, r_max=r_ws)
    d, p, q_sum, n_bad = counts_w(xd, cell.nelec[0], cell, r_ws, fold=fold)
    assert torch.equal(d, d0) and torch.equal(p, p0) and q_sum == len(x) and n_bad == [0, 0]
    assert int(p0.sum()) > 0 and int(d0.sum()) == len(x) * sum(cell.nelec)


@pytest.mark.parametrize('batch,nelec', [(1, (1, 1)), (1025, (3, 2)), (3, (64, 64)), (3, (1, 0))])
def test_counts_w_edge_cases_equal_the_model(batch, nelec):
    """The inputs of test_gpu_realspace.test_shapes.  B != B_src, an index with repeats, -1, B_src and the int32 extremes; the
    weights 0, 1, 2^-20, 255.9, 256.5 (bad), NaN, inf, -1 and a few ordinary ones; q_sum and both n_bad entries; conservation;
    either buffer NULL; the buffers are added to."""
    cell = rh.cubic_cell(*nelec)
    n = sum(nelec)
    x = rh.push_out(rh.uniform_walkers(cell.a, n, batch, 600 + n + batch), cell.a, 600 + n + batch)
    r_ws = estimator.wigner_seitz_radius(cell.a)
    xd = torch.as_tensor(x, device='cuda')
    rng = np.random.default_rng(batch + n)
    B = batch + 37 if batch > 1 else 9
    index = rng.integers(0, batch, size=B)
    index[rng.choice(B, size=4, replace=False)] = [-1, batch, 2 ** 31 - 1, -2 ** 31]
    pool = np.array(EDGE_WEIGHTS + [0.37, 1.25, 1.9])
    weight = pool[np.arange(B) % len(pool)]
    rng.shuffle(weight)
    kw = dict(fold=cell.a, grid=GRID, a=cell.a, n_r=N_R, r_max=r_ws)
    w_plain = np.roll(pool, 3)[np.arange(batch) % len(pool)]               # (starts with an ordinary weight: B = 1 contributes)
    for idx, w in ((index, weight), (index, None), (None, w_plain)):
        ref = fw.counts_w(x, nelec[0], idx, w, SCALE, **kw)
        assert ref['margin'] >= rh.MARGIN
        d, p, q_sum, n_bad = counts_w(xd, nelec[0], cell, r_ws, None if idx is None else ci(idx), None if w is None else cu(w))
        np.testing.assert_array_equal(d.cpu().numpy(), ref['dens'])
        np.testing.assert_array_equal(p.cpu().numpy(), ref['pair'])
        assert q_sum == ref['q_sum'] and n_bad == ref['n_bad'], (q_sum, n_bad, ref['q_sum'], ref['n_bad'])
        assert q_sum > 0 and (idx is None or n_bad[0] == 4) and (idx is None or w is None or n_bad[1] >= 1)
        assert int(d[0].sum()) == nelec[0] * q_sum and int(d[1].sum()) == nelec[1] * q_sum           # conservation
        # either buffer NULL, into buffers that hold something already
        pat_d = torch.arange(2 * 30, **I64).reshape((2,) + GRID) * 7
        pat_p = torch.arange(3 * N_R, **I64).reshape(3, N_R) * 1000
        d1, _, q1, b1 = counts_w(xd, nelec[0], cell, r_ws, None if idx is None else ci(idx), None if w is None else cu(w),
                                 dens=pat_d.clone(), pair=None)
        _, p1, q2, b2 = counts_w(xd, nelec[0], cell, r_ws, None if idx is None else ci(idx), None if w is None else cu(w),
                                 dens=None, pair=pat_p.clone())
        assert torch.equal(d1 - pat_d, d) and torch.equal(p1 - pat_p, p) and q1 == q2 == q_sum and b1 == b2 == n_bad
    with pytest.raises(RuntimeError, match='weight_scale'):
        counts_w(xd, nelec[0], cell, r_ws, weight=cu(np.ones(batch)), scale=0.0)
    with pytest.raises(RuntimeError, match='B_src'):
        counts_w(xd, nelec[0], cell, r_ws, weight=cu(np.ones(batch + 1)))      # no index: B walkers need B rows


# ------------------------------------------------------------------------------------------------------------- 3. ds_dmc_fw_sums
def same_f64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize('B', [1, 255, 256, 257, 1025])
@pytest.mark.parametrize('K', [1, 3])
def test_fw_sums_equal_the_tree_bit_for_bit(B, K):
    rng = np.random.default_rng(10 * B + K)
    B_src = B + 3
    values = rng.normal(size=(B_src, K)) * 10.0 ** rng.integers(-3, 4, size=(B_src, 1))
    index = rng.integers(0, B_src, size=B)
    weight = rng.lognormal(0.0, 1.0, size=B)
    if B >= 255:
        index[rng.choice(B, size=4, replace=False)] = [-1, B_src, 2 ** 31 - 1, -2 ** 31]
        weight[rng.choice(B, size=len(EDGE_WEIGHTS), replace=False)] = EDGE_WEIGHTS
        values[index[(index >= 0) & (index < B_src)][5], K - 1] = np.nan        # one column only
        values[index[(index >= 0) & (index < B_src)][9], 0] = np.inf
    vd = cu(values)
    for idx, w in ((index, weight), (index, None), (None, weight), (None, None)):
        want, want_bad = fw.fw_sums(values, idx, w, B=B)
        out, n_bad = device.dmc_fw_sums(vd, None if idx is None else ci(idx), None if w is None else cu(w))
        if idx is None and w is None:                      # (the wrapper then takes B = B_src: the model too)
            want, want_bad = fw.fw_sums(values, None, None)
        assert same_f64(out.cpu().numpy(), want), (out.cpu().numpy(), want)
        assert n_bad.cpu().numpy().tolist() == want_bad
    if B >= 255:
        assert fw.fw_sums(values, index, weight)[1][0] == 4 and fw.fw_sums(values, index, weight)[1][1] >= 2
    n_bad = torch.tensor([5, 6], **I64)
    device.dmc_fw_sums(vd, ci(np.full(B, -1)), None, n_bad=n_bad)               # n_bad is added to; no walker contributes
    assert n_bad.cpu().numpy().tolist() == [5 + B, 6]
    with pytest.raises(RuntimeError, match='K must be'):
        device.dmc_fw_sums(torch.zeros(4, 65, dtype=torch.float64, device='cuda'))


# ------------------------------------------------------------------------------------------------------- 4. the tracker end to end
@functools.lru_cache(maxsize=None)
def setup(name):
    """-> (cell, DeviceSystem, device parameters, a stand-in for the log-det network that `make_dmc_step` reads the system from)."""
    sysd, dp = system(name)
    cell = sh.case(name)[1]
    return cell, sysd, dp, types.SimpleNamespace(apply=types.SimpleNamespace(system=sysd))


def make_tracker(cell, lags, **kw):
    return dmc.ForwardWalking(cell, lags=lags, density_grid=GRID, pair_bins=8, **kw)


def model_of(tracker, cell):
    return fw.Tracker(tracker.lags, cell.nelec[0], tracker.weight_scale, fold=tracker.rs.fold, grid=GRID, a=cell.a, n_r=8,
                      r_max=tracker.rs.r_max)


def run_blocks(name, B, blocks, tau, steps, branch_every, lags, seed=3, weights='ramp', tracker=None, state=None, model=None, **step_kw):
    """`blocks` blocks through `make_dmc_step(..., want_parents=True)` with `ForwardWalking.update` and the model's update after each;
    the model gets the device's own snapshot, values, parents and weights.  -> (tracker, model, state, list of parents)."""
    cell, sysd, dp, net = setup(name)
    if state is None:
        x0 = cu(dh.start_walkers(name, B, seed))
        ke, ew, _, _ = sysd.local_energy(dp, x0)
        e0 = float(np.round(float((ke[:, 0] + ew).mean()), 3))
        state = dmc.DmcState.fresh(sysd, x0, tau, e0, weight=cu(dh.preset_weights(weights, B)), ecp='pseudopotential' in step_kw)
    block = dmc.make_dmc_step(net, cell, tau, steps, branch_every=branch_every, seed=seed, want_parents=True, **step_kw)
    tracker = make_tracker(cell, lags) if tracker is None else tracker
    model = model_of(tracker, cell) if model is None else model
    all_parents = []
    for _ in range(blocks):
        block(dp, state)
        assert tuple(block.parents.shape) == (steps, B) and block.parents.dtype == torch.int32
        tracker.update(sysd, state, block.parents)
        slot = (tracker.t - 1) % tracker.n_slots
        assert torch.equal(tracker.ring_x[slot], state.arrays['x'])
        model.update(state.arrays['x'].cpu().numpy(), tracker.ring_v[slot].cpu().numpy(), block.parents.cpu().numpy(),
                     state.arrays['weight'].cpu().numpy())
        all_parents.append(block.parents.cpu().numpy())
    return tracker, model, state, all_parents


def assert_tracker_equals_model(tracker, model):
    assert model.margin >= rh.MARGIN
    for i, lag in enumerate(tracker.lags):
        np.testing.assert_array_equal(tracker.density_counts(lag), model.dens[i])
        np.testing.assert_array_equal(tracker.pair_counts(lag), model.pair[i])
        assert int(tracker.q_sum[i]) == int(model.q_sum[i])
        ser = tracker.series_array(lag)
        assert len(ser) == len(model.series[i]) == max(tracker.t - lag, 0)
        assert same_f64(ser, np.stack(model.series[i])), lag
        assert np.array_equal(tracker.anc[(tracker.t - 1 - lag) % tracker.n_slots].cpu().numpy(), model.anc_rows[lag][-1])
    np.testing.assert_array_equal(tracker.n_bad, model.bad)


def tracker_bits(t):
    sd = t.state_dict()
    return {k: (np.asarray(v).dtype.str, np.asarray(v).shape, np.asarray(v).tobytes()) for k, v in sd.items()}


@pytest.mark.parametrize('branch_every', [1, 2])
def test_tracker_equals_the_model_and_resumes_with_the_same_bits(branch_every, tmp_path):
    """h2, the fixture's parameters, B = 64, uneven start weights, 6 blocks of 2 steps, lags (0, 1, 3): every lag's counts and series
    equal the model's; 3 + 3 blocks through save / load give the bits of 6."""
    name, B, tau, lags = 'h2', 64, 0.1, (0, 1, 3)
    cell, sysd, dp, _ = setup(name)
    tracker, model, state, parents = run_blocks(name, B, 6, tau, 2, branch_every, lags)
    assert_tracker_equals_model(tracker, model)
    # the conditions without which the comparison would compare nothing
    counts = [np.bincount(row, minlength=B) for blk in parents for row in blk]
    assert any((c > 1).any() for c in counts) and any((c == 0).any() for c in counts)            # a walker duplicated, one killed
    assert any(not np.array_equal(row, np.arange(B)) for row in model.anc_rows[3])               # a lag-3 row that is not the identity
    assert tracker.lost(3) == 0 and int(tracker.q_sum.min()) > 0
    # built-in scalars: energy is eloc, kinetic + potential = energy to one rounding
    v = tracker.ring_v[(tracker.t - 1) % tracker.n_slots]
    assert torch.equal(bits(v[:, 0].contiguous()), bits(state.arrays['eloc']))
    assert bool((((v[:, 1] + v[:, 2]) - v[:, 0]).abs() <= 4 * np.finfo(np.float64).eps * (v[:, 1].abs() + v[:, 2].abs())).all())
    ew = sysd.ewald(state.arrays['x'])
    assert torch.equal(v[:, 1], (ew[:, 0] + ew[:, 1] + ew[:, 2]).double())
    # results are normalised by q_sum, in the accumulator's conventions
    acc = estimator.RealSpaceAccumulator(cell, density_grid=GRID, pair_bins=8)
    dv = abs(np.linalg.det(acc.fold)) / np.prod(GRID)
    per_fold = abs(np.linalg.det(cell.a)) / abs(np.linalg.det(acc.fold))
    np.testing.assert_allclose(tracker.density(3), model.dens[2] / (float(model.q_sum[2]) * dv * per_fold), rtol=1e-14)
    assert np.isclose(tracker.density(0).sum() * dv, sum(cell.nelec) / per_fold, rtol=1e-12)
    e, err, length = tracker.scalar('energy', 1)
    ser = np.stack(model.series[1])
    assert e == ser[:, 0, 0].sum() / ser[:, 0, 1].sum() and np.isfinite(err) and length >= 1
    # 3 + 3 blocks through save / load
    first, _, st, _ = run_blocks(name, B, 3, tau, 2, branch_every, lags)
    first.save(tmp_path / 'fw.npz')
    st.save(tmp_path / 'state.npz')
    resumed = make_tracker(cell, lags).load(tmp_path / 'fw.npz')
    second, _, st2, _ = run_blocks(name, B, 3, tau, 2, branch_every, lags, tracker=resumed, state=dmc.DmcState.load(tmp_path / 'state.npz'),
                                   model=model_of(resumed, cell))
    assert same_bits(state.arrays, st2.arrays) == []
    a, b = tracker_bits(tracker), tracker_bits(second)
    assert sorted(a) == sorted(b) and [k for k in a if a[k] != b[k]] == []
    # another batch or another cell than the first update's is refused
    with pytest.raises(ValueError, match='first update'):
        tracker.update(sysd, {k: v[:32].contiguous() for k, v in state.arrays.items()}, None)
    with pytest.raises(ValueError, match='another cell'):
        tracker.update(system('lih')[0], state, None)
    with pytest.raises(ValueError, match='parents must be'):
        tracker.update(sysd, state, torch.zeros(2, 32, **I32))


@pytest.mark.parametrize('tmoves', [False, True])
def test_tracker_with_a_pseudopotential(tmoves):
    """The same replay with `ecp=` and with `tmoves=True`, 3 blocks each, on lih with the synthetic potential of dmc_ecp_helpers: the
    parents of those entries feed the tables, energy carries the epp part."""
    name, B = deh.NAME, 12
    ecp = deh.potential(name)
    kw = dict(pseudopotential=ecp, **({'tmoves': True} if tmoves else {}))
    tracker, model, state, parents = run_blocks(name, B, 3, 0.1, 2, 1, (0, 1), seed=1, **kw)
    assert_tracker_equals_model(tracker, model)
    assert any(not np.array_equal(row, np.arange(B)) for blk in parents for row in blk)
    v, a = tracker.ring_v[(tracker.t - 1) % tracker.n_slots], state.arrays
    assert torch.equal(v[:, 0], a['eloc'] + (a['epp'][:, 0] + a['epp'][:, 1]))
    assert float((a['epp'][:, 0] + a['epp'][:, 1]).abs().max()) > 0


def test_branch_parents_give_the_tables_of_the_fused_call():
    """Two steps with the comb after each, fused in one call, against the same steps taken one by one with `ds_dmc_branch` after
    each: the parents, and the ancestor tables they carry, are the same."""
    name, B, tau, seed, o = 'h2', 64, 0.1, 3, 11
    cell, sysd, dp, _ = setup(name)
    x0, w0 = cu(dh.start_walkers(name, B, seed)), cu(dh.preset_weights('ramp', B))
    ke, ew, _, _ = sysd.local_energy(dp, x0)
    e0 = float(np.round(float((ke[:, 0] + ew).mean()), 3))
    kw = dict(e_trial=e0, e_ref=e0, e_cut=0.0, seed=seed)
    fused = sysd.dmc_state(x0, w0)
    out = sysd.dmc_step(dp, fused, 2, tau, offset=o, branch_every=1, state_valid=False, want_parents=True, **kw)
    anc0 = np.stack([np.arange(B), np.arange(B)[::-1], np.where(np.arange(B) % 4 == 0, -1, np.arange(B))])
    anc_f = ci(anc0)
    device.dmc_ancestry(out['parents'], anc_f)
    single, anc_s = sysd.dmc_state(x0, w0), ci(anc0)
    _, _, xi = sysd.dmc_noise(B, 2, seed=seed, offset=o)
    rows = []
    for i in range(2):
        sysd.dmc_step(dp, single, 1, tau, offset=o + i, branch_every=0, state_valid=i > 0, **kw)
        par = sysd.dmc_branch(single, float(xi[i]))
        rows.append(par)
        device.dmc_ancestry(par.reshape(1, B), anc_s)
    assert torch.equal(torch.stack(rows), out['parents']) and same_bits(fused, single) == []
    assert torch.equal(anc_f, anc_s) and not torch.equal(anc_f, ci(anc0))
    assert np.array_equal(anc_f.cpu().numpy(), fw.carry(anc0, fw.compose(out['parents'].cpu().numpy(), B)))


# ------------------------------------------------------------------------------------------------- 5. reduction to what exists
def test_unit_weights_on_combed_blocks_reduce_to_the_accumulator():
    """weight_scale such that q = 1, blocks that end on a comb, lags = (0,): the density and pair buffers equal those of a
    `RealSpaceAccumulator` fed the same x."""
    name, B = 'h2', 64
    cell, sysd, dp, net = setup(name)
    tracker = make_tracker(cell, (0,), weight_scale=1.0)
    acc = estimator.RealSpaceAccumulator(cell, density_grid=GRID, pair_bins=8)
    x0 = cu(dh.start_walkers(name, B, 3))
    ke, ew, _, _ = sysd.local_energy(dp, x0)
    state = dmc.DmcState.fresh(sysd, x0, 0.01, float((ke[:, 0] + ew).mean()))
    block = dmc.make_dmc_step(net, cell, 0.01, 2, branch_every=2, seed=3, want_parents=True)
    for _ in range(4):
        block(dp, state)
        w = state.arrays['weight']
        assert float(w.min()) == float(w.max()) and 0.5 < float(w[0]) < 1.5    # combed, and q = rint(w) = 1
        tracker.update(sysd, state, block.parents)
        acc.update(state.arrays['x'])
    np.testing.assert_array_equal(tracker.density_counts(0), acc.density_counts())
    np.testing.assert_array_equal(tracker.pair_counts(0), acc.pair_counts())
    assert int(tracker.q_sum[0]) == acc.n_walkers == 4 * B
    np.testing.assert_array_equal(tracker.density(0), acc.density())
    np.testing.assert_array_equal(tracker.pair_correlation(0)[1], acc.pair_correlation()[1])


# ---------------------------------------------------------------------------------------------------------------- 6. physics
def test_pure_total_energy_agrees_with_the_mixed_energy(tmp_path):
    """The h2 run of test_gpu_dmc.test_run_dmc_energy_is_not_above_the_vmc_energy through `inference.run_dmc(...,
    forward_walking=...)`: B = 512, tau = 0.01, 32 blocks of 10 steps, the first 8 snapshots left out, lags (0, 4, 8).  H commutes
    with itself, so the pure total energy must agree with the mixed one: |E_pure(l) - E_mixed| <= 5 sqrt(s_pure^2 + s_mixed^2) with
    reblocked errors, for l = 4 and 8 (the two are positively correlated, so the bound is conservative).  And kinetic + potential =
    energy to rounding.
    Measured on an MI355X (EXPERIMENTS.md): (E_pure - E_mixed) / sigma = -3.10 at lag 4 and -3.85 at lag 8, inside the bound.  The
    deviations are systematic, not noise: the pure estimate of the FUNCTION E_L is E0 - <d|H - E0|d> for psi_T = Phi0 + d, second
    order in the error of psi_T, and this fixture's parameters are untrained (E_VMC - E_mixed = +0.090 Ha)."""
    from deepsolid_amd import inference, init_guess, network
    _, cell, klist, net_kw, params = sh.case('h2')
    dp = dev_params(params)
    slog, ld = (network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name=m, **net_kw) for m in ('eval_slogdet', 'eval_logdet'))
    x0 = torch.as_tensor(init_guess.init_electrons(5, cell, cell.a, cell.nelec, 512, init_width=0.8), device='cuda')
    kw = dict(key=7, move_width=0.3, mcmc_steps=10, burn_in=20, vmc_iterations=64)
    tracker = dmc.ForwardWalking(cell, lags=(0, 4, 8), density_grid=8, pair_bins=16)
    state, rows, info = inference.run_dmc(slog, ld, dp, x0, cell, blocks=32, steps_per_block=10, tau=0.01, save_path=str(tmp_path),
                                          forward_walking=tracker, **kw)
    assert tracker.reduced and tracker.t == 32 and (tmp_path / 'forward_walking.npz').exists()
    warm = 8
    e_mixed, s_mixed, _ = tracker.scalar('energy', 0, skip=warm)
    eps = np.finfo(np.float64).eps
    scale = float(getattr(cell, 'scale', 1))
    print(f"h2: E_VMC {info['vmc_energy'] * scale:.6f} +- {info['vmc_error'] * scale:.6f} per simulation cell")
    for lag in (0, 4, 8):
        e, s, _ = tracker.scalar('energy', lag, skip=warm)
        k, v = tracker.scalar('kinetic', lag, skip=warm)[0], tracker.scalar('potential', lag, skip=warm)[0]
        n_terms = 512 * (32 - warm - lag)
        print(f'h2 lag {lag}: E {e:.6f} +- {s:.6f}  T {k:.6f}  V {v:.6f}  (E - E_mixed) / sigma '
              f'{(e - e_mixed) / np.hypot(s, s_mixed):+.3f}  max density difference to lag 0 '
              f'{np.abs(tracker.density(lag) - tracker.density(0)).max():.3e}')
        assert len(tracker.series_array(lag)) == 32 - lag
        assert abs((k + v) - e) <= n_terms * eps * (abs(k) + abs(v) + abs(e))
        if lag:
            assert abs(e - e_mixed) <= 5.0 * np.hypot(s, s_mixed), (lag, e, s, e_mixed, s_mixed)
    assert all(tracker.lost(lag) == 0 for lag in (0, 4, 8)) and not tracker.n_bad.any()
    # the weighted mixed estimate of the tracker and the driver's own block energies describe the same run
    e_rows = dmc.reblock([r['energy'] for r in rows[warm:]])[0]
    assert abs(e_mixed / scale - e_rows) <= 5.0 * np.hypot(info['error'], s_mixed / scale)
    # a resumed run continues the tracker with the same bits: 16 + 16 blocks
    first = dmc.ForwardWalking(cell, lags=(0, 4, 8), density_grid=8, pair_bins=16)
    inference.run_dmc(slog, ld, dp, x0, cell, blocks=16, steps_per_block=10, tau=0.01, save_path=str(tmp_path / 'a'), forward_walking=first, **kw)
    second = dmc.ForwardWalking(cell, lags=(0, 4, 8), density_grid=8, pair_bins=16).load(tmp_path / 'a' / 'forward_walking.npz')
    inference.run_dmc(slog, ld, dp, x0, cell, blocks=16, steps_per_block=10, tau=0.01, state=dmc.DmcState.load(tmp_path / 'a' / 'dmc_state.npz'),
                      forward_walking=second, **kw)
    a, b = tracker_bits(tracker), tracker_bits(second)
    assert [k for k in a if a[k] != b[k]] == []
