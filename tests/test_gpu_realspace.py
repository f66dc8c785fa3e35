"""GPU checks of the real-space counts (`ds_realspace_counts`, csrc/ds_realspace.h, through `device.realspace_counts` and
`estimator.RealSpaceAccumulator`) against the numpy oracle of tests/realspace_helpers.py.

The counts must EQUAL the oracle's integers.  The kernel and numpy round differently (FMA, order of the dot products: about
1e-13 in t = f g or t = r n_r / r_max at most), so a sample closer than 1e-9 to a bin edge could fall in either bin: every
exact test first asserts that the oracle's edge margin of its input is >= 1e-9 (tests/realspace_helpers.py)."""
import functools

import numpy as np
import pytest
import torch

import realspace_helpers as rh
from deepsolid_amd import device, estimator

pytestmark = pytest.mark.gpu

GRIDS = (('simulation', (16, 16, 16)), ('primitive', (2, 3, 5)), ('primitive', (48, 48, 48)), ('primitive', (1, 1, 1)))
BINS = (1, 7, 64, 1024)


def counts(x, n_up, fold=None, grid=None, a=None, n_r=None, r_max=None, dens=None, pair=None):
    """One call into fresh (or the given) buffers -> (dens, pair) device tensors."""
    if grid is not None and dens is None:
        dens = torch.zeros((2,) + tuple(grid), dtype=torch.int64, device='cuda')
    if n_r is not None and pair is None:
        pair = torch.zeros((3, n_r), dtype=torch.int64, device='cuda')
    device.realspace_counts(x, n_up, dens=dens, fold_lattice=fold, pair=pair, latvec=a, r_max=r_max)
    return dens, pair


@functools.lru_cache(maxsize=None)
def reference(name):
    """The shared oracle results of one cell: {(fold name, grid): counts}, {n_r: counts}, r_ws; margins asserted here."""
    cell, x = rh.case(name)
    r_ws = estimator.wigner_seitz_radius(cell.a)
    assert r_ws < 1.5 * estimator.plane_spacings(cell.a).min()
    assert x.min() < 0                                    # pushed out of the cell, some coordinates negative
    dens = {}
    for fold, grid in GRIDS:
        lat = cell.a if fold == 'simulation' else cell.original_cell.a
        dens[fold, grid], margin = rh.density_oracle(x, cell.nelec[0], lat, grid)
        assert margin >= rh.MARGIN, (name, fold, grid, margin)
    dist, chan = rh.pair_images(x, cell.nelec[0], cell.a, 2.0 * r_ws)
    pair = {}
    for n_r in BINS:
        pair[n_r], margin = rh.bin_pairs(dist, chan, n_r, r_ws)
        assert margin >= rh.MARGIN, (name, n_r, margin)
    return dens, pair, r_ws


@pytest.mark.parametrize('name', ['bcc_li', 'graphene', 'lih', 'diamond', 'triclinic'])
def test_cells_equal_the_oracle(name):
    """Every walker pushed out of its cell by lattice vectors: bcc (not orthorhombic), hexagonal with a 20-Bohr axis, fcc, 96
    electrons, and a skewed triclinic cell; unequal grids (index order), 1^3, 16^3, 48^3; n_r = 1, 7, 64, 1024 at r_max = r_ws."""
    cell, x = rh.case(name)
    ref_dens, ref_pair, r_ws = reference(name)
    xd = torch.as_tensor(x, device='cuda')
    B, (n_up, n_dn) = x.shape[0], cell.nelec
    for (fold, grid), n_r in zip(GRIDS, BINS):
        lat = cell.a if fold == 'simulation' else cell.original_cell.a
        dens, pair = counts(xd, n_up, lat, grid, cell.a, n_r, r_ws)
        dens, pair = dens.cpu().numpy(), pair.cpu().numpy()
        np.testing.assert_array_equal(dens, ref_dens[fold, grid])
        np.testing.assert_array_equal(pair, ref_pair[n_r])
        # conservation: every electron is in exactly one bin, every pair inside r_max in exactly one
        assert dens[0].sum() == B * n_up and dens[1].sum() == B * n_dn
        assert pair.sum(axis=1).tolist() == ref_pair[1][:, 0].tolist()


SHAPES = [(1, (1, 1)), (3, (1, 1)), (1025, (3, 2)), (3, (1, 0)), (3, (0, 1)), (7, (0, 6)), (7, (6, 0)), (3, (33, 32)), (3, (64, 64)),
          (2, (100, 28))]


@pytest.mark.parametrize('batch,nelec', SHAPES)
def test_shapes(batch, nelec):
    """B = 1, 3 and 1025 (one more walker than workgroups); N = 2, N = 1 (no pairs), one-spin cells, N = 65 and 128 (pair indices
    beyond one pass of the 256 lanes, electrons beyond one wave) in a cubic cell."""
    cell = rh.cubic_cell(*nelec)
    n = sum(nelec)
    x = rh.push_out(rh.uniform_walkers(cell.a, n, batch, 600 + n + batch), cell.a, 600 + n + batch)
    r_ws = estimator.wigner_seitz_radius(cell.a)
    ref_d, m_d = rh.density_oracle(x, nelec[0], cell.a, (2, 3, 5))
    ref_p, m_p = rh.pair_oracle(x, nelec[0], cell.a, 64, r_ws)
    assert m_d >= rh.MARGIN and m_p >= rh.MARGIN
    assert n == 1 or ref_p.sum() > 0                      # the input has pairs inside r_max
    pattern = torch.arange(3 * 64, dtype=torch.int64, device='cuda').reshape(3, 64) * 1000
    dens, pair = counts(torch.as_tensor(x, device='cuda'), nelec[0], cell.a, (2, 3, 5), cell.a, 64, r_ws, pair=pattern.clone())
    np.testing.assert_array_equal(dens.cpu().numpy(), ref_d)
    np.testing.assert_array_equal((pair - pattern).cpu().numpy(), ref_p)
    assert dens[0].sum().item() == batch * nelec[0] and dens[1].sum().item() == batch * nelec[1]
    if n == 1:
        assert torch.equal(pair, pattern)                 # no pairs: the pair buffer is untouched
    if nelec[0] < 2:
        assert ref_p[0].sum() == 0
    if min(nelec) == 0:
        assert ref_p[1].sum() == 0


def test_accumulation_and_order_independence():
    cell, x = rh.case('bcc_li')
    ref_dens, ref_pair, r_ws = reference('bcc_li')
    xd = torch.as_tensor(x, device='cuda')
    n_up, prim, grid, n_r = cell.nelec[0], cell.original_cell.a, (2, 3, 5), 64
    args = (prim, grid, cell.a, n_r, r_ws)
    one = counts(xd, n_up, *args)
    # two calls on the same input into fresh buffers are bit-identical
    two = counts(xd, n_up, *args)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    # counts(x[:B1]) then counts(x[B1:]) into the same buffers equals one call on x
    d, p = counts(xd[:400], n_up, *args)
    counts(xd[400:], n_up, *args, dens=d, pair=p)
    assert torch.equal(d, one[0]) and torch.equal(p, one[1])
    # the call adds and never overwrites
    gen = torch.Generator().manual_seed(3)
    d0 = torch.randint(-5, 10 ** 12, (2,) + grid, generator=gen).cuda()
    p0 = torch.randint(-5, 10 ** 12, (3, n_r), generator=gen).cuda()
    d1, p1 = counts(xd, n_up, *args, dens=d0.clone(), pair=p0.clone())
    assert torch.equal(d1 - d0, one[0]) and torch.equal(p1 - p0, one[1])
    # density-only and pair-only calls are the halves of the joint call
    d_only, none = counts(xd, n_up, prim, grid)
    assert none is None and torch.equal(d_only, one[0])
    none, p_only = counts(xd, n_up, a=cell.a, n_r=n_r, r_max=r_ws)
    assert none is None and torch.equal(p_only, one[1])
    np.testing.assert_array_equal(one[0].cpu().numpy(), ref_dens['primitive', grid])
    np.testing.assert_array_equal(one[1].cpu().numpy(), ref_pair[n_r])


def test_constructed_case_without_an_oracle():
    """Cubic cell of edge 8, grid 4^3 (bin width 2, centres 1, 3, 5, 7), r_max = 4 = r_ws, 5 radial bins of width 0.8; nelec
    (2, 2).  e0 (1,1,1) and e1 (7,1,1), both up, are 2 apart across the x face: t = 2.5, bin 2.  e2 (1,7,7), down, is sqrt(8) = 2.83
    from e0 across the y and z faces (t = 3.54, bin 3) and sqrt(12) = 3.46 from e1 across all three (t = 4.33, bin 4).  e3 (5,5,5),
    down, is sqrt(48), 6 and sqrt(24) from e0, e1, e2: beyond r_max.  Three copies of the walker, each electron moved by its own
    lattice vector, some to negative coordinates."""
    a = np.eye(3) * 8.0
    base = np.array([[1.0, 1, 1], [7, 1, 1], [1, 7, 7], [5, 5, 5]])
    moves = np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                      [[-1, 2, 0], [1, 0, -2], [0, -1, 1], [2, 2, -2]],
                      [[-2, -2, -2], [-1, 0, 0], [2, -1, 0], [0, 0, -1]]], dtype=np.float64)
    x = (base[None] + moves @ a).reshape(3, 12)
    assert x.min() < 0
    dens, pair = counts(torch.as_tensor(x, device='cuda'), 2, a, (4, 4, 4), a, 5, 4.0)
    want_d = np.zeros((2, 4, 4, 4), np.int64)
    want_d[0, 0, 0, 0] = want_d[0, 3, 0, 0] = want_d[1, 0, 3, 3] = want_d[1, 2, 2, 2] = 3
    want_p = np.zeros((3, 5), np.int64)
    want_p[0, 2] = want_p[1, 3] = want_p[1, 4] = 3
    np.testing.assert_array_equal(dens.cpu().numpy(), want_d)
    np.testing.assert_array_equal(pair.cpu().numpy(), want_p)
    # the same walkers in float32 (all coordinates are small integers: exact)
    dens32, pair32 = counts(torch.as_tensor(x, dtype=torch.float32, device='cuda'), 2, a, (4, 4, 4), a, 5, 4.0)
    assert torch.equal(dens32, dens) and torch.equal(pair32, pair)


@pytest.mark.parametrize('name', ['graphene', 'triclinic', 'lih'])
def test_float32_walkers(name):
    """float32 walkers are widened to float64 on load: the counts equal the oracle at the same rounded walkers."""
    cell, x = rh.case(name)
    x32 = x[:64].astype(np.float32)
    xr = x32.astype(np.float64)
    r_ws = estimator.wigner_seitz_radius(cell.a)
    prim = cell.original_cell.a
    ref_d, m_d = rh.density_oracle(xr, cell.nelec[0], prim, (2, 3, 5))
    ref_p, m_p = rh.pair_oracle(xr, cell.nelec[0], cell.a, 64, r_ws)
    assert m_d >= rh.MARGIN and m_p >= rh.MARGIN
    dens, pair = counts(torch.as_tensor(x32, device='cuda'), cell.nelec[0], prim, (2, 3, 5), cell.a, 64, r_ws)
    np.testing.assert_array_equal(dens.cpu().numpy(), ref_d)
    np.testing.assert_array_equal(pair.cpu().numpy(), ref_p)
    d64, p64 = counts(torch.as_tensor(xr, device='cuda'), cell.nelec[0], prim, (2, 3, 5), cell.a, 64, r_ws)
    assert torch.equal(d64, dens) and torch.equal(p64, pair)


def test_argument_errors():
    cell, x = rh.case('lih')
    xd = torch.as_tensor(x[:8], device='cuda')
    dens = torch.zeros(2, 2, 3, 5, dtype=torch.int64, device='cuda')
    pair = torch.zeros(3, 7, dtype=torch.int64, device='cuda')
    kw = dict(dens=dens, fold_lattice=cell.a, pair=pair, latvec=cell.a, r_max=2.0)
    with pytest.raises(RuntimeError, match='ROCm device'):
        device.realspace_counts(xd.cpu(), 2, **kw)
    with pytest.raises(TypeError, match='float64 or float32'):
        device.realspace_counts(xd.half(), 2, **kw)
    with pytest.raises(ValueError, match='shape'):
        device.realspace_counts(xd[:, :10], 2, **kw)
    with pytest.raises(ValueError, match='empty'):
        device.realspace_counts(xd[:0], 2, **kw)
    with pytest.raises(ValueError, match='neither'):
        device.realspace_counts(xd, 2)
    with pytest.raises(TypeError, match='int64'):
        device.realspace_counts(xd, 2, **dict(kw, dens=dens.int()))
    with pytest.raises(RuntimeError, match='lives on'):
        device.realspace_counts(xd, 2, **dict(kw, pair=pair.cpu()))
    with pytest.raises(ValueError, match='shape'):
        device.realspace_counts(xd, 2, **dict(kw, pair=pair[:2].contiguous()))
    with pytest.raises(ValueError, match='fold_lattice'):
        device.realspace_counts(xd, 2, dens=dens)
    with pytest.raises(ValueError, match='r_max'):
        device.realspace_counts(xd, 2, pair=pair, latvec=cell.a)
    with pytest.raises(RuntimeError, match='n_up'):
        device.realspace_counts(xd, 5, **kw)
    with pytest.raises(RuntimeError, match='r_max'):
        device.realspace_counts(xd, 2, **dict(kw, r_max=-1.0))
    with pytest.raises(RuntimeError, match='grid'):
        device.realspace_counts(xd, 2, dens=torch.zeros(2, 257, 1, 1, dtype=torch.int64, device='cuda'), fold_lattice=cell.a)
    with pytest.raises(RuntimeError, match='n_r'):
        device.realspace_counts(xd, 2, pair=torch.zeros(3, 1025, dtype=torch.int64, device='cuda'), latvec=cell.a, r_max=2.0)
    with pytest.raises(RuntimeError, match='n_elec'):
        device.realspace_counts(torch.zeros(2, 3 * 129, dtype=torch.float64, device='cuda'), 2, **kw)
    assert dens.sum().item() == 0 and pair.sum().item() == 0          # nothing was launched


def test_accumulator_update_merge_and_results():
    """`RealSpaceAccumulator` on the device: two updates equal the oracle of all walkers, the results are normalised, and a
    saved part merged into a continued run gives the counts of one run."""
    cell, x = rh.case('lih')
    ref_dens, ref_pair, r_ws = reference('lih')
    xd = torch.as_tensor(x, device='cuda')
    acc = estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 5), pair_bins=64)
    acc.update(xd[:300])
    acc.update(xd[300:])
    assert acc.n_walkers == x.shape[0] and acc.dens.is_cuda and acc.pair.is_cuda
    np.testing.assert_array_equal(acc.density_counts(), ref_dens['primitive', (2, 3, 5)])
    np.testing.assert_array_equal(acc.pair_counts(), ref_pair[64])
    dv = abs(np.linalg.det(cell.original_cell.a)) / 30
    assert np.allclose(acc.density().sum(axis=(1, 2, 3)) * dv, np.asarray(cell.nelec) / cell.scale, rtol=0, atol=1e-12)
    first = estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 5), pair_bins=64)
    first.update(xd[:300])
    rest = estimator.RealSpaceAccumulator.from_state_dict(first.state_dict())     # as loaded from a file: counts on the host
    rest.update(xd[300:])
    np.testing.assert_array_equal(rest.pair_counts(), ref_pair[64])
    np.testing.assert_array_equal(rest.density_counts(), acc.density_counts())


def test_run_inference_with_accumulators(tmp_path):
    """Three iterations on the LiH fixture network: realspace.npz holds the oracle's counts of the walkers of the three
    iterations (the same seeded `mcmc_step` calls repeated outside the driver); rows and CSV are those of a run without."""
    from deepsolid_amd import inference, qmc
    cell, slog, ld, dp, x0 = rh.lih_drivers(64)
    x0 = x0[:24].contiguous()
    kw = dict(iterations=3, key=17, move_width=0.3, mcmc_steps=4, burn_in=0)
    acc = estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 5), pair_bins=7)
    with_acc, without = tmp_path / 'with', tmp_path / 'without'
    data, width, rows = inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(with_acc), accumulators=(acc,), **kw)
    data2, width2, rows2 = inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(without), **kw)
    assert torch.equal(data, data2) and width == width2 and rows == rows2
    assert (with_acc / 'train_stats.csv').read_text() == (without / 'train_stats.csv').read_text()
    assert not (without / 'realspace.npz').exists()
    # the walkers of the three iterations
    gen = inference._rank_generator(17, x0.device)
    step = qmc.make_mcmc_step(slog.apply, x0.shape[0], latvec=cell.a, steps=4)
    walkers, d = [], x0.clone()
    for _ in range(3):
        d, _ = step(dp, d, gen, 0.3)
        walkers.append(d.cpu().numpy().copy())
    assert np.array_equal(walkers[-1], data.cpu().numpy())
    xs = np.concatenate(walkers)
    ref_d, m_d = rh.density_oracle(xs, cell.nelec[0], cell.original_cell.a, (2, 3, 5))
    ref_p, m_p = rh.pair_oracle(xs, cell.nelec[0], cell.a, 7, acc.r_max)
    assert m_d >= rh.MARGIN and m_p >= rh.MARGIN
    with np.load(str(with_acc / 'realspace.npz')) as f:
        np.testing.assert_array_equal(f['density_counts'], ref_d)
        np.testing.assert_array_equal(f['pair_counts'], ref_p)
        assert int(f['n_walkers']) == 3 * x0.shape[0] and bool(f['reduced'])
        np.testing.assert_array_equal(f['simulation_lattice'], cell.a)
        np.testing.assert_array_equal(f['fold_lattice'], cell.original_cell.a)
        assert f['grid'].tolist() == [2, 3, 5] and f['r_edges'].shape == (8,) and f['r_edges'][-1] == acc.r_max
        np.testing.assert_array_equal(f['density'], acc.density())
        np.testing.assert_array_equal(f['g'], acc.pair_correlation()[1])
    with pytest.raises(RuntimeError, match='already'):
        acc.reduce()


def _walkers_of(slog, dp, cell, x0, key, iterations, width=0.3, steps=4):
    """The walkers `run_inference(burn_in=0)` evaluates: the same seeded `mcmc_step` calls outside the driver."""
    from deepsolid_amd import inference, qmc
    gen = inference._rank_generator(key, x0.device)
    step = qmc.make_mcmc_step(slog.apply, x0.shape[0], latvec=cell.a, steps=steps)
    out, d = [], x0.clone()
    for _ in range(iterations):
        d, _ = step(dp, d, gen, width)
        out.append(d.cpu().numpy().copy())
    return out


def test_continue_from_the_file_run_inference_wrote(tmp_path):
    """realspace.npz of a finished run (written after its reduce()) is loaded and handed to a second `run_inference`: the
    second file holds the counts of the walkers of both runs."""
    from deepsolid_amd import inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(64)
    x0 = x0[:24].contiguous()
    kw = dict(move_width=0.3, mcmc_steps=4, burn_in=0)
    first = estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 5), pair_bins=7)
    data, _, _ = inference.run_inference(slog, ld, dp, x0.clone(), cell, iterations=2, key=17, save_path=str(tmp_path / 'a'),
                                         accumulators=(first,), **kw)
    more = estimator.RealSpaceAccumulator.load(str(tmp_path / 'a' / 'realspace.npz'))
    assert not more.reduced and more.n_walkers == 48
    inference.run_inference(slog, ld, dp, data.clone(), cell, iterations=2, key=18, save_path=str(tmp_path / 'b'),
                            accumulators=(more,), **kw)
    xs = np.concatenate(_walkers_of(slog, dp, cell, x0, 17, 2) + _walkers_of(slog, dp, cell, data, 18, 2))
    ref_d, m_d = rh.density_oracle(xs, cell.nelec[0], cell.original_cell.a, (2, 3, 5))
    ref_p, m_p = rh.pair_oracle(xs, cell.nelec[0], cell.a, 7, first.r_max)
    assert m_d >= rh.MARGIN and m_p >= rh.MARGIN
    with np.load(str(tmp_path / 'b' / 'realspace.npz')) as f:
        assert int(f['n_walkers']) == 96
        np.testing.assert_array_equal(f['density_counts'], ref_d)
        np.testing.assert_array_equal(f['pair_counts'], ref_p)


def test_a_run_that_raises_keeps_its_counts(tmp_path):
    """An exception inside the loop: no reduce, no realspace.npz, but the unreduced counts of the iterations that were
    accumulated are in realspace_partial_rank0.npz, and the exception goes on."""
    from deepsolid_amd import inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(64)
    x0 = x0[:24].contiguous()

    class Interrupted(estimator.RealSpaceAccumulator):
        def update(self, data):
            if self.n_walkers >= 48:
                raise KeyboardInterrupt
            super().update(data)

    acc = Interrupted(cell, density_grid=(2, 3, 5), pair_bins=7)
    with pytest.raises(KeyboardInterrupt):
        inference.run_inference(slog, ld, dp, x0.clone(), cell, iterations=4, key=17, move_width=0.3, mcmc_steps=4, burn_in=0,
                                save_path=str(tmp_path), accumulators=(acc,))
    assert not (tmp_path / 'realspace.npz').exists() and not acc.reduced
    part = estimator.RealSpaceAccumulator.load(str(tmp_path / 'realspace_partial_rank0.npz'))
    xs = np.concatenate(_walkers_of(slog, dp, cell, x0, 17, 2))
    ref_p, m_p = rh.pair_oracle(xs, cell.nelec[0], cell.a, 7, acc.r_max)
    assert m_p >= rh.MARGIN and part.n_walkers == 48
    np.testing.assert_array_equal(part.pair_counts(), ref_p)
    assert len((tmp_path / 'train_stats.csv').read_text().splitlines()) == 3      # header + the two finished iterations
