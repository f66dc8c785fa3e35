"""CPU checks of the real-space observables (deepsolid_amd/estimator.py `RealSpaceAccumulator`, csrc/ds_realspace.h): the C ABI's
symbol, header text and refusals (all answered before any launch), the host geometry (Wigner-Seitz radius, plane spacings), the
normalisation of the density and of g(r) on counts of the numpy oracle (tests/realspace_helpers.py), merge / save / load, and the
2-rank reduction over gloo."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import realspace_helpers as rh
from deepsolid_amd import estimator, systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from deepsolid_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L, L.load()


def _filled(cell, x, **kw):
    """An accumulator holding the oracle's counts of the walkers x (what `update` leaves on the GPU)."""
    acc = estimator.RealSpaceAccumulator(cell, **kw)
    if acc.grid is not None:
        acc.dens = torch.as_tensor(rh.density_oracle(x, cell.nelec[0], acc.fold, acc.grid)[0])
    if acc.n_r is not None:
        acc.pair = torch.as_tensor(rh.pair_oracle(x, cell.nelec[0], cell.a, acc.n_r, acc.r_max)[0])
    acc.n_walkers = x.shape[0]
    return acc


def test_cabi_exports_realspace_counts():
    L, lib = _lib()
    assert hasattr(lib, 'ds_realspace_counts') and 'ds_realspace_counts' in L.SIGNATURES
    hdr = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    assert 'int ds_realspace_counts(' in hdr
    # the binning rules are part of the interface
    for rule in ('f = r . inv(A_f), f -= floor(f), i_j = min(int(f_j * g_j), g_j - 1)', '(i0*g1 + i1)*g2 + i2',
                 'f = (r_i - r_j) . inv(A), f -= floor(f + 1/2)', 'k = int(r * n_r / r_max)', 'only if r < r_max'):
        assert rule in hdr, rule
    assert os.path.exists(os.path.join(ROOT, 'deepsolid_amd', 'csrc', 'ds_realspace.h'))
    assert 'ds_realspace_counts' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_cabi_refusals_without_a_launch():
    """Every limit of the kernel is answered by ds_last_error before anything touches a device."""
    _, lib = _lib()
    eye = np.ascontiguousarray(np.eye(3) * 5.0)
    inv = np.ascontiguousarray(np.linalg.inv(eye))
    pd = lambda m: m.ctypes.data_as(C.POINTER(C.c_double))
    fake = C.c_void_p(0x1000)           # never dereferenced: every call below fails validation first

    def call(fold=inv, grid=(4, 4, 4), a=eye, a_inv=inv, r_max=2.0, n_r=8, dtype=0, x=fake, B=4, n=4, n_up=2, dens=fake, pair=fake):
        g = np.asarray(grid, dtype=np.int32) if grid is not None else None
        rc = lib.ds_realspace_counts(pd(fold) if fold is not None else None,
                                     g.ctypes.data_as(C.POINTER(C.c_int32)) if g is not None else None,
                                     pd(a) if a is not None else None, pd(a_inv) if a_inv is not None else None, r_max, n_r, dtype,
                                     x, B, n, n_up, dens, pair, None)
        return rc, lib.ds_last_error().decode()

    nan = eye.copy()
    nan[1, 2] = np.nan
    cases = [(dict(x=None), 'null argument'), (dict(dens=None, pair=None), 'both null'), (dict(dtype=2), 'dtype'),
             (dict(B=0), 'B must be'), (dict(B=-3), 'B must be'), (dict(n=0), 'n_elec'), (dict(n=129), 'n_elec'),
             (dict(n_up=-1), 'n_up'), (dict(n_up=5), 'n_up'), (dict(grid=(0, 4, 4)), 'grid[0]'), (dict(grid=(4, 257, 4)), 'grid[1]'),
             (dict(grid=(4, 4, -1)), 'grid[2]'), (dict(grid=(256, 256, 128)), 'grid has'), (dict(fold=None), 'fold_inv'),
             (dict(grid=None), 'grid'), (dict(fold=nan), 'not finite'), (dict(n_r=0), 'n_r'), (dict(n_r=1025), 'n_r'),
             (dict(r_max=0.0), 'r_max'), (dict(r_max=-1.0), 'r_max'), (dict(r_max=float('nan')), 'r_max'),
             (dict(a=None), 'latvec'), (dict(a_inv=None), 'latvec'), (dict(a=nan), 'not finite'), (dict(a_inv=nan), 'not finite')]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
    # a part whose buffer is NULL is skipped, so its own arguments are not looked at: these fail only for the OTHER part
    rc, err = call(pair=None, a=None, a_inv=None, n_r=0, r_max=0.0, grid=(0, 1, 1))
    assert rc != 0 and 'grid[0]' in err
    rc, err = call(dens=None, fold=None, grid=None, n_r=2000)
    assert rc != 0 and 'n_r' in err


def test_accumulator_refusals():
    cell, _ = systems.build('lih')
    A = estimator.RealSpaceAccumulator
    with pytest.raises(ValueError, match='neither'):
        A(cell)
    for grid in (0, 257, (4, 4), (4, 0, 4), (256, 256, 128), 2.5):
        with pytest.raises(ValueError, match='density_grid'):
            A(cell, density_grid=grid)
    with pytest.raises(ValueError, match='density_cell'):
        A(cell, density_grid=4, density_cell='conventional')
    with pytest.raises(ValueError, match='density_cell'):
        A(cell, density_grid=4, density_cell=np.zeros((3, 3)))
    for bins in (0, 1025, 2.5):
        with pytest.raises(ValueError, match='pair_bins'):
            A(cell, pair_bins=bins)
    with pytest.raises(ValueError, match='pair_rmax'):
        A(cell, pair_bins=8, pair_rmax=0.0)
    with pytest.raises(ValueError, match='pair_rmax'):
        A(cell, density_grid=4, pair_rmax=1.0)
    r_ws = estimator.wigner_seitz_radius(cell.a)
    with pytest.raises(ValueError, match='Wigner-Seitz'):
        A(cell, pair_bins=8, pair_rmax=r_ws * (1 + 1e-12))
    assert A(cell, pair_bins=8, pair_rmax=r_ws).r_max == r_ws == A(cell, pair_bins=8).r_max
    # the cubic lattice of edge 10 in a skewed basis: r_ws = 5 by the lattice vectors, but the planes spanned by a_1 and a_2 are
    # 10 / sqrt(10) = 3.16 apart in this basis, and 1.5 x 3.16 < 4.9
    skewed = rh.SimpleCell(np.array([[10.0, 0, 0], [0, 10.0, 0], [30.0, 0, 10.0]]), (1, 1))
    assert abs(estimator.wigner_seitz_radius(skewed.a) - 5.0) < 1e-15
    assert abs(estimator.plane_spacings(skewed.a).min() - np.sqrt(10.0)) < 1e-12
    for r_max in (4.9, None):
        with pytest.raises(ValueError, match='plane spacing'):
            A(skewed, pair_bins=8, pair_rmax=r_max)
    assert A(skewed, pair_bins=8, pair_rmax=4.7).r_max == 4.7
    with pytest.raises(ValueError, match='electrons'):
        A(rh.cubic_cell(100, 29), pair_bins=8)
    acc = A(cell, density_grid=4)
    with pytest.raises(ValueError, match='coordinates'):
        acc.update(torch.zeros(3, 9))
    with pytest.raises(RuntimeError, match='ROCm device'):
        acc.update(torch.zeros(3, 12))
    with pytest.raises(ValueError, match='no pair counts'):
        acc.pair_correlation()
    with pytest.raises(ValueError, match='no density'):
        A(cell, pair_bins=4).density()


def test_wigner_seitz_radius_and_plane_spacings():
    """The four library cells: r_ws to the four decimals of the table in DESIGN.md section 15, and in closed form (bcc 2x2x2: half the
    primitive vector sqrt(3)/2 a0 doubled; graphene 2x2: the in-plane vector 2 L; fcc cells: L / sqrt(2) times the tiling)."""
    documented = {'bcc_li': 5.6082, 'graphene': 4.6487, 'lih': 2.6725, 'diamond': 4.7664}
    bohr = 1.0 / 0.52917721067
    closed = {'bcc_li': 0.5 * np.sqrt(3) * 3.4268178940 * bohr, 'graphene': 2.46 * bohr, 'lih': 0.5 * 4.0 * bohr / np.sqrt(2),
              'diamond': 3.567 * bohr / np.sqrt(2)}
    for name, r in documented.items():
        cell, _ = systems.build(name)
        r_ws = estimator.wigner_seitz_radius(cell.a)
        d = estimator.plane_spacings(cell.a)
        assert abs(r_ws - r) <= 5e-5 and abs(r_ws - closed[name]) < 1e-12, (name, r_ws)
        # spacing j = V / |a_k x a_l|
        vol = abs(np.linalg.det(cell.a))
        for j in range(3):
            assert abs(d[j] - vol / np.linalg.norm(np.cross(cell.a[(j + 1) % 3], cell.a[(j + 2) % 3]))) < 1e-12
        assert r_ws < 1.5 * d.min()
    assert abs(estimator.wigner_seitz_radius(rh.TRICLINIC) - 2.5) < 1e-15
    assert estimator.wigner_seitz_radius(rh.TRICLINIC) < 1.5 * estimator.plane_spacings(rh.TRICLINIC).min()
    # a lattice whose shortest vector is not a basis vector: a_0 - a_1 = (1, -1, 0) x 0.1
    skew = np.array([[4.0, 0, 0], [3.9, 0.1, 0], [0, 0, 5.0]])
    assert abs(estimator.wigner_seitz_radius(skew) - 0.5 * np.hypot(0.1, 0.1)) < 1e-15


@pytest.mark.parametrize('name', ['bcc_li', 'lih', 'triclinic'])
def test_density_integrates_to_the_electrons_per_folding_cell(name):
    cell, x = rh.case(name)
    x = x[:40]
    for fold, grid, per_cell in (('primitive', (2, 3, 5), 1.0 / getattr(cell, 'scale', 1)), ('simulation', 16, 1.0)):
        acc = _filled(cell, x, density_grid=grid, density_cell=fold)
        rho = acc.density()
        assert rho.shape == (2,) + acc.grid and rho.dtype == np.float64
        dv = abs(np.linalg.det(acc.fold)) / np.prod(acc.grid)
        for s in (0, 1):
            assert abs(rho[s].sum() * dv - cell.nelec[s] * per_cell) < 1e-12
            assert acc.density_counts()[s].sum() == 40 * cell.nelec[s]


def test_pair_correlation_of_uniform_walkers_is_one():
    """4096 independent uniform walkers in bcc-Li (seed 5): for every channel and every bin whose expected count is >= 100,
    |g - 1| <= 6 sqrt((1 - p_k) / (n p_k)) with p_k = V_shell_k / V_sim and n = n_walkers P_c.  Pair indicators of independent
    uniform points on a torus are pairwise independent, so this is six exact binomial standard deviations."""
    cell, _ = systems.build('bcc_li')
    x = systems.synthetic_walkers(cell, 4096, seed=5)
    acc = _filled(cell, x, pair_bins=64)
    r_mid, g = acc.pair_correlation()
    edges = acc.r_edges()
    assert r_mid.shape == (64,) and g.shape == (3, 64) and abs(edges[-1] - acc.r_ws) < 1e-15
    np.testing.assert_allclose(r_mid, 0.5 * (edges[1:] + edges[:-1]))
    p = 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3) / abs(np.linalg.det(cell.a))
    checked = 0
    for c, pc in enumerate((66, 144, 66)):
        n = 4096 * pc
        big = n * p >= 100
        assert big.sum() >= 40
        assert np.all(np.abs(g[c][big] - 1) <= 6 * np.sqrt((1 - p[big]) / (n * p[big])))
        checked += big.sum()
    assert checked >= 120
    # channels without pairs are NaN, the others are not touched by that
    one = _filled(rh.SimpleCell(cell.a, (1, 3)), x[:50, :12], pair_bins=4)
    g1 = one.pair_correlation()[1]
    assert np.all(np.isnan(g1[0])) and np.all(np.isfinite(g1[1:]))


def test_merge_save_load_round_trip(tmp_path):
    cell, x = rh.case('lih')
    kw = dict(density_grid=(2, 3, 5), pair_bins=7)
    whole, a, b = _filled(cell, x[:60], **kw), _filled(cell, x[:25], **kw), _filled(cell, x[25:60], **kw)
    a.merge(b)
    assert a.n_walkers == 60
    np.testing.assert_array_equal(a.density_counts(), whole.density_counts())
    np.testing.assert_array_equal(a.pair_counts(), whole.pair_counts())
    # through a file: a long run continues by adding counts
    path = str(tmp_path / 'part.npz')
    _filled(cell, x[:25], **kw).save(path)
    back = estimator.RealSpaceAccumulator.load(path)
    assert back.n_walkers == 25 and back.grid == (2, 3, 5) and back.n_r == 7 and back.nelec == tuple(cell.nelec)
    np.testing.assert_array_equal(back.fold, cell.original_cell.a)
    back.merge(b)
    np.testing.assert_array_equal(back.pair_counts(), whole.pair_counts())
    np.testing.assert_array_equal(back.density(), whole.density())
    np.testing.assert_array_equal(back.pair_correlation()[1], whole.pair_correlation()[1])
    # state_dict / load_state_dict on an existing accumulator; another setup is refused
    fresh = estimator.RealSpaceAccumulator(cell, **kw)
    fresh.load_state_dict(whole.state_dict())
    assert fresh.n_walkers == 60 and fresh.density_counts().dtype == np.int64
    np.testing.assert_array_equal(fresh.density_counts(), whole.density_counts())
    with pytest.raises(ValueError, match='another cell'):
        estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 5), pair_bins=8).load_state_dict(whole.state_dict())
    with pytest.raises(ValueError, match='differ'):
        whole.merge(estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 4), pair_bins=7))
    # the file run_inference writes carries the normalised results as well
    whole.save(str(tmp_path / 'full.npz'), results=True)
    with np.load(str(tmp_path / 'full.npz')) as f:
        assert set(f.files) == {'n_walkers', 'simulation_lattice', 'nelec', 'reduced', 'density_counts', 'fold_lattice', 'grid',
                                'pair_counts', 'r_edges', 'pair_rmax', 'density', 'r_mid', 'g'}
        np.testing.assert_array_equal(f['density'], whole.density())
        np.testing.assert_array_equal(f['g'], whole.pair_correlation()[1])
    # an accumulator that never saw a walker: zero counts, NaN results, and it still saves and loads
    empty = estimator.RealSpaceAccumulator(cell, **kw)
    assert empty.density_counts().sum() == 0 and np.all(np.isnan(empty.density()))
    empty.save(str(tmp_path / 'empty.npz'))
    assert estimator.RealSpaceAccumulator.load(str(tmp_path / 'empty.npz')).n_walkers == 0


def test_reduce_is_the_identity_at_world_size_one(monkeypatch):
    from deepsolid_amd import constants
    calls = []
    monkeypatch.setattr(constants.dist, 'all_reduce', lambda t, **kw: calls.append(t.numel()))
    cell, x = rh.case('lih')
    acc = _filled(cell, x[:10], density_grid=2, pair_bins=3)
    before = acc.density_counts().copy(), acc.pair_counts().copy()
    assert acc.reduce() is acc and calls == [] and acc.n_walkers == 10
    np.testing.assert_array_equal(acc.density_counts(), before[0])
    np.testing.assert_array_equal(acc.pair_counts(), before[1])
    with pytest.raises(RuntimeError, match='already'):
        acc.reduce()
    with pytest.raises(RuntimeError, match='after reduce'):
        acc.update(torch.zeros(1, 12))


def test_two_rank_reduce_over_gloo(tmp_path):
    """Each rank holds the oracle counts of its own walkers; ONE all-reduce of the int64 counts with the walker number as the
    trailing element leaves the counts of all walkers on both ranks.  A second reduce() raises."""
    script = tmp_path / 'worker.py'
    script.write_text('''
import sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from deepsolid_amd import constants, estimator
import realspace_helpers as rh
from test_realspace_cpu import _filled
dist.init_process_group('gloo')
r = dist.get_rank()
sizes = []
orig = dist.all_reduce
def recording(t, *a, **k):
    sizes.append((t.numel(), t.dtype))
    return orig(t, *a, **k)
constants.dist.all_reduce = recording
cell, x = rh.case('lih')
kw = dict(density_grid=(2, 3, 5), pair_bins=7)
mine = x[:20] if r == 0 else x[20:50]
acc = _filled(cell, mine, **kw)
whole = _filled(cell, x[:50], **kw)
acc.reduce()
assert sizes == [(2 * 30 + 3 * 7 + 1, torch.int64)], sizes
assert acc.n_walkers == 50
np.testing.assert_array_equal(acc.density_counts(), whole.density_counts())
np.testing.assert_array_equal(acc.pair_counts(), whole.pair_counts())
np.testing.assert_array_equal(acc.density(), whole.density())
try:
    acc.reduce()
    raise SystemExit('second reduce() did not raise')
except RuntimeError:
    pass
assert len(sizes) == 1
# pair-only accumulator: only its counts travel
del sizes[:]
p = _filled(cell, mine, pair_bins=4)
p.reduce()
assert sizes == [(3 * 4 + 1, torch.int64)] and p.n_walkers == 50
np.testing.assert_array_equal(p.pair_counts(), _filled(cell, x[:50], pair_bins=4).pair_counts())
dist.destroy_process_group()
print('rank', r, 'ok')
''' % (ROOT, os.path.join(ROOT, 'tests')))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                          '--master-addr', '127.0.0.1', '--master-port', '29561', str(script)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count('ok') == 2


def test_run_inference_default_takes_no_accumulators():
    import inspect
    from deepsolid_amd import inference
    assert inspect.signature(inference.run_inference).parameters['accumulators'].default == ()


def test_a_file_written_after_reduce_continues(tmp_path):
    """`run_inference` always writes after `reduce()`.  The file must still continue a run: a loaded accumulator is rank-local
    and open, and may be reduced once more; the file itself records that it was written after a reduce."""
    cell, x = rh.case('lih')
    acc = _filled(cell, x[:25], density_grid=(2, 3, 5), pair_bins=7)
    acc.reduce()
    path = str(tmp_path / 'realspace.npz')
    acc.save(path, results=True)
    with np.load(path) as f:
        assert bool(f['reduced'])
    more = estimator.RealSpaceAccumulator.load(path)
    assert not more.reduced and more.n_walkers == 25
    with pytest.raises(RuntimeError, match='ROCm device'):           # not 'after reduce': update is open (and has no CPU path)
        more.update(torch.zeros(2, 12))
    more.merge(_filled(cell, x[25:60], density_grid=(2, 3, 5), pair_bins=7))
    np.testing.assert_array_equal(more.pair_counts(), _filled(cell, x[:60], pair_bins=7).pair_counts())
    assert more.reduce().reduced and more.n_walkers == 60
    fresh = estimator.RealSpaceAccumulator(cell, density_grid=(2, 3, 5), pair_bins=7)
    assert not fresh.load_state_dict(acc.state_dict()).reduced


def test_reduce_marks_only_after_success(monkeypatch):
    from deepsolid_amd import constants
    cell, x = rh.case('lih')
    acc = _filled(cell, x[:10], pair_bins=3)
    before = acc.pair_counts().copy()
    monkeypatch.setattr(constants, 'world_size', lambda: 2)

    def broken(t):
        raise RuntimeError('collective failed')
    monkeypatch.setattr(constants, 'psum_if_pmap', broken)
    with pytest.raises(RuntimeError, match='collective failed'):
        acc.reduce()
    assert not acc.reduced and acc.n_walkers == 10
    np.testing.assert_array_equal(acc.pair_counts(), before)
    # with more than one rank, merge refuses a reduced / rank-local pair
    monkeypatch.setattr(constants, 'psum_if_pmap', lambda t: 2 * t)
    acc.reduce()
    assert acc.reduced and acc.n_walkers == 20
    with pytest.raises(ValueError, match='rank-local'):
        acc.merge(_filled(cell, x[:10], pair_bins=3))
    with pytest.raises(ValueError, match='rank-local'):
        _filled(cell, x[:10], pair_bins=3).merge(acc)
    monkeypatch.setattr(constants, 'world_size', lambda: 1)
    assert acc.merge(_filled(cell, x[:10], pair_bins=3)).n_walkers == 30


@pytest.mark.parametrize('name', ['bcc_li', 'graphene', 'lih', 'triclinic'])
def test_kernel_algorithm_equals_the_brute_force_oracle(name):
    """The kernel's pair algorithm restated in numpy (`realspace_helpers.pair_kernel_algorithm`: the float32 pair-index decode,
    the wrapped difference, the shortest of 27 images, the clamp) against the 125-shift oracle: the same integers, so the 27
    shifts are enough on these cells and the decode visits every pair once."""
    cell, x = rh.case(name)
    x = x[:200]
    r_ws = estimator.wigner_seitz_radius(cell.a)
    dist, chan = rh.pair_images(x, cell.nelec[0], cell.a, 2.0 * r_ws)
    for n_r in (1, 7, 64, 1024):
        ref, margin = rh.bin_pairs(dist, chan, n_r, r_ws)
        assert margin >= rh.MARGIN
        np.testing.assert_array_equal(rh.pair_kernel_algorithm(x, cell.nelec[0], cell.a, n_r, r_ws), ref)
    lo, hi = rh.pair_index_decode(128)
    i, j = np.triu_indices(128, 1)
    assert sorted(zip(lo.tolist(), hi.tolist())) == sorted(zip(i.tolist(), j.tolist()))
