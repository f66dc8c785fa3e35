"""GPU tests of the KFAC factor pass `ds_kfac_factors` (csrc/ds_kfac.h) through the C ABI, against the torch restatement of
tests/kfac_helpers.py (activations captured in the oracle's forward, dy from torch.autograd of sum_b sqrt2 log|psi_b|).

The placement of the blocks and the seed are pinned by that restatement only (the reference's jaxpr tracer cannot run outside
JAX); the arithmetic on them -- which rows, which order, which divisor -- is what these tests hold the kernels to.
Bound (float64): every factor within 1e-9 of its largest entry, the bound test_vjp_vs_oracle_autograd holds the same sweep to;
symmetry exact.  The deviations measured are recorded as test properties.
Measured on an MI355X, worst over each group of cases, of a factor's (a leaf's) largest entry:
  factors / seed gradient, the 17 earlier cases (lih ... graphene): 1.9e-12 / 5.2e-13 (graphene; 3.2e-13 / 2.2e-13 without it);
  twisted, bcc-lattice, doubled, triclinic and two-electron cells: 2.7e-13 / 1.2e-13;
  bcc_li_333 / graphene_331 / diamond at B = 2: 2.4e-13 / 1.0e-12 / 1.1e-12 (gradient 1.6e-13 / 1.3e-12 / 4.2e-13); diamond B = 83:
  3.3e-12 / 1.8e-12; bcc_li_333 B = 4: 1.4e-13 / 9.6e-14;
  int8 value chain at production batches (bcc-Li 1843 / graphene 903 / diamond 403): (a) int8 2.1e-12 / 3.6e-11 / 7.4e-11 (gradient
  1.4e-12 / 2.0e-11 / 4.7e-11), float64 layers 6.1e-14 / 4.3e-12 / 4.2e-12; (d) 1.5e-13 / 9.9e-13 / 7.7e-11 (diamond's passes are
  all float64: (d) is the int8 loss there);
  int8 forced on tiny batches (lih 5 / bcc-Li 3 / graphene 1): 2.1e-12 / 2.3e-12 / 8.8e-12;
  float32 (lih / bcc-Li / diamond), worst factor against its budget: 3.1e-5 of 5.1e-5 / 4.3e-5 of 9.0e-5 / 3.7e-4 of 7.7e-4; the
  kernel's deviation is at most 2.2 x the restatement's own float32 loss of the same factor (lih, the last G; 1.5 x on diamond)."""
import functools

import numpy as np
import pytest
import torch

import kfac_helpers as kh
from common import float32_tolerance, load_case
from deepsolid_amd import systems
from test_gpu_grad import dev_params, fresh_system, leaf_devs, system_for

pytestmark = pytest.mark.gpu

# (case, batch): one walker, a ragged group, exactly one group of PV = 80 walkers, a group plus three; padded and unequal
# widths over four layers, a dropped spin channel, orbital bias, use_last_layer, full_det, the diagonal envelope, a
# determinant count that does not fill the orbital head's column tiles, and the 12-electron graphene cell
FACTOR_CASES = [('lih', 1), ('lih', 5), ('lih', 80), ('lih', 83), ('bcc_li', 1), ('bcc_li', 5), ('bcc_li', 80), ('bcc_li', 83),
                ('lih_narrow', 3), ('lih_mixed', 3), ('li_polarized', 3), ('lih_bias', 3), ('lih_lastlayer', 3),
                ('bcc_li_fulldet', 3), ('lih_diagenv', 3), ('lih_det3', 3), ('graphene', 2),
                # complex k-points in the dy of the orbital head; the bcc symmetry lattice, a doubled cell, a triclinic cell
                # (wider input features) and the two-electron cell
                ('lih_twist', 3), ('bcc_li_twist', 3), ('bcc_li_bcc', 2), ('lih_2x1x1', 3), ('lih_tri', 3), ('h2', 3),
                # orbital heads beyond 192 columns: 656 / 640 (a ragged last block of 16, unequal non-empty spin channels 41 / 40,
                # N^2 = 6561 pairs: not a multiple of 16), 864 (27 block rows, 378 blocks), 768
                ('bcc_li_333', 2), ('graphene_331', 2), ('diamond', 2),
                # B = 4 fills the four-column step of the walker axis, so only the pair axis (6561 = 4 * 1640 + 1) meets the
                # `jq + s < qlim` mask inside a step
                ('bcc_li_333', 4),
                # one full group plus three walkers at 96 electrons
                ('diamond', 83)]
# the batches of the tests that take distinct walkers from `reference` without being factor cases
TINY_I8_CASES = [('lih', 5), ('bcc_li', 3), ('graphene', 1)]
F32_CASES = [('lih', 5), ('bcc_li', 5), ('diamond', 2)]
# the production batches of test_gpu_grad.I8_VJP_CASES: 24 x 24, 12 x 48 and 6 x 96 (group, electron) tiles, a ragged last group
I8_FACTOR_CASES = [('bcc_li', 1843), ('graphene', 903), ('diamond', 403)]
I8_DISTINCT = 29


BATCHES = {}
for _name, _batch in FACTOR_CASES + TINY_I8_CASES + F32_CASES:
    BATCHES.setdefault(_name, set()).add(_batch)


@functools.lru_cache(maxsize=None)
def per_walker(name):
    """The largest batch of a case -- all walkers distinct -- and, for every batch size b the case is used at, the sums over
    its first b walkers of the restatement's (factors, gradient tree) of each walker ALONE, added in walker order.  Computed
    once per case and shared by its batch sizes; only the running sums are kept (a walker's factors are 14 to 26 MB)."""
    fx, cell, klist, net_kw, params = load_case(name)
    n = max(BATCHES[name])
    x = systems.synthetic_walkers(cell, n, seed=91)
    assert len(np.unique(x.round(12), axis=0)) == n
    sums, fsum, gsum = {}, None, None
    for i in range(n):
        f, g = kh.reference_factors(cell, klist, net_kw, params, x[i:i + 1])[:2]
        fsum = f if fsum is None else [(A0 + A, G0 + G) for (A0, G0), (A, G) in zip(fsum, f)]
        gsum = g if gsum is None else _tree_sum([gsum, g], (1.0, 1.0))
        if i + 1 in BATCHES[name]:
            sums[i + 1] = (fsum, gsum)
    return x, sums


def reference(name, batch):
    """(walkers, factors, gradient tree) of the first `batch` walkers of `per_walker`: the factors are means over the walkers
    (A_b and G_b of one walker are already divided by R), the seed gradient is a sum.  No two walkers of a batch are alike, so
    every tile, every split of the tiles over waves and every group of the contraction carries its own data."""
    x, sums = per_walker(name)
    fsum, gsum = sums[batch]
    return x[:batch], [(A / batch, G / batch) for A, G in fsum], gsum


def _tree_sum(trees, weights):
    t0 = trees[0]
    if isinstance(t0, dict):
        return {k: _tree_sum([t[k] for t in trees], weights) for k in t0}
    if isinstance(t0, (list, tuple)):
        return [_tree_sum([t[i] for t in trees], weights) for i in range(len(t0))]
    return sum(float(w) * t for w, t in zip(weights, trees))


def factor_devs(got, ref):
    """Per factor: max |got - ref| / max |ref|."""
    out = []
    for (A, G), (Ar, Gr) in zip(got, ref):
        for a, r in ((A, Ar), (G, Gr)):
            a, r = a.double().cpu(), r.double()
            assert a.shape == r.shape, (a.shape, r.shape)
            out.append(float((a - r).abs().max() / max(float(r.abs().max()), 1e-300)))
    return out


@pytest.mark.parametrize('name,batch', FACTOR_CASES)
def test_factors_and_seed_gradient_vs_restatement(name, batch, record_property):
    """A and G of every tagged layer and the packed gradient of the seed against tests/kfac_helpers.py: 1e-9 of each factor's
    (each leaf's) largest entry, exact symmetry, and the layout `ds_kfac_layout` reports against the shapes the restatement
    derives from the parameter tree.
    Every walker of a batch is distinct (`reference`), so a tile read twice, a tile skipped or a wrong tile stride shows.
    The worst deviations are printed and recorded per case as the properties factor_dev / grad_dev.  Measured on an MI355X:
    at most 3.3e-12 (factors) and 1.8e-12 (seed gradient), both on diamond at B = 83; per group of cases in the module docstring."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    x, ref, gref = reference(name, batch)
    dp = dev_params(params)
    got, flat = sysd.kfac_factors(dp, torch.as_tensor(x, device='cuda'))
    layout = sysd.kfac_layout()
    shapes = kh.block_shapes(params, cell.nelec)
    assert [(b['kind'], b['index'], b['has_bias'], b['d_in'], b['d_out'], b['repeats']) for b in layout] == [tuple(s) for s in shapes]
    off = 0
    for b in layout:                                   # A then G of every block, densely packed
        assert b['a_offset'] == off and b['g_offset'] == off + b['d_in'] ** 2
        off = b['g_offset'] + b['d_out'] ** 2
        assert all(0 <= i < len(sysd.blocks) for i in b['param_blocks'])
    for A, G in got:
        assert torch.equal(A, A.T) and torch.equal(G, G.T)
    devs = factor_devs(got, ref)
    gd = leaf_devs(sysd.unpack_grad(flat, dp), gref)
    record_property('factor_dev', max(devs))
    record_property('grad_dev', max(gd))
    print(f'{name} B={batch}: worst factor deviation {max(devs):.3e}, worst seed-gradient deviation {max(gd):.3e}')
    assert max(devs) <= 1e-9, devs
    assert max(gd) <= 1e-9, gd


@functools.lru_cache(maxsize=None)
def weighted_reference(name, B, n, seed):
    """A batch of B walkers drawn with repetition from n distinct synthetic ones, and its restatement without B restatement
    calls: -> (walkers (B, 3N), factors, gradient tree, counts).  The factors of a batch are the mean over its walkers of each
    walker's own factors and the seed gradient is the sum of each walker's own, so with count_i occurrences of walker i the
    factor is sum_i count_i F_i / B and the gradient sum_i count_i g_i.  A group, an electron tile or a 5-walker pair tile
    that is dropped or counted twice changes some count by one."""
    fx, cell, klist, net_kw, params = load_case(name)
    xs = systems.synthetic_walkers(cell, n, seed=31)
    assert len(np.unique(xs.round(12), axis=0)) == n
    idx = np.random.default_rng(seed).integers(0, n, B)
    counts = np.bincount(idx, minlength=n)
    assert counts.min() >= 1 and counts.min() != counts.max()
    fsum, gsum = None, None
    for i in range(n):
        f, g = kh.reference_factors(cell, klist, net_kw, params, xs[i:i + 1])[:2]
        w = float(counts[i])
        f = [(w * A, w * G) for A, G in f]
        fsum = f if fsum is None else [(A0 + A, G0 + G) for (A0, G0), (A, G) in zip(fsum, f)]
        gsum = _tree_sum([g], (w,)) if gsum is None else _tree_sum([gsum, g], (1.0, w))
    return xs[idx], [(A / B, G / B) for A, G in fsum], gsum, counts


def flat_devs(sysd, flat, other):
    """Per factor: max |flat - other| / max |other| of two flat factor buffers of one system."""
    return [float((u - v).abs().max() / max(float(v.abs().max()), 1e-300))
            for a, b in zip(sysd.kfac_views(flat), sysd.kfac_views(other)) for u, v in zip(a, b)]


@pytest.mark.parametrize('name,B', I8_FACTOR_CASES)
def test_factors_on_int8_value_chain_at_production_batches(name, B, monkeypatch, record_property):
    """With 512 or more (80-walker group, electron) tiles the value chain of `ds_kfac_factors` runs the residual hidden layers as
    the int8 split; A is built from those activations and the sweep reconstructs tanh(z) from them.  The batch is I8_DISTINCT
    distinct synthetic walkers drawn with repetition (`weighted_reference`), so the restatement costs 29 calls, not B.
      a. factors and seed gradient of the default (int8) system and of a DS_NO_I8_VAL=1 (float64 layers) system against the
         restatement: 1e-9 of each factor's / leaf's largest entry, exact symmetry;
      b. the two systems' flat factor buffers differ in at least one bit (the int8 path ran);
      c. two calls on the int8 system are bit-identical;
      d. passes of k groups (a capped workspace; some passes fall below 512 tiles and run float64 layers) against the one-pass
         result: 1e-9 of each factor's scale and of the seed gradient's.
    Measured on an MI355X (bcc-Li / graphene / diamond): (a) int8 2.1e-12 / 3.6e-11 / 7.4e-11, float64 layers 6.1e-14 / 4.3e-12 /
    4.2e-12; (d) 1.5e-13 / 9.9e-13 / 7.7e-11.  One miscounted walker would move a factor by about 1e-6 of its scale."""
    fx, cell, klist, net_kw, params = load_case(name)
    dp = dev_params(params)
    N, PV = sum(cell.nelec), 80
    ng = (B + PV - 1) // PV
    assert ng * N >= 512 and B % PV != 0
    x, ref, gref, counts = weighted_reference(name, B, I8_DISTINCT, 13)
    x = torch.as_tensor(x, device='cuda')
    monkeypatch.delenv('DS_NO_I8_VAL', raising=False)
    monkeypatch.delenv('DS_I8_VAL_MIN_TILES', raising=False)
    s_i8 = fresh_system(cell, klist, net_kw)
    monkeypatch.setenv('DS_NO_I8_VAL', '1')
    s_64 = fresh_system(cell, klist, net_kw)
    monkeypatch.delenv('DS_NO_I8_VAL')
    f8, g8 = s_i8.kfac_factors(dp, x, flat=True)
    f64, g64 = s_64.kfac_factors(dp, x, flat=True)
    # (a)
    worst = {}
    for tag, sysd, f, g in (('a_int8_vs_restatement', s_i8, f8, g8), ('a_float64_vs_restatement', s_64, f64, g64)):
        views = sysd.kfac_views(f)
        for A, G in views:
            assert torch.equal(A, A.T) and torch.equal(G, G.T)
        devs = factor_devs(views, ref)
        gd = leaf_devs(sysd.unpack_grad(g, dp), gref)
        worst[tag] = (max(devs), max(gd))
        record_property(tag, max(devs))
        record_property(tag + '_grad', max(gd))
        print(f'{name} B={B} {tag}: worst factor deviation {max(devs):.3e}, worst seed-gradient deviation {max(gd):.3e}')
    for tag, (d, gd) in worst.items():
        assert d <= 1e-9 and gd <= 1e-9, (tag, d, gd)
    # (b)
    assert not torch.equal(f8, f64)
    # (c)
    f8b, g8b = s_i8.kfac_factors(dp, x, flat=True)
    assert torch.equal(f8, f8b) and torch.equal(g8, g8b)
    # (d) passes of k groups: bcc-Li 22 (528 int8 tiles, then 2 float64 groups), graphene 11 (528, then 1), diamond 5 (480 and 96:
    # float64 only)
    k = min(-(-512 // N), ng - 1)
    assert (ng % k) * N < 512
    cap = int(s_i8.lib.ds_kfac_workspace_bytes(s_i8.handle, k * PV))
    assert cap < int(s_i8.lib.ds_kfac_workspace_bytes(s_i8.handle, B))
    fc, gc = s_i8.kfac_factors(dp, x, flat=True, max_bytes=cap)
    devs = flat_devs(s_i8, fc, f8)
    gd = float((gc - g8).abs().max() / g8.abs().max())
    record_property('d_chunked_vs_one_pass', max(devs))
    record_property('d_chunked_vs_one_pass_grad', gd)
    print(f'{name} B={B} d_chunked_vs_one_pass: factors {max(devs):.3e}, seed gradient {gd:.3e}')
    assert max(devs) <= 1e-9 and gd <= 1e-9, (devs, gd)


@pytest.mark.parametrize('name,batch', TINY_I8_CASES)
def test_factors_int8_value_chain_on_tiny_batches(name, batch, monkeypatch, record_property):
    """DS_I8_VAL_MIN_TILES=1: the int8 split runs the hidden layers of the factor pass's value chain for one 80-walker group that
    is mostly padding, with fewer tiles (4 / 24 / 48) than CUs in the persistent grid.  All walkers distinct (`reference`);
    factors and seed gradient against the restatement at 1e-9; the factors differ in at least one bit from the default system's
    float64 layers (the int8 path ran).
    Measured on an MI355X (lih / bcc-Li / graphene): factors 2.1e-12 / 2.3e-12 / 8.8e-12, seed gradient 2.7e-12 / 2.4e-12 / 5.2e-12."""
    fx, cell, klist, net_kw, params = load_case(name)
    dp = dev_params(params)
    x, ref, gref = reference(name, batch)
    x = torch.as_tensor(x, device='cuda')
    monkeypatch.delenv('DS_NO_I8_VAL', raising=False)
    monkeypatch.setenv('DS_I8_VAL_MIN_TILES', '1')
    s_i8 = fresh_system(cell, klist, net_kw)
    monkeypatch.delenv('DS_I8_VAL_MIN_TILES')
    s_64 = fresh_system(cell, klist, net_kw)
    f8, g8 = s_i8.kfac_factors(dp, x, flat=True)
    f64, _ = s_64.kfac_factors(dp, x, flat=True)
    assert not torch.equal(f8, f64)
    views = s_i8.kfac_views(f8)
    for A, G in views:
        assert torch.equal(A, A.T) and torch.equal(G, G.T)
    devs = factor_devs(views, ref)
    gd = leaf_devs(s_i8.unpack_grad(g8, dp), gref)
    record_property('factor_dev', max(devs))
    record_property('grad_dev', max(gd))
    print(f'{name} B={batch} forced int8: worst factor deviation {max(devs):.3e}, worst seed-gradient deviation {max(gd):.3e}')
    assert max(devs) <= 1e-9, devs
    assert max(gd) <= 1e-9, gd


@pytest.mark.parametrize('name,batch', F32_CASES)
def test_factors_float32(name, batch, record_property):
    """float32 system against the float64 restatement at the float32-rounded walkers: per factor 3x what the restatement's own
    float32 run loses (`common.float32_tolerance`).  `lih` B = 5, `bcc_li` B = 5 and `diamond` B = 2, where the restatement's own
    loss ranges over three decades between the factors (4e-7 ... 3e-4).  The kernel's deviation, the restatement's loss and the
    budget are recorded per factor.  Measured on an MI355X, worst factor against its budget: 3.1e-5 of 5.1e-5 (lih), 4.3e-5 of
    9.0e-5 (bcc-Li), 3.7e-4 of 7.7e-4 (diamond)."""
    fx, cell, klist, net_kw, params = load_case(name)
    x, _, _ = reference(name, batch)
    x32 = x.astype(np.float32)
    ref64, _, _ = kh.reference_factors(cell, klist, net_kw, params, x32.astype(np.float64))
    ref32, _, _ = kh.reference_factors(cell, klist, net_kw, params, x32.astype(np.float64), dtype=torch.float32)
    loss = factor_devs(ref32, ref64)
    sysd = fresh_system(cell, klist, net_kw, torch.float32)
    got, _ = sysd.kfac_factors(dev_params(params, torch.float32), torch.as_tensor(x32, device='cuda'))
    for A, G in got:
        assert torch.equal(A, A.T) and torch.equal(G, G.T)
    devs = factor_devs(got, ref64)
    record_property('factor_dev_f32', max(devs))
    record_property('factor_dev_f32_per_factor', devs)
    record_property('restatement_f32_loss_per_factor', loss)
    record_property('f32_budget_per_factor', [float32_tolerance(loss, i) for i in range(len(loss))])
    print(f'{name} B={batch} float32 deviations', devs, 'oracle float32 loss', loss)
    for i, d in enumerate(devs):
        assert d <= float32_tolerance(loss, i), (i, d, loss[i])


def test_full_envelope_is_refused():
    fx, cell, klist, net_kw, params = load_case('lih_fullenv')
    sysd = system_for(cell, klist, net_kw)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 2, seed=3), device='cuda')
    with pytest.raises(NotImplementedError, match='qmc1'):
        sysd.kfac_factors(dev_params(params), x)


def test_two_calls_same_bits_chunks_agree_and_empty_batch():
    """Two calls give identical bits; a workspace cap that forces more than one chunk agrees with the unchunked call to 1e-12
    of each factor's scale; B = 0 gives zeros."""
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 163, seed=17), device='cuda')        # three groups, the last ragged
    a, ga = sysd.kfac_factors(dp, x)
    a = [(A.clone(), G.clone()) for A, G in a]
    b, gb = sysd.kfac_factors(dp, x)
    assert torch.equal(ga, gb)
    for (A, G), (A2, G2) in zip(a, b):
        assert torch.equal(A, A2) and torch.equal(G, G2)
    need = int(sysd.lib.ds_kfac_workspace_bytes(sysd.handle, 163))
    one = int(sysd.lib.ds_kfac_workspace_bytes(sysd.handle, 1))
    assert one < need                                   # a one-group workspace: three chunks
    c, gc = sysd.kfac_factors(dp, x, max_bytes=one)
    for (A, G), (A2, G2) in zip(a, c):
        for u, v in ((A, A2), (G, G2)):
            assert float((u - v).abs().max()) <= 1e-12 * float(u.abs().max())
    assert float((ga - gc).abs().max()) <= 1e-12 * float(ga.abs().max())
    z, gz = sysd.kfac_factors(dp, x[:0])
    assert float(gz.abs().max()) == 0.0 and all(float(A.abs().max()) == 0.0 and float(G.abs().max()) == 0.0 for A, G in z)
