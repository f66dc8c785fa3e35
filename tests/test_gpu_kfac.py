"""GPU tests of the KFAC factor pass `ds_kfac_factors` (csrc/ds_kfac.h) through the C ABI, against the torch restatement of
tests/kfac_helpers.py (activations captured in the oracle's forward, dy from torch.autograd of sum_b sqrt2 log|psi_b|).

The placement of the blocks and the seed are pinned by that restatement only (the reference's jaxpr tracer cannot run outside
JAX); the arithmetic on them -- which rows, which order, which divisor -- is what these tests hold the kernels to.
Bound (float64): every factor within 1e-9 of its largest entry, the bound test_vjp_vs_oracle_autograd holds the same sweep to;
symmetry exact.  The deviations measured are recorded as test properties."""
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
                ('bcc_li_fulldet', 3), ('lih_diagenv', 3), ('lih_det3', 3), ('graphene', 2)]


MAX_BATCH = {}
for _name, _batch in FACTOR_CASES:
    MAX_BATCH[_name] = max(MAX_BATCH.get(_name, 0), _batch)


@functools.lru_cache(maxsize=None)
def per_walker(name):
    """The largest batch of a case -- all walkers distinct -- and the restatement's (factors, gradient tree) of each walker
    ALONE, computed once per case and shared by its batch sizes."""
    fx, cell, klist, net_kw, params = load_case(name)
    n = MAX_BATCH[name]
    x = systems.synthetic_walkers(cell, n, seed=91)
    assert len(np.unique(x.round(12), axis=0)) == n
    return x, [kh.reference_factors(cell, klist, net_kw, params, x[i:i + 1])[:2] for i in range(n)]


def reference(name, batch):
    """(walkers, factors, gradient tree) of the first `batch` walkers of `per_walker`: the factors are means over the walkers
    (A_b and G_b of one walker are already divided by R), the seed gradient is a sum.  No two walkers of a batch are alike, so
    every tile, every split of the tiles over waves and every group of the contraction carries its own data."""
    x, per = per_walker(name)
    per = per[:batch]
    ones = [1.0] * batch
    nb = len(per[0][0])
    factors = [tuple(sum(p[0][b][j] for p in per) / batch for j in range(2)) for b in range(nb)]
    return x[:batch], factors, _tree_sum([p[1] for p in per], ones)


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
    unmeasured (this test has not yet run on one; the figures belong here once it has)."""
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


def test_factors_float32(record_property):
    """float32 system on `lih`, B = 5, against the float64 restatement at the float32-rounded walkers: per factor 3x what the
    restatement's own float32 run loses (`common.float32_tolerance`)."""
    name, batch = 'lih', 5
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
    print('float32 deviations', devs, 'oracle float32 loss', loss)
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
