"""GPU parity of the parameter gradient (reference train.py:91-142):
`ds_logpsi_vjp` through the C ABI against (1) torch autograd over the CPU oracle and (2) finite
differences of the REFERENCE-executed forward stored in tests/golden (gradfd_*).

Tolerances (float64): 1e-9 relative to the largest entry of each parameter leaf against the oracle;
against the reference finite differences the fixtures' own truncation error (2e-7 absolute).  float32 against the
float64 oracle: per leaf 3x what the oracle's own float32 run loses (`common.float32_tolerance`).
The deviations the new tests measure are recorded as test properties (`--junitxml`, junit_family=legacy)."""
import numpy as np
import pytest
import torch

from oracle import train as otrain
from oracle.testing import make_test_direction

from common import float32_tolerance, load_case, oracle_net
from deepsolid_amd import systems

pytestmark = pytest.mark.gpu


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(np.asarray(vv), dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v]
            for k, v in params.items()}


def system_for(cell, klist, net_kw, dtype=torch.float64):
    from deepsolid_amd.device import DeviceSystem
    return DeviceSystem.for_network(cell, klist, net_kw, dtype)


def leaves(tree):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from leaves(tree[k])
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            yield from leaves(v)
    else:
        yield tree


def tree_dot(tree, direction):
    return sum(float((a.double().cpu() * torch.as_tensor(np.asarray(d))).sum()) for a, d in zip(leaves(tree), leaves(direction)))


def assert_tree_close(got, ref, rtol):
    for g, r in zip(leaves(got), leaves(ref)):
        g = g.double().cpu().numpy()
        r = r.detach().numpy() if isinstance(r, torch.Tensor) else np.asarray(r)
        assert g.shape == r.shape
        scale = max(np.abs(r).max(), 1e-12)
        assert np.abs(g - r).max() <= rtol * scale, (g.shape, np.abs(g - r).max(), scale)


def leaf_devs(got, ref):
    """Per leaf: max |got - ref| / max |ref| (the measure `assert_tree_close` bounds)."""
    out = []
    for g, r in zip(leaves(got), leaves(ref)):
        g = g.double().cpu().numpy()
        r = r.detach().double().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r, dtype=np.float64)
        assert g.shape == r.shape
        out.append(float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-12)))
    return out


def fresh_system(cell, klist, net_kw, dtype=torch.float64):
    """A new `DeviceSystem` (not the per-cell cache of `system_for`): the DS_ switches are read when it is created."""
    from deepsolid_amd.device import DeviceSystem
    from deepsolid_amd.ewaldsum import EwaldTables
    return DeviceSystem(cell, klist, net_kw, EwaldTables(cell), dtype)


def oracle_vjp(cell, klist, net_kw, params, x, cot, dtype=None):
    """oracle.train.logpsi_vjp at walkers x (B, 3N) with cotangents cot (B, 2) (numpy or torch, any device)."""
    from oracle.network import working_dtype
    x = torch.as_tensor(x).detach().cpu().double()
    cot = torch.as_tensor(cot).detach().cpu().double()
    cc = torch.complex(cot[:, 0].contiguous(), cot[:, 1].contiguous())
    if dtype is None:
        return otrain.logpsi_vjp(oracle_net(cell, klist, net_kw, 'eval_logdet').apply, params, x, cc)
    with working_dtype(dtype):
        net = oracle_net(cell, klist, net_kw, 'eval_logdet')
    return otrain.logpsi_vjp(net.apply, params, x, cc, dtype=dtype)


@pytest.mark.parametrize('name,batch', [('h2', 5), ('lih', 7), ('lih_twist', 4), ('lih_2x1x1', 3), ('bcc_li', 5),
                                        ('lih_fulldet', 4), ('lih_tri', 4), ('lih_bias', 4), ('lih_diagenv', 4), ('lih_fullenv', 4), ('lih_lastlayer', 4),
                                        ('lih_fn_defaults', 3), ('bcc_li_fulldet', 2), ('graphene', 2)])
def test_vjp_vs_oracle_autograd(name, batch):
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    x = systems.synthetic_walkers(cell, batch, seed=77)
    cot = np.random.default_rng(5).normal(size=(batch, 2))
    dp = dev_params(params)
    flat, la, ph = sysd.logpsi_vjp(dp, torch.as_tensor(x, device='cuda'), torch.as_tensor(cot, device='cuda'))
    got = sysd.unpack_grad(flat, dp)
    net = oracle_net(cell, klist, net_kw, 'eval_logdet')
    cc = torch.complex(torch.as_tensor(cot[:, 0]), torch.as_tensor(cot[:, 1]))
    ref = otrain.logpsi_vjp(net.apply, params, torch.as_tensor(x), cc)
    assert_tree_close(got, ref, 1e-9)
    from oracle.network import params_to_torch
    pt = params_to_torch(params)
    lp = torch.stack([net.apply(pt, torch.as_tensor(xx)) for xx in x])
    assert float((la.cpu() - lp.real).abs().max()) < 1e-10
    assert float((torch.angle(ph.cpu() * torch.exp(-1j * lp.imag))).abs().max()) < 1e-10


LARGE_VJP_CASES = ['bcc_li_twist',      # twisted 24-electron cell: complex k-points in the envelope phase
                   'bcc_li_bcc',        # 24 electrons, bcc symmetry lattice in the input features
                   'bcc_li_333',        # odd N = 81: 41 / 40 spins, unequal determinants, NP = 6561 pairs
                   'diamond',           # 96 electrons, 48 x 48 determinants
                   'graphene_331']      # 108 electrons, 54 x 54 determinants through k_det_inverse


@pytest.mark.parametrize('name', LARGE_VJP_CASES)
def test_vjp_large_and_untested_cells_vs_oracle_autograd(name, record_property):
    """`ds_logpsi_vjp` on the cells the reverse sweep had never been compared on, against torch autograd over the oracle
    (1e-9 of each leaf's largest entry), one call over the fixture walkers followed by 2 synthetic walkers:
      bcc_li_twist -- a twisted cell (complex k-points: the phase factors of the envelope and of the orbital head);
      bcc_li_bcc   -- bcc symmetry lattice in the input features;
      bcc_li_333   -- odd N = 81: 41 / 40 spins (determinant channels of unequal size) and NP = 6561 pairs, not a multiple of
                      16 (a partial pair tile in k_two_bwd / k_outer_gemm);
      diamond      -- 96 electrons: 48 x 48 determinants, more electrons than a 64-lane wave;
      graphene_331 -- 108 electrons: 54 x 54 determinants through k_det_inverse.
    log|psi| and the phase the call returns on the fixture walkers hold the REFERENCE-executed values (1e-9).
    Measured on the MI355X: gradient at most 3.0e-12 of a leaf's largest entry (diamond; bcc_li_333 4.3e-13, graphene_331 1.4e-12),
    log|psi| / phase within 2.2e-12 of the fixtures."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = fresh_system(cell, klist, net_kw)
    nfx = len(fx['x'])
    x = np.concatenate([fx['x'], systems.synthetic_walkers(cell, 2, seed=77)])
    cot = np.random.default_rng(5).normal(size=(len(x), 2))
    dp = dev_params(params)
    flat, la, ph = sysd.logpsi_vjp(dp, torch.as_tensor(x, device='cuda'), torch.as_tensor(cot, device='cuda'))
    devs = leaf_devs(sysd.unpack_grad(flat, dp), oracle_vjp(cell, klist, net_kw, params, x, cot))
    record_property('max_leaf_dev', max(devs))
    assert max(devs) <= 1e-9, devs
    la, ph = la.cpu().numpy(), ph.cpu().numpy()
    record_property('logabs_dev', float(np.abs(la[:nfx] - fx['logabs']).max()))
    record_property('phase_dev', float(np.abs(ph[:nfx] - fx['phase']).max()))
    np.testing.assert_allclose(la[:nfx], fx['logabs'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ph[:nfx], fx['phase'], rtol=0, atol=1e-9)
    assert np.isfinite(la).all()


I8_VJP_CASES = [('bcc_li', 1843),       # 24 groups x 24 electrons = 576 tiles, last group 3 walkers
                ('graphene', 903),      # 12 groups x 48 electrons = 576 tiles, last group 23 walkers
                ('diamond', 403)]       # 6 groups x 96 electrons = 576 tiles, last group 3 walkers


@pytest.mark.parametrize('name,B', I8_VJP_CASES)
def test_vjp_on_int8_value_chain_at_production_batches(name, B, monkeypatch, record_property):
    """With 512 or more (80-walker group, electron) tiles the VJP's forward (run_value_chain) runs the residual 320 -> 256
    hidden layers as the int8 split (i8::k_layer_i8<5, 4>) and the reverse sweep reads those activations back
    (k_layer_bwd_prep<true>: tanh(z) = sqrt2 out - in).  The batch is the fixture walkers, then synthetic ones.
      a. against the same VJP with DS_NO_I8_VAL=1 (float64 MFMA layers): every leaf within 1e-9 of its largest entry, and
         log|psi| differs in at least one bit (the int8 path ran);
      b. a cotangent that is zero except on 6 walkers (a fixture walker, 79 / 80 across the first group boundary, one mid-batch,
         the last two in the ragged group), run over the FULL batch so the int8 path stays on, against the oracle on those 6
         walkers: 1e-9;
      c. two calls are bit-identical (fixed reduction order; the int8 kernel's LDS column maxima do not depend on order);
      d. passes of few groups (a workspace smaller than the batch): some passes fall below 512 tiles and run in float64;
         the result agrees with the one-pass result within (a)'s tolerance.
    Measured on the MI355X (bcc-Li / graphene / diamond, of a leaf's largest entry): (a) 2.5e-11 / 3.4e-11 / 8.7e-11;
    (b) 8.0e-12 / 2.5e-11 / 3.9e-11; (d) 1.5e-12 / 8.4e-13 / 8.7e-11 (diamond's passes are all float64: (d) is (a) there)."""
    fx, cell, klist, net_kw, params = load_case(name)
    dp = dev_params(params)
    nfx = len(fx['x'])
    x = torch.as_tensor(np.concatenate([fx['x'], systems.synthetic_walkers(cell, B - nfx, seed=31)]), device='cuda')
    cot = torch.as_tensor(np.random.default_rng(13).normal(size=(B, 2)), device='cuda')
    N, PV = sum(cell.nelec), 80
    ng = (B + PV - 1) // PV
    assert ng * N >= 512 and B % PV != 0
    monkeypatch.delenv('DS_NO_I8_VAL', raising=False)
    monkeypatch.delenv('DS_I8_VAL_MIN_TILES', raising=False)
    s_i8 = fresh_system(cell, klist, net_kw)
    monkeypatch.setenv('DS_NO_I8_VAL', '1')
    s_64 = fresh_system(cell, klist, net_kw)
    monkeypatch.delenv('DS_NO_I8_VAL')
    # the default workspace holds every group: one pass, all ng * N tiles in one forward
    wsb = [int(s_i8.lib.ds_vjp_workspace_bytes(s_i8.handle, k * PV)) for k in (1, 2, ng)]
    assert wsb[2] - wsb[0] == (ng - 1) * (wsb[1] - wsb[0])
    g8, la8, ph8 = s_i8.logpsi_vjp(dp, x, cot)
    g8 = g8.clone()
    g64, la64, ph64 = s_64.logpsi_vjp(dp, x, cot)
    # (a)
    devs = leaf_devs(s_i8.unpack_grad(g8, dp), s_64.unpack_grad(g64, dp))
    record_property('a_int8_vs_float64', max(devs))
    assert max(devs) <= 1e-9, devs
    assert not torch.equal(la8, la64)
    for la, ph in ((la8, ph8), (la64, ph64)):
        np.testing.assert_allclose(la[:nfx].cpu().numpy(), fx['logabs'], rtol=0, atol=1e-9)
        np.testing.assert_allclose(ph[:nfx].cpu().numpy(), fx['phase'], rtol=0, atol=1e-9)
    # (c)
    again, la_again, _ = s_i8.logpsi_vjp(dp, x, cot)
    assert torch.equal(g8, again) and torch.equal(la8, la_again)
    # (b)
    sel = [1, 79, 80, B // 2, B - 2, B - 1]
    cm = torch.zeros_like(cot)
    cm[sel] = cot[sel]
    gm, _, _ = s_i8.logpsi_vjp(dp, x, cm)
    devs = leaf_devs(s_i8.unpack_grad(gm, dp), oracle_vjp(cell, klist, net_kw, params, x[sel], cot[sel]))
    record_property('b_masked_vs_oracle', max(devs))
    assert max(devs) <= 1e-9, devs
    # (d) passes of k groups: bcc-Li 22 (528 int8 tiles, then 2 float64 groups), graphene 11 (528, then 1), diamond 5 (480 and 96:
    # float64 only)
    k = min(-(-512 // N), ng - 1)
    assert (ng % k) * N < 512
    ch, la_ch, _ = s_i8.logpsi_vjp(dp, x, cot, max_bytes=int(s_i8.lib.ds_vjp_workspace_bytes(s_i8.handle, k * PV)))
    devs = leaf_devs(s_i8.unpack_grad(ch, dp), s_i8.unpack_grad(g8, dp))
    record_property('d_chunked_vs_one_pass', max(devs))
    assert max(devs) <= 1e-9, devs
    np.testing.assert_allclose(la_ch.cpu().numpy(), la8.cpu().numpy(), rtol=2e-12, atol=1e-10)


@pytest.mark.parametrize('name,batch', [('lih', 5), ('bcc_li', 3), ('graphene', 1)])
def test_vjp_int8_value_chain_on_tiny_batches(name, batch, monkeypatch, record_property):
    """DS_I8_VAL_MIN_TILES=1: the int8 split runs the residual hidden layers of the VJP's forward even for one 80-walker group
    that is mostly padding, with fewer tiles (4 / 24 / 48) than CUs in the persistent grid.  The gradient against the oracle
    (1e-9 of each leaf's largest entry), log|psi| / phase against the reference-executed fixture values (1e-9), and the result
    differs from the default system's float64 layers (the int8 path ran).
    Measured on the MI355X: gradient 8.9e-13 / 2.2e-12 / 2.4e-11 of a leaf's largest entry (lih / bcc-Li / graphene)."""
    fx, cell, klist, net_kw, params = load_case(name)
    dp = dev_params(params)
    x = fx['x'][:batch]
    cot = np.random.default_rng(6).normal(size=(batch, 2))
    monkeypatch.delenv('DS_NO_I8_VAL', raising=False)
    monkeypatch.setenv('DS_I8_VAL_MIN_TILES', '1')
    s_i8 = fresh_system(cell, klist, net_kw)
    monkeypatch.delenv('DS_I8_VAL_MIN_TILES')
    s_64 = fresh_system(cell, klist, net_kw)
    xd, cd = torch.as_tensor(x, device='cuda'), torch.as_tensor(cot, device='cuda')
    g8, la8, ph8 = s_i8.logpsi_vjp(dp, xd, cd)
    g8 = g8.clone()
    g64, la64, _ = s_64.logpsi_vjp(dp, xd, cd)
    assert not (torch.equal(g8, g64) and torch.equal(la8, la64))
    devs = leaf_devs(s_i8.unpack_grad(g8, dp), oracle_vjp(cell, klist, net_kw, params, x, cot))
    record_property('max_leaf_dev', max(devs))
    assert max(devs) <= 1e-9, devs
    np.testing.assert_allclose(la8.cpu().numpy(), fx['logabs'][:batch], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ph8.cpu().numpy(), fx['phase'][:batch], rtol=0, atol=1e-9)


@pytest.mark.parametrize('name', ['lih', 'lih_twist', 'bcc_li', 'lih_fulldet', 'lih_tri'])
def test_vjp_vs_reference_finite_differences(name):
    """d/dh log psi(theta + h v) at h = 0 from the reference's own forward (tools/make_golden.py)."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    v = make_test_direction(int(fx['gradfd_seed']), params)
    dp = dev_params(params)
    n = len(fx['gradfd_dlogabs'])
    x = torch.as_tensor(fx['x'][:n], device='cuda')
    for b in range(n):
        for cot, key in (((1.0, 0.0), 'gradfd_dlogabs'), ((0.0, 1.0), 'gradfd_darg')):
            c = torch.zeros(n, 2, dtype=torch.float64, device='cuda')
            c[b] = torch.tensor(cot, dtype=torch.float64)
            flat, _, _ = sysd.logpsi_vjp(dp, x, c)
            got = tree_dot(sysd.unpack_grad(flat, dp), v)
            assert abs(got - float(fx[key][b])) < 2e-7 * max(1.0, abs(float(fx[key][b]))), (b, key, got, fx[key][b])


def test_vjp_groups_chunks_and_linearity():
    """Batches that span several 80-walker groups, a ragged tail, several passes (small workspace)."""
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    B = 203
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=3), device='cuda')
    cot = torch.as_tensor(np.random.default_rng(9).normal(size=(B, 2)), device='cuda')
    dp = dev_params(params)
    full, la, _ = sysd.logpsi_vjp(dp, x, cot)
    full = full.clone()
    # the same call again: bit-identical (fixed reduction order, no atomics)
    again, _, _ = sysd.logpsi_vjp(dp, x, cot)
    assert torch.equal(full, again)
    # one group per pass
    one_group = int(sysd.lib.ds_vjp_workspace_bytes(sysd.handle, 1))
    chunked, la2, _ = sysd.logpsi_vjp(dp, x, cot, max_bytes=one_group)
    scale = float(full.abs().max())
    assert float((chunked - full).abs().max()) < 1e-12 * scale
    assert torch.equal(la, la2)
    # linearity in the cotangent / additivity over walkers
    parts = torch.zeros_like(full)
    for lo, hi in ((0, 1), (1, 80), (80, 81), (81, 203)):
        g, _, _ = sysd.logpsi_vjp(dp, x[lo:hi], cot[lo:hi])
        parts += g
    assert float((parts - full).abs().max()) < 1e-12 * scale
    # against the oracle on a subset that crosses a group boundary
    sel = slice(70, 90)
    g, _, _ = sysd.logpsi_vjp(dp, x[sel], cot[sel])
    net = oracle_net(cell, klist, net_kw, 'eval_logdet')
    ref = otrain.logpsi_vjp(net.apply, params, x[sel].cpu(), torch.view_as_complex(cot[sel].cpu().contiguous()))
    assert_tree_close(sysd.unpack_grad(g, dp), ref, 1e-9)


def test_vjp_zero_cotangent_and_empty_batch():
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    x = torch.as_tensor(fx['x'], device='cuda')
    g, _, _ = sysd.logpsi_vjp(dp, x, torch.zeros(x.shape[0], 2, dtype=torch.float64, device='cuda'))
    assert float(g.abs().max()) == 0.0
    g, la, ph = sysd.logpsi_vjp(dp, x[:0], torch.zeros(0, 2, dtype=torch.float64, device='cuda'))
    assert g.shape == (sysd.param_count,) and float(g.abs().max()) == 0.0 and la.shape == (0,)


def test_vjp_float32():
    fx, cell, klist, net_kw, params = load_case('lih')
    s64, s32 = system_for(cell, klist, net_kw), system_for(cell, klist, net_kw, torch.float32)
    x = systems.synthetic_walkers(cell, 90, seed=8)
    cot = np.random.default_rng(2).normal(size=(90, 2))
    p64, p32 = dev_params(params), dev_params(params, torch.float32)
    g64, _, _ = s64.logpsi_vjp(p64, torch.as_tensor(x, device='cuda'), torch.as_tensor(cot, device='cuda'))
    g32, _, _ = s32.logpsi_vjp(p32, torch.as_tensor(x, dtype=torch.float32, device='cuda'),
                               torch.as_tensor(cot, dtype=torch.float32, device='cuda'))
    t64, t32 = s64.unpack_grad(g64, p64), s32.unpack_grad(g32, p32)
    for a, b in zip(leaves(t64), leaves(t32)):
        assert float((a - b.double()).abs().max()) < 2e-3 * max(1.0, float(a.abs().max()))


@pytest.mark.parametrize('name', ['bcc_li', 'diamond'])
def test_vjp_float32_vs_float64_oracle_with_budget(name, record_property):
    """The float32 VJP against the float64 oracle at the float32-ROUNDED fixture walkers and cotangents.  Per leaf the bound is
    `common.float32_tolerance` over the leaves: 3x what the oracle's own float32 VJP (oracle.train.logpsi_vjp(dtype=float32),
    float32-rounded parameters) loses on that leaf -- or 3x its mean over the leaves where that run lands close -- + 1e-6,
    everything relative to the leaf's largest float64 entry.
    Measured on the MI355X: bcc-Li at most 0.51x, diamond at most 0.59x of the bound (worst leaf deviation 1.7e-5 / 8.3e-4)."""
    fx, cell, klist, net_kw, params = load_case(name)
    s32 = fresh_system(cell, klist, net_kw, torch.float32)
    x32 = torch.as_tensor(fx['x'], dtype=torch.float32)
    c32 = torch.as_tensor(np.random.default_rng(4).normal(size=(len(x32), 2)), dtype=torch.float32)
    p32 = dev_params(params, torch.float32)
    g, la, _ = s32.logpsi_vjp(p32, x32.cuda(), c32.cuda())
    assert g.dtype == torch.float32
    got = s32.unpack_grad(g, p32)
    ref = oracle_vjp(cell, klist, net_kw, params, x32.double(), c32.double())
    own = oracle_vjp(cell, klist, net_kw, params, x32, c32, dtype=torch.float32)
    assert all(t.dtype == torch.float32 for t in leaves(own))
    loss = leaf_devs(own, ref)
    devs = leaf_devs(got, ref)
    ratio = [d / float32_tolerance(loss, i) for i, d in enumerate(devs)]
    record_property('max_leaf_dev', max(devs))
    record_property('max_ratio_to_bound', max(ratio))
    assert max(ratio) <= 1.0, list(zip(devs, loss))
    np.testing.assert_allclose(la.double().cpu().numpy(), fx['logabs'], rtol=0, atol=2e-3)


def test_energy_gradient_at_a_production_batch(monkeypatch, record_property):
    """`make_loss(...).value_and_grad` on 1843 bcc-Li walkers (24 groups x 24 electrons = 576 tiles: the VJP's forward on the
    int8 split) with real clipping at 5.0 -- the step the training loop runs at scale.  The gradient equals `logpsi_vjp` with the
    cotangent rebuilt on the host from aux.local_energy by the reference formula (train.py:91-142 as oracle/train.py states it:
    clip(E_L - mean Re E_L) / B) to 1e-12 of each leaf's largest entry; loss and variance equal numpy on aux.local_energy to
    1e-12 relative.  Measured on the MI355X: gradient 4.6e-15 of a leaf's largest entry; loss and variance bit-equal."""
    from deepsolid_amd import network as dnet, train as dtrain
    monkeypatch.delenv('DS_NO_I8_VAL', raising=False)
    monkeypatch.delenv('DS_I8_VAL_MIN_TILES', raising=False)
    fx, cell, klist, net_kw, params = load_case('bcc_li')
    B = 1843
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type='real')
    dp = dev_params(params)
    x = torch.as_tensor(np.concatenate([fx['x'], systems.synthetic_walkers(cell, B - len(fx['x']), seed=41)]), device='cuda')
    (loss, aux), grads = loss_fn.value_and_grad(dp, x)
    e_l = aux.local_energy.detach().cpu().to(torch.complex128)
    assert bool(torch.isfinite(torch.view_as_real(e_l)).all())
    el = e_l.numpy()
    mean = el.mean()
    loss_np, var_np = mean.real, (np.abs(el) ** 2).mean() - abs(mean.real) ** 2
    record_property('loss_dev', abs(float(loss) - loss_np) / max(1.0, abs(loss_np)))
    record_property('variance_dev', abs(float(aux.variance) - var_np) / max(1.0, var_np))
    assert abs(float(loss) - loss_np) <= 1e-12 * max(1.0, abs(loss_np))
    assert abs(float(aux.variance) - var_np) <= 1e-12 * max(1.0, var_np)
    diff = e_l - e_l.mean().real
    clipped = otrain.clip_difference(diff, 5.0, 'real')
    assert int((clipped != diff).sum()) > 0             # the clip is active
    cot = torch.view_as_real(clipped / B).contiguous()
    system = loss_fn.system
    flat, _, _ = system.logpsi_vjp(dp, x, cot.cuda())
    devs = leaf_devs(grads, system.unpack_grad(flat, dp))
    record_property('max_leaf_dev', max(devs))
    assert max(devs) <= 1e-12, devs


@pytest.mark.parametrize('clip_type,clip', [('real', 5.0), ('real', 0.5), ('complex', 0.7), ('real', 0.0)])
def test_energy_gradient_vs_oracle(clip_type, clip):
    """total_energy.value_and_grad == jax.value_and_grad(total_energy) through the custom JVP (train.py:91-142)."""
    from deepsolid_amd import network as dnet, train as dtrain
    fx, cell, klist, net_kw, params = load_case('lih')
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=clip, clip_type=clip_type)
    dp = dev_params(params)
    x = torch.as_tensor(fx['x'], device='cuda')
    (loss, aux), grads = loss_fn.value_and_grad(dp, x)
    onet_ = oracle_net(cell, klist, net_kw, 'eval_logdet')
    oloss = otrain.make_loss(onet_.apply, cell, mode='hessian', clip_local_energy=clip, clip_type=clip_type)
    (l_ref, aux_ref), g_ref = oloss.value_and_grad(params, torch.as_tensor(fx['x']))
    assert abs(float(loss) - float(l_ref)) < 1e-8
    assert float((aux.local_energy.cpu() - aux_ref.local_energy).abs().max()) < 1e-8
    assert_tree_close(grads, g_ref, 1e-7)


@pytest.mark.parametrize('hidden_dims,use_last', [(((40, 10), (56, 12), (56, 12)), False), (((100, 20), (100, 20)), True),
                                                  (((64, 20), (64, 24), (64, 24)), False)])
def test_hidden_widths_without_kernel_instances(hidden_dims, use_last):
    """Widths the kernels have no instance for (one-electron widths that are not multiples of 64, pair widths other than 16 / 32)
    run with zero-padded weights (the library's own plan: ds_device_widths, deepsolid_amd/device.py::device_plan): exact, because a
    padded feature is tanh(0) = 0 in every layer.  The residual connections follow the REFERENCE widths (network.py:525-528) through
    explicit flags: 40 -> 56 has none although both pad to 64, 56 -> 56 has one; 10 -> 12 has none (both 16), 12 -> 12 has one;
    20 -> 24 has none although both run the 32-wide pair kernels (refused until round 5).  Loss, local energies and the energy
    gradient -- mapped back to the reference's parameter shapes -- against the oracle."""
    from deepsolid_amd import network as dnet, train as dtrain
    from oracle.testing import make_test_params
    cell, klist = systems.build('lih')
    net_kw = dict(systems.DETNET_DEFAULTS, hidden_dims=hidden_dims, use_last_layer=use_last)
    params = make_test_params(17, cell.original_cell.atom_coords(), cell.nelec, net_kw)
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type='real')
    dp = dev_params(params)
    xn = systems.synthetic_walkers(cell, 5, seed=21)
    (loss, aux), grads = loss_fn.value_and_grad(dp, torch.as_tensor(xn, device='cuda'))
    onet_ = oracle_net(cell, klist, net_kw, 'eval_logdet')
    oloss = otrain.make_loss(onet_.apply, cell, mode='hessian', clip_local_energy=5.0, clip_type='real')
    (l_ref, aux_ref), g_ref = oloss.value_and_grad(params, torch.as_tensor(xn))
    assert abs(float(loss) - float(l_ref)) < 1e-8
    assert float((aux.local_energy.cpu() - aux_ref.local_energy).abs().max()) < 1e-8
    assert_tree_close(grads, g_ref, 1e-7)


@pytest.mark.parametrize('system,hidden_dims', [('lih', ((8, 16), (64, 16), (64, 16))),        # two atoms, 'nu': 8 input features = hidden_single[0]
                                                ('bcc_li', ((4, 16), (4, 16), (64, 16))),      # one atom: 4; layers 0 AND 1 residual at width 4
                                                ('lih', ((64, 4), (64, 4), (64, 16))),         # pair stream: 4 pair features = hidden_double[0] (and [1])
                                                ('lih', ((8, 4), (64, 16)))])                  # both streams at once, two layers
def test_first_layer_as_wide_as_its_input_features(system, hidden_dims):
    """hidden_single[0] == nf x atoms (or hidden_double[0] == nf): the reference adds a residual at the FIRST layer (network.py:525-528).  Refused until round 6
    (its K = features + pair-mean rows is 64 k + 4 / + 8, and a width like 8 pads to 64 device features of which only 8 have a
    residual); now layer 0 runs without its residual and csrc/ds_kernels.h::k_layer_res_add (k_pair_res_add) finishes it.  Loss, local energies and
    the energy gradient -- energy chain, value chain and reverse sweep -- against the oracle."""
    from deepsolid_amd import network as dnet, train as dtrain
    from oracle.testing import make_test_params
    cell, klist = systems.build(system, **({'nelec': (3, 2)} if system == 'bcc_li' else {}))
    net_kw = dict(systems.DETNET_DEFAULTS, hidden_dims=hidden_dims)
    params = make_test_params(29, cell.original_cell.atom_coords(), cell.nelec, net_kw)
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    assert any(net.apply.system.residuals[0])
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type='real')
    dp = dev_params(params)
    xn = systems.synthetic_walkers(cell, 5, seed=23)
    (loss, aux), grads = loss_fn.value_and_grad(dp, torch.as_tensor(xn, device='cuda'))
    onet_ = oracle_net(cell, klist, net_kw, 'eval_logdet')
    oloss = otrain.make_loss(onet_.apply, cell, mode='hessian', clip_local_energy=5.0, clip_type='real')
    (l_ref, aux_ref), g_ref = oloss.value_and_grad(params, torch.as_tensor(xn))
    assert abs(float(loss) - float(l_ref)) < 1e-8
    assert float((aux.local_energy.cpu() - aux_ref.local_energy).abs().max()) < 1e-8
    assert_tree_close(grads, g_ref, 1e-7)


def test_forty_determinants():
    """More than 32 determinants (the reference has no bound; the library's is 64 since round 4): loss, local energies and energy
    gradient of a 40-determinant LiH wave function against the oracle."""
    from deepsolid_amd import network as dnet, train as dtrain
    from oracle.testing import make_test_params
    cell, klist = systems.build('lih')
    net_kw = dict(systems.DETNET_DEFAULTS, determinants=40)
    params = make_test_params(23, cell.original_cell.atom_coords(), cell.nelec, net_kw)
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type='real')
    xn = systems.synthetic_walkers(cell, 4, seed=22)
    (loss, aux), grads = loss_fn.value_and_grad(dev_params(params), torch.as_tensor(xn, device='cuda'))
    oloss = otrain.make_loss(oracle_net(cell, klist, net_kw, 'eval_logdet').apply, cell, mode='hessian', clip_local_energy=5.0, clip_type='real')
    (l_ref, aux_ref), g_ref = oloss.value_and_grad(params, torch.as_tensor(xn))
    assert abs(float(loss) - float(l_ref)) < 1e-8
    assert float((aux.local_energy.cpu() - aux_ref.local_energy).abs().max()) < 1e-8
    assert_tree_close(grads, g_ref, 1e-7)


def test_training_step_runs_and_lowers_the_energy_estimate():
    """train.make_training_step (train.py:147-184) with Adam: a few steps on LiH from a fixed seed."""
    from deepsolid_amd import network as dnet, qmc, train as dtrain
    fx, cell, klist, net_kw, params = load_case('lih')
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    B = 512
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type='real')
    mcmc = qmc.make_mcmc_step(slog.apply, B, cell.a, steps=5)
    init, update = dtrain.adam(2e-3)
    dp = dev_params(params)
    state = init(dp)
    step = dtrain.make_training_step(mcmc, loss_fn, update)
    data = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1), device='cuda')
    gen = torch.Generator(device='cuda'); gen.manual_seed(0)
    before = [p.clone() for p in leaves(dp)]
    losses = []
    for t in range(12):
        data, dp, state, loss, aux, pmove, g = step(t, data, dp, state, gen, 0.1)
        assert np.isfinite(float(loss)) and 0.0 < float(pmove) <= 1.0
        losses.append(float(loss))
    assert any(not torch.equal(a, b) for a, b in zip(before, leaves(dp)))
    assert np.mean(losses[-3:]) < np.mean(losses[:3])


def test_training_step_rejects_a_step_with_a_nan_walker():
    """process.py:303-318 (cfg.debug.check_nan) through the real kernels: one walker with a NaN coordinate makes its local energy
    NaN, `ds_energy_stats` counts it (n_nonfinite, all-reduced), and the step is DISCARDED before Adam touches anything --
    parameters, optimiser moments / step count and the walkers come back bit-identical, loss = aux = None.  The next step on
    finite walkers is applied.  Without check_nan the same step poisons the parameters (the reason it is on in run_training)."""
    from deepsolid_amd import network as dnet, qmc, train as dtrain
    fx, cell, klist, net_kw, params = load_case('lih')
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    B = 256
    loss_fn = dtrain.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type='real')
    real_mcmc = qmc.make_mcmc_step(slog.apply, B, cell.a, steps=3)
    poison = {'on': True}

    def mcmc(p, d, key, w):
        d2, pm = real_mcmc(p, d, key, w)
        if poison['on']:
            d2 = d2.clone()
            d2[7, 4] = float('nan')                       # one coordinate of one walker
        return d2, pm

    init, update = dtrain.adam(2e-3)
    dp = dev_params(params)
    state = init(dp)
    data = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=2), device='cuda')
    # the statistics kernel sees the bad walker
    bad = data.clone(); bad[7, 4] = float('nan')
    _, aux_bad = loss_fn(dp, bad)
    assert float(aux_bad.n_nonfinite) == 1.0
    step = dtrain.make_training_step(mcmc, loss_fn, update, check_nan=True)
    before = [p.clone() for p in leaves(dp)]
    d1, dp, state, loss, aux, pmove, g = step(0, data, dp, state, 11, 0.1)
    assert loss is None and aux is None and g is None and d1 is data
    assert state['count'] == 0 and all(float(m.abs().max()) == 0.0 for m in state['m'])
    assert all(torch.equal(a, b) for a, b in zip(before, leaves(dp)))
    poison['on'] = False
    d2, dp, state, loss, aux, pmove, g = step(1, data, dp, state, 12, 0.1)
    assert loss is not None and np.isfinite(float(loss)) and state['count'] == 1 and float(aux.n_nonfinite) == 0.0
    assert any(not torch.equal(a, b) for a, b in zip(before, leaves(dp)))
    # the reference's default (no check): the poisoned step is applied and the parameters are lost
    poison['on'] = True
    dq = dev_params(params)
    sq = init(dq)
    plain = dtrain.make_training_step(mcmc, loss_fn, update)
    _, dq, sq, loss, *_ = plain(0, data, dq, sq, 11, 0.1)
    assert not all(bool(torch.isfinite(p).all()) for p in leaves(dq))


def test_training_loop_writes_stats_and_reference_checkpoints(tmp_path):
    """inference.run_training (process.py:204-383, Adam branch): CSV rows in the reference schema, checkpoints that
    `checkpoint.restore` (reference layout) reads back, parameters updated in place."""
    from deepsolid_amd import checkpoint, inference, network as dnet
    fx, cell, klist, net_kw, params = load_case('lih')
    logdet = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    dp = dev_params(params)
    w0 = dp['single'][0]['w'].clone()
    data = torch.as_tensor(systems.synthetic_walkers(cell, 256, seed=4), device='cuda')
    data, dp2, state, width, rows = inference.run_training(slog, logdet, dp, data, cell, iterations=6, key=3, burn_in=5,
                                                           mcmc_steps=4, learning_rate=1e-3, save_path=str(tmp_path),
                                                           save_every=3)
    assert len(rows) == 6 and all(np.isfinite(r['energy']) for r in rows)
    assert not torch.equal(w0, dp['single'][0]['w'])
    lines = open(tmp_path / 'train_stats.csv').read().strip().splitlines()
    assert lines[0] == 'step,energy,variance,pmove,imaginary,kinetic,ewald' and len(lines) == 7
    last = checkpoint.find_last_checkpoint(str(tmp_path))
    assert last.endswith('qmcjax_ckpt_000005.npz')
    t, d, p, opt, w = checkpoint.restore(last, batch_size=256)
    x, p1, w1 = checkpoint.to_single_device(d, p, w)
    assert t == 6 and x.shape == (256, 12)
    np.testing.assert_array_equal(p1['single'][0]['w'], dp['single'][0]['w'].cpu().numpy())
    # resume (process.py:120-123,381): Adam moments and step count come back, no second burn-in, last step always saved
    opt1 = checkpoint.opt_state_to_single_device(opt)
    assert opt1['count'] == 6 and len(opt1['m']) == len(state['m'])
    np.testing.assert_array_equal(np.asarray(opt1['m'][0]), state['m'][0].cpu().numpy())
    data2, dp3, state2, _, rows2 = inference.run_training(slog, logdet, dp, torch.as_tensor(x, device='cuda'), cell, iterations=2, key=3,
                                                          burn_in=5, mcmc_steps=4, learning_rate=1e-3, save_path=str(tmp_path),
                                                          save_every=100, t_init=t, opt_state=opt1)
    assert [r['step'] for r in rows2] == [6, 7] and state2['count'] == 8
    assert checkpoint.find_last_checkpoint(str(tmp_path)).endswith('qmcjax_ckpt_000007.npz')


REF_GRAD_CASES = [c for c in __import__('oracle.testing', fromlist=['CASES']).CASES
                  if __import__('oracle.testing', fromlist=['CASES']).CASES[c].get('grad_walkers')]


@pytest.mark.parametrize('name', REF_GRAD_CASES)
def test_energy_gradient_vs_reference_train(name):
    """`total_energy.value_and_grad` (HIP local energy + clip + ds_logpsi_vjp) against the gradient the REFERENCE's own
    train.make_loss / jax.value_and_grad produced (tools/make_golden.py, torch-backed jax stand-in): loss, variance,
    every leaf's norm, its projection on a seeded direction, and the small leaves element-wise (1e-8 of the largest norm)."""
    from deepsolid_amd import network as dnet, train
    from oracle.testing import CASES
    from test_oracle_golden import check_gradient_against_reference
    fx, cell, klist, net_kw, params = load_case(name)
    net = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    dp = dev_params(params)
    nb = int(fx['grad_ref_walkers'])
    x = torch.as_tensor(fx['x'][:nb], device='cuda')
    for clip_type in CASES[name].get('grad_clip_types', ('real',)):
        sfx = '' if clip_type == 'real' else '_' + clip_type
        loss_fn = train.make_loss(net.apply, None, cell, clip_local_energy=5.0, clip_type=clip_type)
        (loss, aux), g = loss_fn.value_and_grad(dp, x)
        assert abs(float(loss) - float(fx['grad_ref_loss' + sfx])) < 1e-9 * max(1.0, abs(float(loss)))
        assert abs(float(aux.variance) - float(fx['grad_ref_variance' + sfx])) < 1e-8 * max(1.0, float(aux.variance))
        assert abs(float(aux.imaginary) - float(fx['grad_ref_imag' + sfx])) < 1e-9 * max(1.0, abs(float(loss)))
        assert float(aux.n_nonfinite) == 0.0
        check_gradient_against_reference(fx, params, g, sfx)
