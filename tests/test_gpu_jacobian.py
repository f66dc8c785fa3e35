"""`ds_logpsi_jacobian`: the per-walker Jacobian of log psi in the packed parameters (csrc/ds_jac.h), against
  (1) the CPU oracle: rows from `oracle.train.logpsi_vjp` with one-hot cotangents (every leaf of every row within 1e-9 of that
      row-leaf's largest entry: the bound `test_vjp_vs_oracle_autograd` holds the same sweep to);
  (2) the library's own gradient: J^T [c_re ; c_im] (numpy, float64) = `logpsi_vjp(c)` for a random cotangent c, per leaf within
      1e-9 of its largest entry (float32: `common.float32_tolerance` against the float64 oracle);
  (3) itself: chunked against uncapped, call against call, repeated walkers -- to the bit.
Measured on the MI355X, J^T c against `logpsi_vjp(c)`, worst leaf: lih 7.8e-15 / 8.0e-15 / 6.0e-15 (B = 80 / 83 / 161), bcc_li 8.7e-15,
bcc_li_333 3.8e-14, diamond 1.1e-13, graphene 4.5e-14."""
import numpy as np
import pytest
import torch

import spring_helpers as sh
from common import float32_tolerance, load_case
from deepsolid_amd import systems
from test_gpu_grad import dev_params, fresh_system, leaf_devs, oracle_vjp, system_for

pytestmark = pytest.mark.gpu


def _jac_with_slack(sysd, dp, x, slack=5, **kw):
    B, P = x.shape[0], sysd.param_count
    out = torch.full((2 * B, P + slack), float('nan'), dtype=sysd.dtype, device='cuda')
    J, la, ph = sysd.logpsi_jacobian(dp, x, out=out, **kw)
    assert J.data_ptr() == out.data_ptr() and tuple(J.shape) == (2 * B, P)
    return out, J, la, ph


ORACLE_CASES = [('lih', 1), ('lih', 5), ('lih_twist', 4), ('lih_mixed', 3), ('lih_bias', 3), ('lih_lastlayer', 3), ('lih_fulldet', 3),
                ('lih_diagenv', 3), ('lih_fullenv', 3), ('li_polarized', 3), ('h2', 4), ('bcc_li', 2)]


@pytest.mark.parametrize('name,batch', ORACLE_CASES)
def test_jacobian_vs_oracle(name, batch, record_property):
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    x = systems.synthetic_walkers(cell, batch, seed=77)
    dp = dev_params(params)
    out, J, la, ph = _jac_with_slack(sysd, dp, torch.as_tensor(x, device='cuda'))
    P = sysd.param_count
    full = out.cpu().numpy()
    got = full[:, :P]
    assert not np.isnan(got).any()
    assert np.isnan(full[:, P:]).all()                        # the columns beyond param_count are not touched
    gather = sysd.param_map.layout(params).gather
    assert (got[:, gather < 0] == 0.0).all()                  # padding columns: exact zeros
    ref = sh.oracle_jacobian((cell, klist, net_kw, params), x, sysd.param_map)
    worst = 0.0
    for path, cols in sh.leaf_columns(sysd.param_map, params):
        g, r = got[:, cols], ref[:, cols]
        dev = np.abs(g - r).max(axis=1) / np.maximum(np.abs(r).max(axis=1), 1e-12)
        worst = max(worst, float(dev.max()))
        assert dev.max() <= 1e-9, (path, int(dev.argmax()), float(dev.max()))
    record_property('max_row_leaf_dev', worst)
    la2, ph2 = sysd.logpsi(dp, torch.as_tensor(x, device='cuda'))
    assert float((la - la2).abs().max()) < 1e-10 and float((ph - torch.view_as_complex(ph2)).abs().max()) < 1e-10


VJP_CASES = [('lih', 80), ('lih', 83), ('lih', 161), ('bcc_li', 83), ('bcc_li_333', 2), ('diamond', 2), ('graphene', 2)]


@pytest.mark.parametrize('name,batch', VJP_CASES)
def test_jacobian_contracts_to_the_vjp(name, batch, record_property):
    """lih at 80 / 83 / 161: a full group, a ragged last group, three groups; bcc_li_333: odd N, 6561 pairs (a partial pair tile)."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    x = torch.as_tensor(systems.synthetic_walkers(cell, batch, seed=78), device='cuda')
    cot = np.random.default_rng(6).normal(size=(batch, 2))
    dp = dev_params(params)
    out, J, _, _ = _jac_with_slack(sysd, dp, x)
    assert torch.isnan(out[:, sysd.param_count:]).all() and not torch.isnan(J).any()
    flat, _, _ = sysd.logpsi_vjp(dp, x, torch.as_tensor(cot, device='cuda'))
    got = J.cpu().numpy().T @ np.concatenate([cot[:, 0], cot[:, 1]])
    devs = leaf_devs(sysd.unpack_grad(torch.as_tensor(got), dp), sysd.unpack_grad(flat.cpu(), dp))
    record_property('max_leaf_dev', max(devs))
    print(f'{name} B={batch}: J^T c vs logpsi_vjp, worst leaf {max(devs):.3e}')
    assert max(devs) <= 1e-9, devs


def test_jacobian_float32_contracts_to_the_vjp(record_property):
    """lih, float32, B = 83: J^T c against the float64 oracle at the float32-rounded walkers and cotangents, per leaf within
    `common.float32_tolerance` of what the oracle's own float32 VJP loses."""
    fx, cell, klist, net_kw, params = load_case('lih')
    s32 = fresh_system(cell, klist, net_kw, torch.float32)
    x32 = torch.as_tensor(systems.synthetic_walkers(cell, 83, seed=78), dtype=torch.float32)
    c32 = torch.as_tensor(np.random.default_rng(6).normal(size=(83, 2)), dtype=torch.float32)
    p32 = dev_params(params, torch.float32)
    out, J, _, _ = _jac_with_slack(s32, p32, x32.cuda())
    assert J.dtype == torch.float32 and torch.isnan(out[:, s32.param_count:]).all() and not torch.isnan(J).any()
    got = J.double().cpu().numpy().T @ np.concatenate([c32[:, 0].double().numpy(), c32[:, 1].double().numpy()])
    ref = oracle_vjp(cell, klist, net_kw, params, x32.double(), c32.double())
    own = oracle_vjp(cell, klist, net_kw, params, x32, c32, dtype=torch.float32)
    loss = leaf_devs(own, ref)
    devs = leaf_devs(s32.unpack_grad(torch.as_tensor(got), p32), ref)
    ratio = [d / float32_tolerance(loss, i) for i, d in enumerate(devs)]
    record_property('max_leaf_dev', max(devs))
    record_property('max_ratio_to_bound', max(ratio))
    assert max(ratio) <= 1.0, list(zip(devs, loss))


def test_jacobian_chunks_calls_and_repeated_walkers_are_bit_identical():
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = fresh_system(cell, klist, net_kw)
    dp = dev_params(params)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 161, seed=79), device='cuda')
    J1 = sysd.logpsi_jacobian(dp, x)[0].clone()
    J2 = sysd.logpsi_jacobian(dp, x)[0].clone()
    assert torch.equal(J1, J2)
    one_group = int(sysd.lib.ds_jacobian_workspace_bytes(sysd.handle, 1))
    assert one_group < int(sysd.lib.ds_jacobian_workspace_bytes(sysd.handle, 161))
    J3 = sysd.logpsi_jacobian(dp, x, max_bytes=one_group)[0]
    assert torch.equal(J1, J3)
    xr = x[7:8].repeat(83, 1).contiguous()
    Jr = sysd.logpsi_jacobian(dp, xr)[0]
    assert torch.equal(Jr[:83], Jr[0:1].expand(83, -1)) and torch.equal(Jr[83:], Jr[83:84].expand(83, -1))
    assert torch.equal(Jr[0], J1[7]) and torch.equal(Jr[83], J1[161 + 7])


def test_jacobian_empty_batch_and_small_workspace():
    """B = 0 succeeds and writes nothing (the C contract); a workspace too small for one group is refused with a message before
    any launch (the output keeps its NaN fill)."""
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = fresh_system(cell, klist, net_kw)
    dp = dev_params(params)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 3, seed=80), device='cuda')
    J, la, ph = sysd.logpsi_jacobian(dp, x[:0])
    assert tuple(J.shape) == (0, sysd.param_count) and la.numel() == 0 and ph.numel() == 0
    out = torch.full((6, sysd.param_count), float('nan'), dtype=torch.float64, device='cuda')
    with pytest.raises(RuntimeError, match='workspace too small'):
        sysd.logpsi_jacobian(dp, x, out=out, max_bytes=4096)
    assert torch.isnan(out).all()
    with pytest.raises(ValueError, match='out must be'):
        sysd.logpsi_jacobian(dp, x, out=out[:, :-1])
