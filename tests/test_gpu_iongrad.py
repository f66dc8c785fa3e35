"""GPU tests of `ds_logpsi_ion_vjp` (csrc/ds_iongrad.h), `DeviceSystem.logpsi_ion_vjp` / `logpsi_ion_grad` and
`estimator.PrimitiveForces`: the gradient of log psi in the atoms of the primitive cell against torch
autograd over the CPU oracle (tests/iongrad_helpers.py), the translation identities that tie it to the walker gradient of the
forward-Laplacian chain, chunking, the float32 handle, the refusals and the accumulator's block rows.

Tolerances: float64 1e-9 of the largest reference entry of a case (what `test_vjp_vs_oracle_autograd` puts on the same sweep);
float32 per walker 3x what the helper's own float32 run loses (`common.float32_tolerance`); sums 1e-10 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import iongrad_helpers as H
from common import float32_tolerance, load_case
from deepsolid_amd import systems

pytestmark = pytest.mark.gpu

PV = 80


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(np.asarray(vv), dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v]
            for k, v in params.items()}


def system_for(cell, klist, net_kw, dtype=torch.float64):
    from deepsolid_amd.device import DeviceSystem
    return DeviceSystem.for_network(cell, klist, net_kw, dtype)


def cu(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dtype, device='cuda')


CASES = [('h2', 5), ('lih', 7), ('lih_twist', 4), ('lih_2x1x1', 3), ('lih_fulldet', 4), ('lih_tri', 4), ('lih_diagenv', 4),
         ('lih_fullenv', 4), ('lih_lastlayer', 4), ('lih_bias', 4), ('lih_det3', 3), ('lih_fcc', 3), ('lih_narrow', 3),
         ('graphene_hex', 2), ('li_polarized', 3), ('graphene', 2), ('diamond', 2)]


def check_against_reference(sysd, dp, x, O, record_property):
    """random cotangent and both parts of logpsi_ion_grad against O (B, A, 3) complex: 1e-9 of the largest reference entry"""
    B = len(x)
    cot = np.random.default_rng(5).normal(size=(B, 2))
    out, la, ph = sysd.logpsi_ion_vjp(dp, cu(x), cu(cot))
    assert out.dtype == torch.float64 and tuple(out.shape) == O.shape
    ref = cot[:, 0, None, None] * O.real + cot[:, 1, None, None] * O.imag
    dev_cot = float(np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max())
    got = sysd.logpsi_ion_grad(dp, cu(x)).cpu().numpy()
    dev_re = float(np.abs(got.real - O.real).max() / np.abs(O.real).max())
    dev_im = float(np.abs(got.imag - O.imag).max() / max(np.abs(O.imag).max(), 1e-300))
    for k, v in (('dev_cot', dev_cot), ('dev_re', dev_re), ('dev_im', dev_im)):
        record_property(k, v)
    print(f'ion grad deviations: cot {dev_cot:.3e} re {dev_re:.3e} im {dev_im:.3e} (max |O| {np.abs(O).max():.3e})')
    assert dev_cot <= 1e-9 and dev_re <= 1e-9
    # a real psi (no twist) has an arg that is piecewise constant: the reference is exactly zero there, and so must the call be
    if np.abs(O.imag).max() > 0:
        assert dev_im <= 1e-9
    else:
        assert np.abs(got.imag).max() <= 1e-9 * np.abs(O.real).max()
    return la, ph


@pytest.mark.parametrize('name,batch', CASES)
def test_ion_grad_vs_oracle_autograd(name, batch, record_property):
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    x, O, lp = H.reference(name, batch)
    la, ph = check_against_reference(sysd, dev_params(params), x, O, record_property)
    assert float(np.abs(la.cpu().numpy() - lp.real).max()) < 1e-9
    assert float(np.abs(np.angle(ph.cpu().numpy() * np.exp(-1j * lp.imag))).max()) < 1e-9


def test_ion_grad_first_layer_residuals(record_property):
    """hidden_dims = ((8, 4), (64, 16), (64, 16)) on LiH: both first-layer residuals are active, so the carry of layer 0's output
    cotangent reaches the 8 feature rows (and only them: the device width is 64)."""
    from oracle.testing import make_test_params
    cell, klist = systems.build('lih')
    net_kw = dict(systems.DETNET_DEFAULTS, hidden_dims=((8, 4), (64, 16), (64, 16)))
    params = make_test_params(29, cell.original_cell.atom_coords(), cell.nelec, net_kw)
    sysd = system_for(cell, klist, net_kw)
    assert all(sysd.residuals[0])
    x = systems.synthetic_walkers(cell, 4, seed=77)
    O, _ = H.ion_grad_ref(cell, klist, net_kw, params, x)
    check_against_reference(sysd, dev_params(params), x, O, record_property)


@pytest.mark.parametrize('name', ['lih_twist', 'bcc_li', 'graphene', 'diamond'])
def test_translation_identities_on_the_device(name, record_property):
    """A rigid translation of electrons AND atoms multiplies psi by exp(i t . sum of the occupied k-points):
    sum_a O_a + sum_i grad_i log psi = i sum of the klist rows.  The two sides come from different chains -- the reverse sweep of
    the value chain and the forward jets of the energy chain -- at B = PV + 1 (two groups, the second with one walker)."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    B, N = PV + 1, sum(cell.nelec)
    x = cu(systems.synthetic_walkers(cell, B, seed=77))
    O = sysd.logpsi_ion_grad(dp, x).cpu().numpy()
    g = sysd.logpsi_grad(dp, x)[1].cpu().numpy().reshape(B, N, 3)
    s = O.sum(1) + g.sum(1)
    ksum = H.klist_row_sum(klist, cell.nelec)
    scale = max(np.abs(g).max(), np.abs(O).max())
    dev_re, dev_im = float(np.abs(s.real).max() / scale), float(np.abs(s.imag - ksum).max() / scale)
    record_property('dev_re', dev_re)
    record_property('dev_im', dev_im)
    print(f'translation identity: re {dev_re:.3e} im {dev_im:.3e} (scale {scale:.3e}, k sum {ksum})')
    assert dev_re <= 1e-9 and dev_im <= 1e-9


def test_chunking_is_bit_identical():
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    B = 2 * PV + 1
    x = cu(systems.synthetic_walkers(cell, B, seed=77))
    cot = cu(np.random.default_rng(9).normal(size=(B, 2)))
    full, la, ph = sysd.logpsi_ion_vjp(dp, x, cot)
    full, la = full.clone(), la.clone()
    one_group = int(sysd.lib.ds_ion_vjp_workspace_bytes(sysd.handle, 1))
    assert int(sysd.lib.ds_ion_vjp_workspace_bytes(sysd.handle, B)) > one_group
    chunked, la2, _ = sysd.logpsi_ion_vjp(dp, x, cot, max_bytes=one_group)          # three passes
    assert torch.equal(full, chunked) and torch.equal(la, la2)
    again, _, _ = sysd.logpsi_ion_vjp(dp, x, cot)
    assert torch.equal(full, again)
    assert bool(torch.isfinite(full).all())
    scale = float(full.abs().max())
    for b in (1, PV - 1):                                                              # a single walker, a group one short
        part, _, _ = sysd.logpsi_ion_vjp(dp, x[:b], cot[:b])
        assert tuple(part.shape) == (b, 2, 3)
        assert float((part - full[:b]).abs().max()) <= 1e-12 * scale


F32_CASES = [('lih', 7), ('graphene', 2), ('diamond', 2)]


@pytest.mark.parametrize('name,batch', F32_CASES)
def test_float32_handle(name, batch, record_property):
    """A float32 handle at the float32-rounded walkers against the float64 reference there.  Per walker the deviation
    max |got - ref| / max |ref| is bounded by `float32_tolerance` of what the helper's own float32 run loses."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw, torch.float32)
    x32 = systems.synthetic_walkers(cell, batch, seed=77).astype(np.float32)
    ref, _ = H.ion_grad_ref(cell, klist, net_kw, params, x32.astype(np.float64))
    own, _ = H.ion_grad_ref(cell, klist, net_kw, params, x32, dtype=torch.float32)
    scale = np.abs(ref).reshape(batch, -1).max(1)
    loss = tuple(float(v) for v in np.abs(own - ref).reshape(batch, -1).max(1) / scale)
    got = sysd.logpsi_ion_grad(dev_params(params, torch.float32), cu(x32, torch.float32))
    assert got.dtype == torch.complex128
    dev = np.abs(got.cpu().numpy() - ref).reshape(batch, -1).max(1) / scale
    record_property('dev', [float(v) for v in dev])
    record_property('loss', list(loss))
    print(f'float32 {name}: deviation {dev} against the oracle\'s own float32 loss {loss}')
    for b in range(batch):
        assert dev[b] <= float32_tolerance(loss, b), (b, dev[b], loss[b])


def test_refusals_launch_nothing():
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    B = 3
    x = cu(systems.synthetic_walkers(cell, B, seed=77))
    cot = cu(np.ones((B, 2)))
    p = sysd.pack_params(dp)
    out = torch.empty(B, 2, 3, dtype=torch.float64, device='cuda')
    nbytes = int(sysd.lib.ds_ion_vjp_workspace_bytes(sysd.handle, B))
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    small = int(sysd.lib.ds_ion_vjp_workspace_bytes(sysd.handle, 1)) - 257          # (the size carries 256 bytes of slack)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(None)

    def call(x_=None, cot_=None, out_=None, B_=B, ws_bytes=nbytes):
        return sysd.lib.ds_logpsi_ion_vjp(sysd.handle, ptr(p), ptr(x) if x_ is None else x_, B_, ptr(cot) if cot_ is None else cot_,
                                          ptr(out) if out_ is None else out_, null, null, ptr(ws), ws_bytes, null)
    torch.cuda.synchronize()
    sysd.profile(True)
    try:
        for kw, word in ((dict(x_=null), 'x'), (dict(cot_=null), 'cot'), (dict(out_=null), 'out'), (dict(B_=0), 'B'), (dict(B_=-2), 'B'),
                         (dict(ws_bytes=small), 'workspace'), (dict(ws_bytes=0), 'workspace')):
            rc = call(**kw)
            msg = sysd.lib.ds_last_error().decode()
            assert rc != 0 and word in msg and 'ds_logpsi_ion_vjp' in msg, (kw, rc, msg)
        assert sysd.profile_read()['ion_vjp'][1] == 0            # no chunk of the pass was entered: nothing was launched
        assert call() == 0                                       # ... and the counter does count a call that runs
        assert sysd.profile_read()['ion_vjp'][1] == 1
    finally:
        sysd.profile(False)
    assert bool(torch.isfinite(out).all())


def test_primitive_forces_block_rows(tmp_path):
    """Two updates of B = 200 on lih_2x1x1 (two images per primitive atom), one walker of the second made non-finite: the block
    rows against the numpy model of iongrad_helpers built from `local_energy`, `ion_forces` and `logpsi_ion_grad` read back (sums
    in a different order: 1e-10 relative), the bad walker absent from every column and counted once, and `energies=` passed by
    the caller giving the same bits as the accumulator's own."""
    from deepsolid_amd import dmc, estimator, network
    fx, cell, klist, net_kw, params = load_case('lih_2x1x1')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    sysd, dp = net.apply.system, dev_params(params)
    B, A = 200, 2
    xs = [cu(systems.synthetic_walkers(cell, B, seed=77)), cu(systems.synthetic_walkers(cell, B, seed=78))]
    xs[1][137, 4] = float('nan')
    acc, given = estimator.PrimitiveForces(net, dp), estimator.PrimitiveForces(net, dp)
    assert acc.scale == 2 and acc.n_atoms == A
    model = []
    for x in xs:
        acc.update(x)
        ke, ew, _, _ = sysd.local_energy(dp, x)
        E = torch.complex(ke[:, 0] + ew, ke[:, 1])
        given.update(x, energies=E)
        f = sysd.ion_forces(x, sysd.logpsi_grad(dp, x)[1].real.contiguous())
        O = sysd.logpsi_ion_grad(dp, x)
        model.append(H.block_row_model(E.cpu().numpy(), f['zv'].cpu().numpy(), f['hf'].cpu().numpy(), O.cpu().numpy(), acc.owner, A))
    rows = acc.rows
    assert rows.is_cuda and tuple(rows.shape) == (2, 3 + 9 * A)
    assert torch.equal(rows, given.rows)
    rows, model = rows.cpu().numpy(), np.asarray(model)
    dev = np.abs(rows - model) / np.abs(model)
    print(f'PrimitiveForces block rows against the model: largest relative deviation {dev.max():.3e}; sum t {rows[:, 3:].reshape(2, A, 3, 3)[..., 2]}')
    assert np.isfinite(rows).all() and dev.max() <= 1e-10
    assert rows[0, 0] == B and rows[1, 0] == B - 1 and int(acc.n_bad) == 1 and acc.n_walkers == 2 * B
    r = acc.forces()
    ref = H.forces_model(model, A, dmc.reblock)
    for k in ('total', 'zv', 'hf', 'pulay'):
        np.testing.assert_allclose(r[k], ref[k][0], rtol=1e-9, atol=1e-12)
    assert r['n_blocks'] == 2 and r['n_bad'] == 1 and r['cutoff'] == sysd.force_cutoff()
    np.testing.assert_array_equal(r['atoms'], np.asarray(cell.original_cell.atom_coords()))
    acc.save(str(tmp_path / 'forces_total.npz'))
    np.testing.assert_array_equal(estimator.PrimitiveForces.load(str(tmp_path / 'forces_total.npz')).forces()['total'], r['total'])
