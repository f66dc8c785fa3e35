"""The SPRING optimizer on the GPU (`deepsolid_amd.spring`): the device step against the float64 numpy model of
tests/spring_helpers.py fed the device's own Jacobian, its tie to the existing energy gradient, the training driver, and that it
optimises."""
import types

import numpy as np
import pytest
import torch

import spring_helpers as sh
from common import load_case
from deepsolid_amd import systems
from test_gpu_grad import dev_params, system_for

pytestmark = pytest.mark.gpu


def _leaves(tree):
    from deepsolid_amd.params import tree_leaves
    return tree_leaves(tree)


@pytest.mark.parametrize('name,batch', [('lih', 5), ('lih', 83), ('lih', 300), ('lih_twist', 4)])
def test_step_against_the_model_on_the_device_jacobian(name, batch, record_property):
    """Two consecutive steps, mu = 0.9, lambda = 1e-3: phi' within 1e-9 of its largest entry, and the parameters follow.  The
    bound holds at condition <= 1e4 of T + lambda I, which is checked on the read-back matrix.
    On the fixture parameters T's largest eigenvalue is 2e3 ... 7e4, so with lambda = 1e-3 the raw condition is 2e6 (lih, B = 5),
    7e7 (lih, B = 83) and 6e6 (lih_twist) and no case would be fit.  The step takes the Jacobian as an argument, so device and
    model are both fed the device's J times a power of two s (exact in floating point; it amounts to the parameters theta / s)
    chosen from the read-back matrix such that the largest eigenvalue of T lies in (1.25, 5]: condition <= 5e3 + 1.
    B = 300 (R = 600 rows, param_count 469056) is the one case beyond the small-shape branches of csrc/ds_minsr.h: five rows of
    Gram tiles (15 tiles, the parameters dealt to 34 partials) and block = 300 > 256 in the centring kernels.  Its raw condition
    is 2.1e7 and 2.6e7, 1.3e3 and 1.6e3 after the scaling; measured on the MI355X, phi' deviates by 4.7e-15 and 4.4e-15 of its
    largest entry in the two steps."""
    from deepsolid_amd import spring
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    x = torch.as_tensor(systems.synthetic_walkers(cell, batch, seed=81), device='cuda')
    rng = np.random.default_rng(8)
    lam, mu, C = 1e-3, 0.9, 1e-3
    init, step = spring.spring(lambda t: 0.05 / (1 + t), damping=lam, mu=mu, norm_constraint=C)
    state = init(dp)
    model = {'count': 0, 'phi': np.zeros(sysd.param_count)}
    record_property('param_count', int(sysd.param_count))
    print(f'{name} B={batch}: param_count {sysd.param_count}')
    for k in range(2):
        d = rng.normal(size=batch) + 1j * rng.normal(size=batch)
        J = sysd.logpsi_jacobian(dp, x)[0]
        Jh = J.cpu().numpy()
        Jb = sh.centre(Jh, batch) / np.sqrt(batch)
        raw = np.linalg.eigvalsh(Jb @ Jb.T)[-1]
        s = 2.0 ** np.floor(0.5 * np.log2(5.0 / raw))
        print(f'{name} B={batch} step {k}: raw condition {(raw + lam) / lam:.3e}, J scaled by {s:g}')
        J, Jh, Jb = J * s, Jh * s, Jb * s
        ev = np.linalg.eigvalsh(Jb @ Jb.T)
        cond = (ev[-1] + lam) / (max(ev[0], 0.0) + lam)
        record_property(f'condition_step{k}', float(cond))
        print(f'{name} B={batch} step {k}: condition of T + lambda I = {cond:.3e}')
        if cond > 1e4:
            pytest.fail(f'unfit case: condition {cond:.3e} of T + lambda I exceeds 1e4')
        theta = sysd.pack_params(dp).double().cpu().numpy()
        model, theta_ref = sh.spring_step(Jh, d, model, theta, lambda t: 0.05 / (1 + t), damping=lam, mu=mu, norm_constraint=C)
        state, dp, phi = step(sysd, dp, state, J, torch.as_tensor(d, device='cuda'))
        got = phi.cpu().numpy()
        dev = float(np.abs(got - model['phi']).max() / np.abs(model['phi']).max())
        record_property(f'phi_dev_step{k}', dev)
        print(f'{name} B={batch} step {k}: phi deviation {dev:.3e}')
        assert dev <= 1e-9
        assert state['count'] == k + 1 and torch.equal(state['phi'], phi)
        theta_new = sysd.pack_params(dp).double().cpu().numpy()
        moved = np.abs(theta_ref - theta).max()
        assert moved > 0 and np.abs(theta_new - theta_ref).max() <= 1e-9 * moved + 4e-16 * np.abs(theta_ref).max()


def _energy(cell, klist, net_kw, **kw):
    from deepsolid_amd import network as dnet
    from deepsolid_amd import train
    logdet = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    return train.make_loss(logdet.apply, None, cell, **kw)


def test_large_damping_gives_the_energy_gradient(record_property):
    """Clipping off, mu = 0, lambda = 1e8 tr T: lambda phi' = the energy gradient within 1e-6 of its largest entry (the
    truncation term is |T| / lambda <= 1e-8).  Jbar^T e is the gradient of `value_and_grad_packed` whenever mean(d) = 0; with
    clipping off only Re mean(d) vanishes (measured here: mean(d) = -8.6e-17 - 0.28i, and the two gradients differ by 2.5e-2 of
    the largest entry, which is mean(Im d) times the mean phase row).  So the reference is the same gradient pass
    (`ds_logpsi_vjp`) with the centred cotangent (d - mean d) / B, and `value_and_grad_packed` is tied to that pass by its own
    cotangent d / B to the bit.  Measured on the MI355X: 1.5e-9."""
    from deepsolid_amd import spring
    fx, cell, klist, net_kw, params = load_case('lih')
    energy = _energy(cell, klist, net_kw, clip_local_energy=0.0)
    sysd = energy.system
    x = torch.as_tensor(systems.synthetic_walkers(cell, 83, seed=82), device='cuda')
    dp = dev_params(params)
    (loss, aux), grad = energy.value_and_grad_packed(dp, x)
    (loss2, _), d = energy.value_and_clip_diff(dp, x)
    assert torch.equal(loss, loss2)
    J = sysd.logpsi_jacobian(dp, x)[0]
    Jb = sh.centre(J.cpu().numpy(), 83) / np.sqrt(83)
    lam = 1e8 * float(np.trace(Jb @ Jb.T))
    before = sysd.pack_params(dp).clone()
    _, step = spring.spring(0.0, damping=lam, mu=0.0)
    state, dp, phi = step(sysd, dp, {'count': 0}, J, d)
    assert torch.equal(before, sysd.pack_params(dp))           # lr = 0: nothing moved
    assert abs(float(d.real.mean())) <= 1e-12 * float(d.abs().max())
    assert torch.equal(grad, sysd.logpsi_vjp(dp, x, d / 83)[0])
    print(f'mean(d) = {complex(d.mean()):.3e}; lambda phi vs value_and_grad_packed: {float((lam * phi - grad.double()).abs().max() / grad.abs().max()):.3e}')
    g = sysd.logpsi_vjp(dp, x, (d - d.mean()) / 83)[0].double()
    dev = float((lam * phi - g).abs().max() / g.abs().max())
    record_property('dev', dev)
    print(f'lambda phi vs energy gradient: {dev:.3e}')
    assert dev <= 1e-6


def _drivers(batch=16):
    from deepsolid_amd import network as dnet
    fx, cell, klist, net_kw, params = load_case('lih')
    logdet = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    x = torch.as_tensor(systems.synthetic_walkers(cell, batch, seed=4), device='cuda')
    return cell, slog, logdet, params, x


def test_run_training_spring_rows_and_bitwise_resume(tmp_path):
    from deepsolid_amd import checkpoint, inference
    cell, slog, logdet, params, x = _drivers()
    kw = dict(burn_in=0, mcmc_steps=4, move_width=0.1, optimizer='spring', spring={'damping': 1e-3, 'mu': 0.9})
    dp = dev_params(params)
    w0 = dp['single'][0]['w'].clone()
    _, p4, st4, _, rows = inference.run_training(slog, logdet, dp, x, cell, iterations=4, key=torch.Generator().manual_seed(5),
                                                 save_path=str(tmp_path / 'a'), **kw)
    assert len(rows) == 4 and all(set(r) == set(inference.TRAIN_SCHEMA) and np.isfinite(r['energy']) for r in rows)
    assert st4['count'] == 4 and set(st4) == {'count', 'phi'} and not torch.equal(w0, p4['single'][0]['w'])
    gen = torch.Generator().manual_seed(5)
    inference.run_training(slog, logdet, dev_params(params), x, cell, iterations=2, key=gen, save_path=str(tmp_path / 'b'), **kw)
    t, d, p, opt, w = checkpoint.restore(checkpoint.find_last_checkpoint(str(tmp_path / 'b')), batch_size=16)
    d, p, w = checkpoint.to_single_device(d, p, w)
    opt = checkpoint.opt_state_to_single_device(opt)
    assert t == 2 and opt['count'] == 2
    _, p22, st22, _, rows2 = inference.run_training(slog, logdet, dev_params(p), torch.as_tensor(d, device='cuda'), cell, iterations=2,
                                                    key=gen, t_init=t, opt_state=opt, **{**kw, 'move_width': w})
    assert [r['step'] for r in rows2] == [2, 3] and st22['count'] == 4
    for a, b in zip(_leaves(p4), _leaves(p22)):
        assert torch.equal(a, b)
    assert torch.equal(st4['phi'], st22['phi'])
    assert [r['energy'] for r in rows[2:]] == [r['energy'] for r in rows2]
    with pytest.raises(ValueError, match='unknown spring settings'):
        inference.run_training(slog, logdet, dev_params(params), x, cell, iterations=1, key=3, **{**kw, 'spring': {'momentum': 0.9}})


def test_discarded_steps_leave_everything_untouched():
    """check_nan: a NaN walker is caught before the Jacobian pass, a direction that is not finite before the update; either
    way walkers, parameters and state stay bit-identical, and the same step without the fault is kept."""
    from deepsolid_amd import spring
    fx, cell, klist, net_kw, params = load_case('lih')
    energy = _energy(cell, klist, net_kw)
    sysd = energy.system
    dp = dev_params(params)
    opt = spring.spring(0.05, mu=0.9)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 16, seed=40), device='cuda')
    mcmc = lambda p, data, key, width: (data + 0.01, torch.tensor(0.5))
    step = spring.make_spring_training_step(mcmc, energy, opt, check_nan=True)
    x, dp, state, loss, *_ = step(0, x, dp, opt[0](dp), None, 0.1)
    assert loss is not None and state['count'] == 1
    snap = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in state.items()}
    psnap = [t.clone() for t in _leaves(dp)]

    def untouched(out, data):
        d2, p2, s2, loss, aux, pmove, direction = out
        assert loss is None and aux is None and direction is None and d2 is data and s2 is state and p2 is dp
        assert state['count'] == snap['count'] and torch.equal(state['phi'], snap['phi'])
        assert all(torch.equal(a, b) for a, b in zip(psnap, _leaves(dp)))
    bad = x.clone()
    bad[3, 2] = float('nan')
    keep = bad.clone()
    untouched(step(1, bad, dp, state, None, 0.1), bad)
    assert torch.equal(torch.nan_to_num(bad, nan=7.0), torch.nan_to_num(keep, nan=7.0))
    # a direction that is not finite although every local energy is: the cotangent carries an infinity
    poison = [True]

    def value_and_clip_diff(p, data):
        out, d = energy.value_and_clip_diff(p, data)
        if poison[0]:
            d = d.clone()
            d[2] = float('inf')
        return out, d
    fake = types.SimpleNamespace(system=sysd, value_and_clip_diff=value_and_clip_diff)
    step2 = spring.make_spring_training_step(mcmc, fake, opt, check_nan=True)
    untouched(step2(1, x, dp, state, None, 0.1), x)
    poison[0] = False
    data, dp2, state2, loss, aux, pmove, direction = step2(1, x, dp, state, None, 0.1)
    assert loss is not None and state2['count'] == 2 and not torch.equal(data, x)
    assert not all(torch.equal(a, b) for a, b in zip(psnap, _leaves(dp)))


def test_it_optimises(record_property):
    """`lih`, B = 256, 12 iterations from the example's random start, mcmc_steps = 4: the last row's energy lies below the first
    row's by more than five standard errors of the first row.
    The norm constraint caps a step's length at sqrt(C), and from random parameters it binds in every step: the default C = 1e-3
    (tuned for long runs from a pretrained start) allows a path of 12 x 0.032 = 0.38 in these 12 iterations and measured a drop of
    2.2 standard errors, C = 1e-2 4.2.  The optimizer's settings are this test's to choose: it runs C = 0.1 (steps of at most
    0.32), everything else at its default.  Measured on the MI355X: 7.3 standard errors (-2.070 -> -3.512 Ha, sigma 0.197)."""
    from deepsolid_amd import inference, network
    cell, klist = systems.build('lih')
    kw = dict(systems.DETNET_DEFAULTS)
    logdet = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **kw)
    slogdet = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **kw)
    params = logdet.init(0)
    data = torch.as_tensor(systems.synthetic_walkers(cell, 256), device='cuda')
    _, _, state, _, rows = inference.run_training(slogdet, logdet, params, data, cell, iterations=12, burn_in=20, move_width=0.1,
                                                  mcmc_steps=4, optimizer='spring', spring={'norm_constraint': 0.1})
    assert len(rows) == 12 and all(np.isfinite(r['energy']) for r in rows) and state['count'] == 12
    e0, e1 = rows[0]['energy'], rows[-1]['energy']
    sigma = float(np.sqrt(rows[0]['variance'] / 256))
    record_property('energies', [r['energy'] for r in rows])
    print('spring energies:', ' '.join(f"{r['energy']:.4f}" for r in rows), f'sigma0 = {sigma:.4f}')
    assert e1 < e0 - 5 * sigma, (e0, e1, sigma)
