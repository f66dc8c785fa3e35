"""CPU checks of the pretraining stage: the yardstick of the GPU tests (torch autograd over the oracle's `eval_mats`,
pretrain_helpers.oracle_pretrain) against the reference-executed fixture tests/golden/pretrain.npz, and the host logic of
deepsolid_amd/pretrain.py."""
import inspect
import os

import numpy as np
import pytest
import torch

from common import GOLDEN, load_case
from deepsolid_amd import pretrain, systems
from pretrain_helpers import GOLDEN_CASES, check_against_fixture, make_targets, oracle_pretrain, plane_waves


@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_oracle_autograd_vs_reference_executed_pretrain_step(name):
    """Loss and gradient of the reference's own make_pretrain_step (fixture) against autograd over the oracle: loss 1e-10
    relative, gradient 1e-8 of the largest leaf norm.  Covers the list mean (c_s), the per-entry counts, the block-diagonal
    target of full_det, use_last_layer, bias_orbitals, 16 determinants, a complex twist."""
    fx = np.load(os.path.join(GOLDEN, 'pretrain.npz'))
    cfx, cell, klist, net_kw, params = load_case(name)
    nw = int(fx[name + ':n_walkers'])
    x = cfx['x'][:nw]
    targets = make_targets(klist, x, int(fx[name + ':seed']))
    for s, t in enumerate(targets):
        np.testing.assert_array_equal(t, fx[f'{name}:target_{s}'])
    loss, grad = oracle_pretrain(cell, klist, net_kw, params, x, targets)
    check_against_fixture(fx, name, loss, grad, params)


def test_plane_wave_orbitals_against_numpy():
    cell, klist = systems.build('lih', twist=(0.25, 0.1, 0.4))
    x = systems.synthetic_walkers(cell, 5, seed=3)
    got = pretrain.PlaneWaveOrbitals(klist).eval_orb_mat(x.reshape(5, -1, 3))
    n_up = cell.nelec[0]
    for s, g in enumerate(got):
        xs = x.reshape(5, -1, 3)[:, :n_up] if s == 0 else x.reshape(5, -1, 3)[:, n_up:]
        ref = np.exp(1j * np.einsum('bic,mc->bim', xs, np.asarray(klist[s])))
        assert g.dtype == torch.complex128 and tuple(g.shape) == ref.shape
        np.testing.assert_allclose(g.numpy(), ref, rtol=0, atol=1e-14)
    for a, b in zip(got, plane_waves(klist, x)):
        np.testing.assert_allclose(a.numpy(), b, rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        pretrain.PlaneWaveOrbitals(klist).eval_orb_mat(x)


def test_block_diagonal_target_rule():
    """pretrain.py:79-86: blockdiag(up, dn), zeros elsewhere, [walker, electron, orbital]."""
    rng = np.random.default_rng(0)
    up = torch.as_tensor(rng.normal(size=(3, 2, 2)) + 1j * rng.normal(size=(3, 2, 2)))
    dn = torch.as_tensor(rng.normal(size=(3, 1, 1)) + 1j * rng.normal(size=(3, 1, 1)))
    t = pretrain.block_diagonal_target(up, dn)
    assert tuple(t.shape) == (3, 3, 3)
    assert torch.equal(t[:, :2, :2], up) and torch.equal(t[:, 2:, 2:], dn)
    assert float(t[:, :2, 2:].abs().max()) == 0.0 and float(t[:, 2:, :2].abs().max()) == 0.0


def test_signatures_follow_the_reference():
    sig = inspect.signature(pretrain.make_pretrain_step)
    assert list(sig.parameters)[:5] == ['batch_orbitals', 'batch_network', 'latvec', 'optimizer', 'full_det']
    assert sig.parameters['full_det'].default is False
    sig = inspect.signature(pretrain.pretrain_hartree_fock)
    assert list(sig.parameters)[:10] == ['params', 'data', 'batch_network', 'batch_orbitals', 'sharded_key', 'cell', 'scf_approx',
                                         'full_det', 'iterations', 'learning_rate']
    assert sig.parameters['iterations'].default == 1000 and sig.parameters['learning_rate'].default == 5e-3
    from deepsolid_amd import inference
    sig = inspect.signature(inference.run_training)
    assert sig.parameters['pretrain_iterations'].default == 0 and sig.parameters['scf_approx'].default is None


def test_make_pretrain_step_checks_its_networks():
    from deepsolid_amd import network, train
    cell, klist = systems.build('lih')
    kw = dict(systems.DETNET_DEFAULTS)
    mats = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_mats', **kw)
    slog = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **kw)
    opt = train.adam(5e-3)
    with pytest.raises(TypeError):
        pretrain.make_pretrain_step(slog.apply, slog.apply, cell.a, opt)
    with pytest.raises(ValueError):
        pretrain.make_pretrain_step(mats.apply, slog.apply, cell.a, opt, full_det=True)
    step = pretrain.make_pretrain_step(mats.apply, slog.apply, cell.a, opt)
    assert list(inspect.signature(step).parameters) == ['data', 'target', 'params', 'state', 'key']


@pytest.mark.skipif(torch.cuda.is_available(), reason='CPU-only behaviour')
def test_pretraining_fails_loudly_without_gpu():
    from deepsolid_amd import network
    cell, klist = systems.build('lih')
    kw = dict(systems.DETNET_DEFAULTS)
    mats = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_mats', **kw)
    slog = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **kw)
    params = slog.init(0)
    data = torch.as_tensor(systems.synthetic_walkers(cell, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        pretrain.pretrain_hartree_fock(params, data, slog.apply, mats.apply, 0, cell, pretrain.PlaneWaveOrbitals(klist), iterations=1)
