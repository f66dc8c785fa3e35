"""The SPRING optimizer without a GPU: the numpy model of tests/spring_helpers.py against the parameter-space form, its momentum
recursion, norm constraint and null-vector property; the C ABI of the new entries; what `spring(...)` and `run_training` refuse;
the state's round trip through a checkpoint."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spring_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['ds_jacobian_workspace_bytes', 'ds_logpsi_jacobian', 'ds_minsr_gram_workspace_bytes', 'ds_minsr_gram',
       'ds_minsr_matvec_workspace_bytes', 'ds_minsr_matvec', 'ds_minsr_solve_workspace_bytes', 'ds_minsr_solve']


def _problem(B=7, P=50, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(2 * B, P)), rng.normal(size=B) + 1j * rng.normal(size=B), rng


def test_mu_zero_is_damped_stochastic_reconfiguration():
    """The push-through identity: Jbar^T (Jbar Jbar^T + l I)^-1 e = (Jbar^T Jbar + l I)^-1 Jbar^T e, 1e-10 relative."""
    J, d, _ = _problem()
    for lam in (1e-3, 1e-1, 3.0):
        a = sh.spring_direction(J, d, np.zeros(50), lam, 0.0)
        b = sh.sr_direction(J, d, lam)
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), lam


def test_momentum_recursion_over_three_steps():
    """phi_k = mu phi_{k-1} + Jbar_k^T (T_k + l I)^-1 (e_k - mu Jbar_k phi_{k-1}), written out with explicit matrices."""
    lam, mu, B = 1e-2, 0.9, 7
    state, theta = {'count': 0, 'phi': np.zeros(50)}, np.zeros(50)
    phi = np.zeros(50)
    for k in range(3):
        J, d, _ = _problem(seed=10 + k)
        state, theta_new = sh.spring_step(J, d, state, theta, lr=10.0, damping=lam, mu=mu, norm_constraint=1e6)
        H = np.eye(2 * B) - np.kron(np.eye(2), np.full((B, B), 1.0 / B))
        Jb = H @ J / np.sqrt(B)
        e = np.concatenate([d.real, d.imag]) / np.sqrt(B)
        phi = mu * phi + Jb.T @ np.linalg.inv(Jb @ Jb.T + lam * np.eye(2 * B)) @ (e - mu * Jb @ phi)
        assert state['count'] == k + 1
        assert np.abs(state['phi'] - phi).max() <= 1e-10 * np.abs(phi).max()
        # C = 1e6 leaves the norm constraint slack: the step is lr phi'
        assert np.abs(theta_new - (theta - 10.0 * phi)).max() <= 1e-9 * np.abs(theta_new).max()
        theta = theta_new


def test_norm_constraint_on_both_sides_of_its_kink():
    J, d, _ = _problem(seed=3)
    phi = sh.spring_direction(J, d, np.zeros(50), 1e-3, 0.0)
    n = np.linalg.norm(phi)
    for lr, C, want in ((0.5 / n, 1.0, 0.5 / n),              # lr below sqrt(C) / |phi'|: the plain step
                        (2.0 / n, 1.0, 1.0 / n),              # above: the step has length sqrt(C)
                        (1e-3, 1e-3, min(1e-3, np.sqrt(1e-3) / n))):
        state, theta = sh.spring_step(J, d, {'count': 0, 'phi': np.zeros(50)}, np.zeros(50), lr, damping=1e-3, mu=0.0, norm_constraint=C)
        assert np.abs(theta + want * phi).max() <= 1e-14 * np.abs(want * phi).max()
        assert np.abs(state['phi'] - phi).max() == 0.0         # phi is kept unscaled
    _, theta = sh.spring_step(J, d, {'count': 0, 'phi': np.zeros(50)}, np.zeros(50), 2.0 / n, damping=1e-3, mu=0.0, norm_constraint=1.0)
    assert abs(np.linalg.norm(theta) - 1.0) < 1e-12


def test_a_constant_added_to_d_changes_nothing():
    """e - mu Jbar phi meets the null vectors of T only through mean(d), and Jbar^T annihilates that component."""
    J, d, rng = _problem(seed=4)
    phi0 = rng.normal(size=50)
    for mu in (0.0, 0.9):
        a = sh.spring_direction(J, d, phi0, 1e-3, mu)
        b = sh.spring_direction(J, d + (0.7 - 0.3j), phi0, 1e-3, mu)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), mu


def test_new_entries_are_declared_exported_and_bound():
    from deepsolid_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r'\b%s\s*\(' % n, src), f'{n} is not declared in the header'
        assert hasattr(lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES
    # the argument checks that need no device
    lib = _lib.load()
    assert lib.ds_minsr_solve_workspace_bytes(6, 4) == -1 and lib.ds_minsr_solve_workspace_bytes(6, 3) > 0
    assert lib.ds_minsr_solve_workspace_bytes(6, 0) > 0
    assert lib.ds_minsr_gram_workspace_bytes(2, 70001) > 0 and lib.ds_minsr_gram_workspace_bytes(8192, 500000) == 0
    assert lib.ds_minsr_matvec_workspace_bytes(0, 4, 4) == 0 and lib.ds_minsr_matvec_workspace_bytes(2, 4, 4) == -1
    one = C.c_void_p(8)      # (never dereferenced: the calls below are refused before any launch)
    assert lib.ds_minsr_solve(6, 4, 1.0, 1e-3, one, one, one, one, 1 << 20, None) != 0
    assert b'multiple of block' in lib.ds_last_error()
    assert lib.ds_minsr_solve(6, 3, 1.0, 0.0, one, one, one, one, 1 << 20, None) != 0
    assert b'lambda must be positive' in lib.ds_last_error()
    assert lib.ds_minsr_gram(2, one, 4, 4, 4, one, one, 0, None) != 0 and b'dtype' in lib.ds_last_error()
    assert lib.ds_minsr_matvec(0, 0, one, 4, 8, 4, one, one, None, 0, None) != 0 and b'ld' in lib.ds_last_error()


def test_spring_refuses_bad_settings():
    from deepsolid_amd import spring
    for kw in ({'damping': 0.0}, {'damping': -1.0}, {'mu': 1.0}, {'mu': -0.1}, {'norm_constraint': 0.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            spring.spring(1e-2, **kw)
    init, step = spring.spring(1e-2)
    assert init({}) == {'count': 0}
    assert spring.spring(1e-2, mu=0.0) and spring.spring(lambda t: 0.1, damping=1e-6, mu=0.5, norm_constraint=10.0)


def test_run_training_refuses_before_touching_the_gpu():
    from deepsolid_amd import inference
    args = (None, None, {}, torch.zeros(2, 12), None)
    with pytest.raises(ValueError, match='optimizer'):
        inference.run_training(*args, iterations=1, optimizer='sgd')
    with pytest.raises(ValueError, match='spring'):
        inference.run_training(*args, iterations=1, optimizer='adam', spring={'mu': 0.5})
    with pytest.raises(ValueError, match='kfac'):
        inference.run_training(*args, iterations=1, optimizer='spring', kfac={'damping': 1e-3})


def test_more_than_one_rank_is_refused(monkeypatch):
    import types

    from deepsolid_amd import constants, spring
    monkeypatch.setattr(constants, 'world_size', lambda: 2)
    energy = types.SimpleNamespace(system=None, value_and_clip_diff=None)
    step = spring.make_spring_training_step(None, energy, spring.spring(1e-2))
    with pytest.raises(NotImplementedError, match="every rank"):
        step(0, None, None, {'count': 0}, None, 0.1)


def test_state_round_trip_through_a_checkpoint(tmp_path):
    from deepsolid_amd import checkpoint
    phi = torch.arange(11, dtype=torch.float64) / 7
    state = {'count': 3, 'phi': phi}
    params = {'single': [{'w': torch.ones(2, 3), 'b': torch.zeros(3)}]}
    name = checkpoint.save(str(tmp_path), 5, torch.zeros(4, 6), params, state, 0.1)
    t, data, p, opt, width = checkpoint.restore(name, batch_size=4)
    opt = checkpoint.opt_state_to_single_device(opt)
    assert t == 6 and set(opt) == {'count', 'phi'} and opt['count'] == 3
    assert np.array_equal(np.asarray(opt['phi']), phi.numpy())
    fresh = {'count': 0}                                       # before the first step the state has no phi yet
    name = checkpoint.save(str(tmp_path), 0, torch.zeros(4, 6), params, fresh, 0.1)
    assert checkpoint.opt_state_to_single_device(checkpoint.restore(name, batch_size=4)[3]) == {'count': 0}
