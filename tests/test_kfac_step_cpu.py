"""CPU checks of the KFAC step: the C-ABI boundary of `ds_kfac_inverses` / `ds_kfac_precondition` (csrc/ds_kfac.h), the torch
restatement the GPU tests compare against (tests/kfac_step_helpers.py) against reference-executed numbers
(tests/golden/kfac_inverse.npz, tools/make_kfac_golden.py) and against closed forms, and what `deepsolid_amd.kfac` refuses."""
import math
import os
import re

import numpy as np
import pytest
import torch

import kfac_step_helpers as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ds_kfac_step_workspace_bytes', 'ds_kfac_inverses', 'ds_kfac_precondition', 'ds_kfac_inverses_sized_workspace_bytes',
               'ds_kfac_inverses_sized')


def test_kfac_step_symbols_exported_and_declared():
    from deepsolid_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, src), f'{n} is not declared in include/deepsolid_hip.h'


def test_restatement_against_reference_executed_inverses():
    """`pi_adjusted_inverse` of the restatement against the reference's own (executed by tools/make_kfac_golden.py): 1e-12 of
    each inverse's largest entry -- both sides are float64 direct solves of the same well-conditioned systems -- and the
    reference's `psd_inv_cholesky` against a plain inverse of matrix + damping I."""
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'kfac_inverse.npz')) as z:
        gold = {k: z[k] for k in z.files}
    cases = [str(c) for c in gold['cases']]
    assert len(cases) == 8 and any(c.startswith('zero') for c in cases)
    for c in cases:
        f0, f1, damping = gold[f'{c}:factor_0'], gold[f'{c}:factor_1'], float(gold[f'{c}:damping'])
        a_inv, g_inv = ks.pi_adjusted_inverse(f0, f1, damping)
        for got, ref in ((a_inv, gold[f'{c}:inverse_0']), (g_inv, gold[f'{c}:inverse_1'])):
            ref = torch.as_tensor(ref)
            assert got.shape == ref.shape
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), c
        if f'{c}:chol_inverse' in gold:
            ref = torch.as_tensor(gold[f'{c}:chol_inverse'])
            got = torch.linalg.inv(torch.as_tensor(f0) + damping * torch.eye(f0.shape[0], dtype=torch.float64))
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), c


@pytest.mark.parametrize('d_in,d_out,a,g,lam', [(3, 2, 0.5, 2.0, 1e-3), (7, 5, 1e-4, 3.0, 1e-1)])
def test_scaled_identities_closed_form(d_in, d_out, a, g, lam):
    """A = a I, G = g I: s = a g d_in d_out, A / n0 = I / d_in, so A^- = I / ((1 / d_in + sqrt(lam d_out / (s d_in))) sqrt(s))."""
    a_inv, g_inv = ks.pi_adjusted_inverse(a * torch.eye(d_in, dtype=torch.float64), g * torch.eye(d_out, dtype=torch.float64), lam)
    s = a * g * d_in * d_out
    ea = 1.0 / ((1.0 / d_in + math.sqrt(lam * d_out / (s * d_in))) * math.sqrt(s))
    eg = 1.0 / ((1.0 / d_out + math.sqrt(lam * d_in / (s * d_out))) * math.sqrt(s))
    assert float((a_inv - ea * torch.eye(d_in, dtype=torch.float64)).abs().max()) <= 1e-13 * ea
    assert float((g_inv - eg * torch.eye(d_out, dtype=torch.float64)).abs().max()) <= 1e-13 * eg
    # the Kronecker product of the two inverses is the inverse of  A (x) G + lam I  up to the pi split:
    # 1 / (ea eg) = (a + pi-damping)(g + damping / pi) >= a g + lam
    assert 1.0 / (ea * eg) >= a * g + lam * (1 - 1e-12)


def test_zero_factor_gives_identity_over_sqrt_lambda():
    lam = 1e-3 / 4
    a_inv, g_inv = ks.pi_adjusted_inverse(torch.zeros(4, 4), torch.eye(3, dtype=torch.float64), lam)
    assert torch.equal(a_inv, torch.eye(4, dtype=torch.float64) / math.sqrt(lam))
    assert torch.equal(g_inv, torch.eye(3, dtype=torch.float64) / math.sqrt(lam))
    assert ks.damped(torch.zeros(4, 4), torch.eye(3), lam) is None


def _toy(scale, seed=0):
    rng = np.random.default_rng(seed)
    t = lambda *s: torch.as_tensor(rng.normal(size=s) * scale)
    tree = lambda: {'single': [{'w': t(3, 2), 'b': t(2)}], 'double': [], 'orbital': [{'w': t(2, 4)}],
                    'envelope': [{'pi': t(2, 2), 'sigma': t(2, 2)}]}
    shapes = [('single', 0, True, 4, 2, 3), ('orbital', 0, False, 2, 4, 2)]
    x = [torch.as_tensor(rng.normal(size=(6, s[3]))) for s in shapes]
    y = [torch.as_tensor(rng.normal(size=(6, s[4]))) for s in shapes]
    factors = [(a.T @ a / 6, b.T @ b / 6) for a, b in zip(x, y)]
    return shapes, tree, factors


@pytest.mark.parametrize('scale,clipped', [(1.0, True), (1e-6, False)])
def test_norm_constraint(scale, clipped):
    """With c < 1 the update has <P, g> lr^2 c^2 = norm_constraint; a tiny gradient is not clipped (c = 1)."""
    shapes, tree, factors = _toy(1.0)
    params, seed_grad = tree(), tree()
    grad = {k: [{kk: vv * scale for kk, vv in d.items()} for d in v] for k, v in tree().items()}
    lr, nc = 0.05, 1e-3
    state, delta = ks.kfac_step(ks.init_state(shapes, params), shapes, params, grad, factors, seed_grad, 6, lr, norm_constraint=nc)
    assert (state['c'] < 1.0) == clipped
    # delta = -lr c P, so <delta, g> = -lr c <P, g>  and  <P, g> lr^2 c^2 = -<delta, g> lr c
    dot = sum(float((delta[s[0]][s[1]] * ks.block_matrix(grad, s[0], s[1])).sum()) for s in shapes)
    dot += sum(float((delta['envelope'][0][k] * grad['envelope'][0][k]).sum()) for k in ('pi', 'sigma'))
    size = -dot * lr * state['c']
    if clipped:
        assert abs(size - nc) <= 1e-12 * nc
    else:
        assert state['c'] == 1.0 and 0 < size < nc


def test_ema_weights_after_k_steps():
    shapes, tree, factors = _toy(1.0)
    params = tree()
    state = ks.init_state(shapes, params)
    for k in range(1, 6):
        state, _ = ks.kfac_step(state, shapes, params, tree(), factors, tree(), 6, 0.05)
        assert abs(state['ema_weight'] - sum(0.95 ** i for i in range(k))) <= 1e-15 * k
        # constant input: the moving average's value is the input itself
        assert float((state['factors'][0][0] / state['ema_weight'] - factors[0][0]).abs().max()) <= 1e-14
    assert state['count'] == 5


def test_invert_every_keeps_the_inverses_between_updates():
    shapes, tree, factors = _toy(1.0)
    params = tree()
    state = ks.init_state(shapes, params)
    state, _ = ks.kfac_step(state, shapes, params, tree(), factors, tree(), 6, 0.05, invert_every=2)
    kept = state['inverses']
    state, _ = ks.kfac_step(state, shapes, params, tree(), factors, tree(), 6, 0.05, invert_every=2)
    assert state['inverses'] is kept
    state, _ = ks.kfac_step(state, shapes, params, tree(), factors, tree(), 6, 0.05, invert_every=2)
    assert state['inverses'] is not kept


def test_what_the_optimizer_refuses():
    from deepsolid_amd import kfac
    with pytest.raises(NotImplementedError, match='momentum'):
        kfac.kfac(0.05, momentum=0.9)
    with pytest.raises(NotImplementedError, match='adaptive'):
        kfac.kfac(0.05, adaptive_damping=True)
    with pytest.raises(NotImplementedError, match='register_only_generic'):
        kfac.kfac(0.05, register_only_generic=True)
    init, step = kfac.kfac(lambda t: 0.05)
    assert init({}) == {'count': 0, 'ema_weight': 0.0}
