"""CPU side of test_gpu_ratios_large.py (no GPU): the sliced oracle evaluator against the one-vmap call it replaces, the oracle's
ratios of exactly the samples the GPU tests take on the large cells (finite, their |q| range), the pair counts and cutoff margins
of the two large pseudopotential cases, how far the oracle's ratios move when the inputs move in their last places (the evidence
that the float64 tolerance of the GPU tests is not eaten by the inputs), and what the float32 oracle loses by itself.

Measured (8 threads, whole file in 16 s): conditioning at most 4.9e-4 TOL_Q (graphene_331; graphene 1.5e-4, diamond 5.3e-5,
bcc_li_333 6.2e-5); float32 oracle loss 3.8e-4 (diamond) and 2.1e-4 (bcc_li_333); one-body |q| from 3.1e-4 to 1.4e3."""
import numpy as np
import pytest
import torch

import ecp_helpers as eh
import onebody_helpers as oh
import ratios_large_helpers as rl
import sampler_helpers as sh
import spin_helpers as sp


def unsliced(o, xs):
    """The call the helpers made before `Oracle.logdet`: every configuration through one vmap."""
    with o._ctx(), torch.no_grad():
        return torch.func.vmap(lambda y: o.ld.apply(o.p, y))(o._x(np.asarray(xs, dtype=np.float64)))


def close(q, q_old):
    return np.all(np.abs(q - q_old) <= 1e-12 * np.maximum(1.0, np.abs(q_old)))


# ------------------------------------------------------------------------------------------------ 1. the sliced evaluator
@pytest.mark.parametrize('name', ['lih', 'bcc_li'])
def test_sliced_evaluator_equals_the_unsliced_call(name):
    """The configurations of the one-body, spin and pseudopotential ratios of the existing cases through `Oracle.logdet` in slices
    of 8 (what the large cells get) against one vmap over all of them: the ratios differ by the summation order of a batched
    product at most, 1e-12 max(1, |q|).  The helpers themselves keep one vmap below 48 electrons: their ratios are the old bits."""
    fx, cell, _, _, _ = sh.case(name)
    o = sh.oracle(name)
    x = np.asarray(fx['x'], dtype=np.float64)
    nelec = tuple(int(v) for v in cell.nelec)
    N, P = sum(nelec), nelec[0] * nelec[1]
    B = len(x)
    l0 = unsliced(o, x)
    assert close(np.exp(o.logdet(x, step=3).numpy()), np.exp(l0.numpy()))
    s, _ = oh.replay_shifts(rl.SEED, rl.OFFSET, B, N + 1, cell.a)
    f = eh.fixture(name)
    rot = eh.replay_rotations(eh.SEED, eh.OFFSET, B)
    we = np.repeat(f['pairs']['w'], 12)
    passes = [('one-body', oh.displaced(x, s, N - 1).reshape(B * (N + 1), -1), np.repeat(np.arange(B), N + 1),
               lambda: oh.oracle_ratios(o, x, s, N - 1).reshape(-1)),
              ('spin', sp.swapped(x, nelec).reshape(B * P, -1), np.repeat(np.arange(B), P),
               lambda: sp.oracle_ratios(o, x, nelec, P, 0).reshape(-1)),
              ('pseudopotential', eh.displaced(x, f['pairs'], rot, 12), we,
               lambda: eh.oracle_ratios(o, x, eh.displaced(x, f['pairs'], rot, 12), we))]
    for what, cfg, w, helper in passes:
        assert len(cfg) > 8
        w = torch.as_tensor(w)
        old = np.exp((unsliced(o, cfg) - l0[w]).numpy())
        new = np.exp((o.logdet(cfg, step=8) - o.logdet(x, step=8)[w]).numpy())
        print(f'{name} {what}: {len(cfg)} configurations, max scaled |q_sliced - q_unsliced| = {rl.scaled(new, old).max():.2e}')
        assert close(new, old), what
        assert np.array_equal(helper(), old), what
    # a wrapped subset of the pairs is the same columns
    M = min(P, 5) + 2
    allq = sp.oracle_ratios(o, x, nelec, P, 0)
    assert close(sp.oracle_ratios(o, x, nelec, M, P - 2), allq[:, sp.pair_indices(M, nelec, P - 2)])


# ------------------------------------------------------------------------------------------------ 2. the samples of the GPU tests
@pytest.mark.parametrize('name', rl.ONEBODY_CELLS)
def test_onebody_samples_of_the_large_cells_are_finite(name):
    """M = N + 1 from N - 1: every electron once, the index wraps, both spins; 2 (N + 1) configurations, neither a multiple of 80
    nor of 64.  On bcc_li_333 the up electrons take 41 + 41 samples, the down electrons 2 x 40."""
    ref, M, first = rl.onebody_reference(name)
    N = sum(ref['nelec'])
    assert ref['q'].shape == (rl.WALKERS, N + 1) and (2 * M) % 80 and (2 * M) % 64 and 2 * M <= 218
    assert sorted(set(oh.electrons(M, N, first))) == list(range(N))
    print(f'{name} one-body: {rl.q_range(ref["q"])}')
    assert np.all(np.isfinite(ref['q']))
    if name == 'bcc_li_333':
        assert oh.samples_per_spin(rl.WALKERS, M, first, ref['nelec']).tolist() == [82, 82] and ref['nelec'] == (41, 40)


@pytest.mark.parametrize('name', rl.SPIN_CELLS)
def test_spin_samples_of_the_large_cells_are_finite(name):
    ref, M, first = rl.spin_reference(name)
    nu, nd = ref['nelec']
    assert ref['q'].shape == (rl.WALKERS, 130) and first + M > nu * nd
    print(f'{name} spin: {rl.q_range(ref["q"])}')
    assert np.all(np.isfinite(ref['q']))
    if name == 'bcc_li_333':
        # with the roles of n_up and n_dn confused (i = p / n_up) a sample would exchange another pair
        p = sp.pair_indices(M, (nu, nd), first)
        wrong = np.stack([p // nu, nu + p % nu], axis=1)
        assert (nu, nd) == (41, 40) and np.any(wrong != sp.pairs((nu, nd))[p])


@pytest.mark.parametrize('name,n_quad', rl.ECP_RULES)
def test_ecp_cases_of_the_large_cells(name, n_quad):
    """Two walkers, r_cut 1.2 Bohr: pairs [17, 18] (diamond, nearest distance to a cutoff 2.2e-3 Bohr, half the smallest height
    3.89) and [5, 9] (bcc_li_333: 4.7e-3, 6.87); the oracle's ratios of every configuration are finite."""
    ref = rl.ecp_reference(name, n_quad)
    r_cut, counts = eh.LARGE_CASES[name]
    assert ref['pairs']['counts'].tolist() == counts == {'diamond': [17, 18], 'bcc_li_333': [5, 9]}[name]
    r, _, _ = eh.min_image(ref['x'], ref['ecp'].atoms, ref['ecp'].a)
    margin = min(np.abs(r - rc).min() for rc in (r_cut, eh.LOCAL_FRACTION * r_cut))
    half = 0.5 * eh.heights(ref['cell'].a).min()
    print(f'{name}: nearest distance to a cutoff {margin:.2e} Bohr, half the smallest height {half:.3f} Bohr, {rl.q_range(ref["q"])}')
    want_margin, want_half = {'diamond': (2.2e-3, 3.89), 'bcc_li_333': (4.7e-3, 6.87)}[name]
    assert abs(margin - want_margin) < 0.05e-3 and margin > eh.CUTOFF_MARGIN and abs(half - want_half) < 0.005
    assert ref['q'].shape == (sum(counts) * n_quad,) and np.all(np.isfinite(ref['q']))
    assert ref['e_loc_terms'].sum() > 0


def test_float32_samples_of_diamond_are_finite_and_keep_their_pairs():
    ob, M, first = rl.onebody_reference('diamond', True)
    assert set(oh.electrons(M, 96, first) >= 48) == {False, True}
    spn, _, _ = rl.spin_reference('diamond', True)
    ecp = rl.ecp_reference('diamond', 12, True)                        # (asserts the float64 counts and the margin at the rounded walkers)
    assert ecp['pairs']['counts'].tolist() == eh.LARGE_CASES['diamond'][1]
    for what, q in (('one-body', ob['q']), ('spin', spn['q']), ('pseudopotential', ecp['q'])):
        print(f'diamond float32 {what}: {rl.q_range(q)}')
        assert np.all(np.isfinite(q))


# ------------------------------------------------------------------------------------------------ 3. conditioning
@pytest.mark.parametrize('name', rl.ONEBODY_CELLS)
def test_ratios_move_little_when_the_inputs_move_in_their_last_places(name):
    """x and s moved by +-2 and +-4 ulp, 2 x 24 samples: the oracle's q moves by less than 1e-2 TOL_Q max(1, |q|), so the float64
    tolerance of the GPU tests is not spent on how the inputs are rounded.  Measured: at most 4.9e-4 TOL_Q (graphene_331)."""
    worst, mag = rl.onebody_conditioning(name)
    print(f'{name}: q moves by {worst / rl.TOL_Q:.2e} TOL_Q at most, |q| in [{mag.min():.3g}, {mag.max():.3g}]')
    assert worst < 1e-2 * rl.TOL_Q


# ------------------------------------------------------------------------------------------------ 4. float32 by itself
@pytest.mark.parametrize('name', ['diamond', 'bcc_li_333'])
def test_float32_oracle_loss_is_inside_the_float32_tolerance(name):
    """The float32 oracle against the float64 oracle at the same float32-rounded configurations, 48 one-body samples.  Measured:
    3.8e-4 (diamond), 2.1e-4 (bcc_li_333) of max(1, |q|); TOL_Q_F32 is 1.4e-2."""
    loss = rl.onebody_f32_oracle_loss(name)
    print(f'{name}: float32 oracle loss {loss:.2e} (TOL_Q_F32 {rl.TOL_Q_F32:.1e})')
    assert loss < rl.TOL_Q_F32


# ------------------------------------------------------------------------------------------------ 5. the batches
def test_distinct_walkers_are_distinct_inside_the_cell_and_stable():
    fx, cell, _, _, _ = sh.case('lih')
    x = rl.lih_walkers(2100)
    assert x.shape == (2100, 12) and len(np.unique(x, axis=0)) == 2100
    frac = x.reshape(2100, 4, 3) @ np.linalg.inv(np.asarray(cell.a, dtype=np.float64).reshape(3, 3))
    assert frac.min() >= 0 and frac.max() <= 1
    assert np.array_equal(sh.distinct_walkers(cell, fx['x'], 275), x[:275])          # a slice of a batch is the smaller batch
    t = sh.tiled_walkers(cell, fx['x'], 2100)
    d = (x - t).reshape(2100, 4, 3) @ np.linalg.inv(np.asarray(cell.a, dtype=np.float64).reshape(3, 3))
    d = (d - np.round(d)) @ np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    assert np.abs(d).max() <= 0.05 + 1e-12 and np.abs(d).max() > 0.04


def test_big_batches_cross_what_they_are_meant_to_cross():
    ref = rl.ecp_big_reference()
    total = int(ref['off'][-1])
    w = ref['straddle']
    print(f'ECP batch: {total // 12} pairs, {total} configurations; walker {w} holds configuration 65520')
    assert total > 65520 and ref['off'][w] < 65520 < ref['off'][w + 1]
    assert np.isfinite(np.concatenate([ref['q'][v] for v in ref['check']])).all()
    ob = rl.onebody_big_reference()
    assert ob['q'].shape == (3, 61) and np.all(np.isfinite(ob['q']))
    spn = rl.spin_big_reference()
    assert spn['q'].shape == (4, 4) and np.all(np.isfinite(spn['q'])) and np.isnan(spn['x']).sum() == 2
