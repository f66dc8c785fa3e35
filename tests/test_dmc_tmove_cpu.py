"""CPU tests of the numpy model of DMC with T-moves (dmc_tmove_helpers.py): the heat-bath choice of step 6 of `ds_dmc_step_tmove` on
terms given by hand, and the oracle-only conditions of the replay that test_gpu_dmc_tmove.py compares the device against."""
import numpy as np
import pytest

import dmc_ecp_helpers as deh
import dmc_helpers as dh
import dmc_tmove_helpers as th

TAU = 0.1
# real and complex terms with both signs; interval widths tau |Re term| from 1e-4 to 0.3
TERMS = np.asarray([0.4, -1.2, 0.0, -0.001, 2.5, -3.0, -0.25, 0.7, -0.6 + 2.0j, 0.3 - 1.0j, -1e-2 - 5.0j, 1.1])
NEG = [c for c, t in enumerate(TERMS) if t.real < 0]


def test_u_zero_stays():
    assert th.heat_bath(TERMS, TAU, 0.0) == -1
    assert th.heat_bath(TERMS[:0], TAU, 0.9) == -1


def test_no_negative_term_stays_for_every_u():
    terms = np.abs(TERMS.real) + 1j * TERMS.imag
    for u in (0.0, 0.3, 0.999, 1.0 - 2.0 ** -53):
        assert th.heat_bath(terms, TAU, u) == -1


def test_the_midpoint_of_every_interval_picks_its_configuration():
    """For a complex term the real part decides; a term with Re >= 0 has an empty interval and is never picked."""
    t, r = th.intervals(TERMS, TAU)
    assert r[0] == 1.0 and r[-1] == pytest.approx(1.0 + TAU * sum(-TERMS[c].real for c in NEG))
    assert th.heat_bath(TERMS, TAU, th.midpoint(TERMS, TAU, -1)[0]) == -1
    for c in NEG:
        u, half = th.midpoint(TERMS, TAU, c)
        assert half > 0 and th.heat_bath(TERMS, TAU, u) == c
    for u in np.linspace(0.0, 1.0, 997, endpoint=False):
        assert th.heat_bath(TERMS, TAU, u) in [-1] + NEG


def test_theta_rounded_onto_z_is_clamped_to_the_last_positive_interval():
    """theta = Z: every r_c <= theta, the count is n, and the choice is the last configuration with t_c > 0, not the non-negative
    terms behind it.  (For Z in [2^k, 2^(k+1)) the largest uniform below 1, 1 - 2^-53, gives u Z = Z - Z 2^-53, at least half an
    ulp (2^(k-53)) below Z and exactly representable where it is a tie, so a Philox uniform never rounds onto Z; the clamp is what
    keeps an explicit uniform of 1 inside the walker's configurations.)"""
    terms = np.asarray([-3.0, 0.5, -2.0, 0.25, 0.0])
    _, r = th.intervals(terms, TAU)
    assert (1.0 - 2.0 ** -53) * r[-1] < r[-1] and th.heat_bath(terms, TAU, 1.0 - 2.0 ** -53) == 2
    assert 1.0 * r[-1] == r[-1] and th.heat_bath(terms, TAU, 1.0) == 2


def test_frequencies_match_the_heat_bath_probabilities():
    """10^5 uniforms.  The count n_c of an outcome of probability p_c = t_c / Z (1 / Z for no move) is binomial with variance
    N p_c (1 - p_c); the bound is 5 standard deviations plus 1, which 13 independent outcomes all meet with probability
    1 - 13 x 5.7e-7: a failure means a wrong choice, not bad luck."""
    N = 100000
    t, r = th.intervals(TERMS, TAU)
    Z = r[-1]
    u = np.random.default_rng(20250101).random(N)
    got = np.asarray([th.heat_bath(TERMS, TAU, v) for v in u])
    for c, p in [(-1, 1.0 / Z)] + [(c, t[c] / Z) for c in NEG]:
        n = int((got == c).sum())
        assert abs(n - N * p) <= 5.0 * np.sqrt(N * p * (1.0 - p)) + 1.0, (c, n, N * p)
    assert set(got.tolist()) <= set([-1] + NEG)


def test_the_replay_trajectory_meets_its_conditions():
    """The lih replay on the oracle: at least one T-move, one rejected walker that is then evaluated where it stands, one walker that
    dies, and every Metropolis decision, comb tooth and T-move choice decidable."""
    ref = th.replay_reference(th.NAME)
    c = ref['cond']
    th.assert_conditions(c)
    s0 = ref['steps'][0]
    assert s0['w_commit'][th.DEAD] == 0.0 and s0['choice'][th.DEAD] == -1
    # a walker that made a T-move differs from x_cur in exactly one electron, and its eloc is the chain energy at the new position
    for s in ref['steps']:
        for k, e, point in s['moved']:
            assert s['choice'][k] >= 0
    assert all(np.isfinite(ref['state'][k]).all() for k in th.KEYS7)


@pytest.mark.parametrize('name, B', th.STEER_CASES)
def test_the_steered_inputs_stay_within_the_skip_cap(name, B):
    """The inputs of test_gpu_dmc_tmove.test_the_choice_is_steered on the oracle: at most a quarter of the walkers have a target
    interval narrower than 10 x the a-priori bound, and every kind of target (stay, first, last, middle) is hit."""
    ecp = deh.potential(name)
    orc = th.TmoveOracle(name, ecp, th.STEER_ROT[0])
    x0 = dh.start_walkers(name, B, th.STEER_WALKERS)
    aux = orc.evaluate(x0, th.STEER_ROT[1])[-1]
    target, u, skipped = th.steer_all(aux['terms'], aux['scales'], aux['pl']['counts'], ecp.n_quad, th.STEER_TAU, deh.tol_q())
    assert int(skipped.sum()) <= B // 4, skipped
    moved = np.nonzero(target >= 0)[0]
    assert len(moved) >= min(3, B - 2) and (target[np.arange(B) % 4 == 0] == -1).all()
    assert ((u >= 0.0) & (u < 1.0)).all()
    for w in moved:                                        # the model picks its own target
        p0, terms, _ = th.walker_terms(aux, w, ecp.n_quad)
        assert th.heat_bath(terms, th.STEER_TAU, u[w]) == target[w]
