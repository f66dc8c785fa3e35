"""CPU tests of tests/dmc_parts_helpers.py, the array-level restatement of one DMC step that test_gpu_dmc_parts.py holds the
kernels to: against the numpy model of dmc_helpers.py on the `lih24` replay (two steps without a comb, so that the state after a
step is the one its row was formed from), and the summation order of `tree_rows` on hand-built inputs."""
import functools

import numpy as np

import dmc_helpers as dh
import dmc_parts_helpers as ph

EPS = ph.EPS


@functools.lru_cache(maxsize=None)
def model_run():
    name, B, tau, _, seed, wk = dh.REPLAYS['lih24']
    orc = dh.dmc_oracle(name)
    x0 = dh.start_walkers(name, B, seed)
    e_ref = float(np.round(np.mean(orc.evaluate(x0)[3]), 3))
    e_cut = 0.05 * np.sqrt(orc.n / tau)
    runs = [dh.run_model(orc, x0, dh.preset_weights('ramp', B), steps, tau, tau, e_ref, e_ref, e_cut, 0, 0, seed, 0) for steps in (1, 2)]
    return dict(orc=orc, tau=tau, e_ref=e_ref, e_cut=e_cut, runs=runs, B=B)


def test_log_ratio_equals_the_models_within_its_own_bound():
    m = model_run()
    orc, tau = m['orc'], m['tau']
    seen = 0
    for s in m['runs'][1]['steps']:
        la, _, dr, _, _ = orc.evaluate(s['x_prev'])
        la2, _, dr2, _, _ = orc.evaluate(s['x_prop'])
        A, tol = ph.log_ratio(la, la2, dr, dr2, s['chi'], tau)
        print('max |A - model A|', np.abs(A - s['A']).max(), 'max tol_A', tol.max(), 'min tol_A', tol.min())
        assert (np.abs(A - s['A']) <= tol).all() and tol.max() < 1e-10 and (tol > 0).all()
        seen += len(A)
    assert seen == 2 * m['B']


def test_proposal_equals_the_models():
    m = model_run()
    orc, tau = m['orc'], m['tau']
    L = ph.longest_cell_vector(orc.cell)
    for s in m['runs'][1]['steps']:
        dr = orc.evaluate(s['x_prev'])[2]
        xp = ph.proposal(orc.cell, s['x_prev'], dr, s['chi'], tau)
        print('max |proposal - model x_prop|', np.abs(xp - s['x_prop']).max(), 'bound', 16 * EPS * L)
        assert np.abs(xp - s['x_prop']).max() <= 16 * EPS * L
        assert (ph.min_image_distance(orc.cell, xp, s['x_prop']) <= 16 * EPS * L).all()
    # the distance is up to lattice vectors, and only up to those
    a = np.asarray(orc.cell.a, dtype=np.float64).reshape(3, 3)
    x = m['runs'][0]['state']['x']
    moved = x.copy().reshape(len(x), -1, 3)
    moved[0, 1] += a[0] - 2 * a[2]
    moved[1, 0, 2] += 1e-3
    d = ph.min_image_distance(orc.cell, moved.reshape(len(x), -1), x)
    assert d[0] <= 16 * EPS * 3 * L and abs(d[1] - 1e-3) <= 1e-12 and (d[2:] == 0).all()


def test_stats_from_state_equals_the_models_row():
    m = model_run()
    for r in m['runs']:
        st, row = r['state'], r['steps'][-1]['row']
        w, e = st['weight'], st['eloc']
        cols, clipped = ph.stats_from_state(w, e, m['e_ref'], m['e_cut'])
        terms = (w, w * e, w * e * e, w * w)
        for got, j, t in zip(cols, (0, 1, 2, 7), terms):
            assert abs(got - row[j]) <= len(t) * EPS * np.abs(t).sum(), (j, got, row[j])
        assert clipped == row[5] and clipped >= 1
    # ... and weights_after is the model's update: one step from the preset weights
    r = m['runs'][0]
    s = r['steps'][0]
    e_old = r['state0']['eloc']
    e_new = np.where(s['acc'], s['e_prop'], e_old)
    want = ph.weights_after(dh.preset_weights('ramp', m['B']), e_new, e_old, m['tau'], m['e_ref'], m['e_ref'], m['e_cut'])
    assert (np.abs(want - r['state']['weight']) <= 4 * EPS * want).all() and s['acc'].any() and not s['acc'].all()


def test_stats_from_state_drops_the_energy_of_dead_walkers_and_counts_their_clips():
    w = np.array([1.0, 0.0, 2.0, 0.0, 0.5])
    e = np.array([-1.0, np.nan, 3.0, 9.0, -0.25])
    cols, clipped = ph.stats_from_state(w, e, 0.0, 2.0)
    assert np.array_equal(cols, [3.5, -1.0 + 6.0 - 0.125, 1.0 + 18.0 + 0.03125, 1.0 + 4.0 + 0.25])
    assert clipped == 2                                          # 3.0 and the 9.0 of a dead walker; the NaN is not clipped
    assert ph.stats_from_state(w, e, 0.0, 0.0)[1] == 0          # e_cut = 0 clips nothing
    epp = np.array([[1.0, 2.0, 3.0], [np.nan, np.nan, np.nan], [0.5, -1.0, 0.25], [7.0, 7.0, 7.0], [2.0, 0.0, -4.0]])
    assert np.array_equal(ph.ecp_stats_from_state(w, epp), [1.0 + 1.0 + 1.0, 2.0 - 2.0, 3.0 + 0.5 - 2.0])
    c, f = ph.clip(np.array([-3.0, -2.0, 0.5, 2.0, 2.5, np.nan]), 0.0, 2.0)
    assert np.array_equal(c[:5], [-2.0, -2.0, 0.5, 2.0, 2.0]) and np.isnan(c[5]) and f.tolist() == [True, False, False, False, True, False]


def test_tree_rows_is_exact_on_integers():
    rng = np.random.default_rng(5)
    for B in (1, 255, 256, 257, 600, 1000):
        v = rng.integers(-2 ** 20, 2 ** 20, size=(B, 3))
        assert np.array_equal(ph.tree_rows(v), v.sum(0).astype(np.float64)), B
        assert ph.tree_rows(v[:, 0]) == float(v[:, 0].sum())


def tree_by_the_text(v):
    """The statement of the order, walker by walker in plain Python floats."""
    total = 0.0
    for g0 in range(0, len(v), 256):
        sh = [float(t) for t in v[g0:g0 + 256]] + [0.0] * (256 - len(v[g0:g0 + 256]))
        s = 128
        while s >= 1:
            for t in range(s):
                sh[t] = sh[t] + sh[t + s]
            s //= 2
        total = total + sh[0]
    return total


def test_tree_rows_has_the_stated_group_structure():
    """300 terms (two groups, the last of 44) and 600 (three, the last of 88).  With 2^53 in place, a 1 added to it alone is lost and
    two 1s added together first are not: which of the two happens shows where the groups and the tree's pairs are."""
    big = 2.0 ** 53
    rng = np.random.default_rng(9)
    for B in (300, 600):
        r = rng.lognormal(0.0, 2.0, B) * rng.choice([-1.0, 1.0], B)
        assert ph.tree_rows(r) == tree_by_the_text(r)
    # inside group 0: the last level adds the even-thread subtotal and the odd-thread subtotal, so 1s at threads 1 and 3 meet first
    v = np.zeros(300)
    v[0], v[1], v[3] = big, 1.0, 1.0
    assert ph.tree_rows(v) == big + 2.0
    v[3], v[256] = 0.0, 1.0                                      # the same 1 in group 1: each is added to 2^53 alone
    assert ph.tree_rows(v) == big
    v[1], v[299] = 0.0, 1.0                                      # both in group 1 (the partial one): added together first
    assert ph.tree_rows(v) == big + 2.0
    # three groups, added in group order onto 0: (g0 + g1) + g2
    v = np.zeros(600)
    v[0], v[256], v[257] = big, 1.0, 1.0
    assert ph.tree_rows(v) == big + 2.0
    v[257], v[512] = 0.0, 1.0                                    # moved to group 2
    assert ph.tree_rows(v) == big
    v[256], v[599] = 0.0, 1.0                                    # both in group 2: 88 walkers, thread 87 the last
    assert ph.tree_rows(v) == big + 2.0
    v = np.zeros(600)
    v[511], v[0], v[1] = big, 1.0, 1.0                           # group 0 = 2, then + 2^53: the order of the groups, not of size
    assert ph.tree_rows(v) == big + 2.0
    v = np.zeros(600)
    v[0], v[300], v[599] = 1.0, big, 1.0                         # (1 + 2^53) + 1
    assert ph.tree_rows(v) == big
