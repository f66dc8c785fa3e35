"""CPU tests of the fixed-phase DMC (csrc/ds_dmc.h, deepsolid_amd/dmc.py): the exported symbols, the properties of the comb model
of tests/dmc_helpers.py, the blocking error bar, and the oracle-only conditions that keep the replay fixtures of test_gpu_dmc.py
meaningful (no GPU: the model runs on the CPU oracle)."""
import os
import re

import numpy as np
import pytest

import dmc_helpers as dh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('ds_dmc_workspace_bytes', 'ds_dmc_step', 'ds_dmc_noise', 'ds_dmc_branch_workspace_bytes', 'ds_dmc_branch')


def test_library_exports_and_header_declares_the_dmc_symbols():
    from deepsolid_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
        decl = re.search(r'\b' + n + r'\(([^;]*)\);', header)
        assert decl, f'{n} is not declared in include/deepsolid_hip.h'
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[n][1]), n          # as many arguments bound as declared
    assert lib.ds_dmc_workspace_bytes(None, 4) == -1
    assert lib.ds_dmc_branch_workspace_bytes(0, 4, 0) == -1 and lib.ds_dmc_branch_workspace_bytes(0, 4, 2 ** 20 + 1) == -1
    assert lib.ds_dmc_branch_workspace_bytes(0, 4, 2 ** 20) > lib.ds_dmc_branch_workspace_bytes(1, 4, 2 ** 20) > 0


def test_branch_refusals_need_no_device():
    """Every refusal of ds_dmc_branch comes before any launch, so it can be seen without a GPU."""
    from deepsolid_amd import _lib
    lib = _lib.load()
    one = 8                                    # any non-null address: nothing is dereferenced before the checks pass
    ok = dict(dtype=0, n=2, B=4, xi=0.5, ptrs=[one] * 6, par=None, ws=one, wsb=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ds_dmc_branch(a['dtype'], a['n'], a['B'], a['xi'], *a['ptrs'], a['par'], a['ws'], a['wsb'], None)
    for kw, text in ((dict(ptrs=[one, one, None, one, one, one]), 'null state pointer'), (dict(ws=None), 'null workspace'),
                     (dict(n=0), 'n_elec must be >= 1'), (dict(B=0), 'B must be in 1..1048576'), (dict(B=2 ** 20 + 1), 'B must be in'),
                     (dict(xi=1.0), 'xi must be in [0, 1)'), (dict(xi=float('nan')), 'xi must be in'), (dict(xi=-0.1), 'xi must be in'),
                     (dict(wsb=16), 'workspace too small for ds_dmc_branch')):
        assert call(**kw) == 1, kw
        assert text in lib.ds_last_error().decode(), (kw, lib.ds_last_error())


# ---------------------------------------------------------------------------------------------------------------- the comb model
@pytest.mark.parametrize('B', [1, 5, 64, 257, 700])
def test_comb_model_weights_and_copy_counts(B):
    rng = np.random.default_rng(B)
    w = rng.lognormal(0.0, 1.0, B)
    w[rng.random(B) < 0.2] = 0.0
    if not w.any():
        w[0] = 1.0
    for xi in (0.0, 0.37, 1.0 - 2.0 ** -53):
        c = dh.comb(w, xi)
        assert c['run'] and c['W'] == dh.prefix_sums(w)[-1] and c['step'] == c['W'] / B       # new weights are all W / B
        copies = np.bincount(c['parents'], minlength=B)
        assert copies.sum() == B and (np.diff(c['parents']) >= 0).all()
        share = B * w / c['W']
        assert (copies >= np.floor(share - 1e-9)).all() and (copies <= np.ceil(share + 1e-9)).all(), (xi, copies, share)
        assert (copies[w == 0.0] == 0).all()


@pytest.mark.parametrize('B', [1, 2, 63, 256, 257, 1000])
def test_comb_model_identity_and_one_hot(B):
    # (weights whose sums are exact, so that xi = 0 puts every tooth exactly on an edge: '<=' then counts that edge, as stated;
    #  after a comb every weight is W / B, and for sums that round the edge case xi = 0 has probability 2^-53)
    for weight in (1.0, 0.75, 2.0 ** -10):
        for xi in (0.0, 0.5, 1.0 - 2.0 ** -53):
            assert np.array_equal(dh.comb(np.full(B, weight), xi)['parents'], np.arange(B)), (B, weight, xi)
    for hot in sorted({0, B // 2, B - 1}):
        w = np.zeros(B)
        w[hot] = 2.5
        for xi in (0.0, 0.5, 1.0 - 2.0 ** -53):
            assert (dh.comb(w, xi)['parents'] == hot).all(), (B, hot, xi)


def test_comb_model_skips_a_total_that_is_not_positive_or_not_finite():
    for w in (np.zeros(5), np.array([1.0, np.nan, 2.0]), np.array([1.0, np.inf])):
        c = dh.comb(w, 0.3)
        assert not c['run'] and np.array_equal(c['parents'], np.arange(len(w)))


def test_prefix_sums_follow_the_documented_order():
    """Sequential inside chunks of 256, chunk offsets sequential, then offset + running sum: different bits from one sequential
    sum over all walkers, which is what the device must NOT be compared with."""
    w = np.random.default_rng(3).lognormal(0.0, 1.0, 700)
    C = dh.prefix_sums(w)
    assert np.array_equal(C[:256], np.cumsum(w[:256]))
    off1 = np.cumsum(w[:256])[-1]
    assert np.array_equal(C[256:512], off1 + np.cumsum(w[256:512]))
    assert np.array_equal(C[512:], (off1 + np.cumsum(w[256:512])[-1]) + np.cumsum(w[512:]))
    assert not np.array_equal(C, np.cumsum(w)) and np.allclose(C, np.cumsum(w), rtol=1e-13)


# ------------------------------------------------------------------------------------------------------------------- reblocking
def test_reblock_on_an_ar1_series_with_known_variance():
    """x_t = phi x_{t-1} + eps: the variance of the mean of n samples tends to sigma_x^2 (1 + phi) / ((1 - phi) n).  The blocking
    error must come out near it (within 25 % at n = 2^16, phi = 0.9: the statistical spread of the estimate at a block length
    of a few hundred) and far above the naive error, which is too small by sqrt((1 + phi) / (1 - phi)) = 4.4."""
    from deepsolid_amd import dmc
    phi, n = 0.9, 2 ** 16
    rng = np.random.default_rng(11)
    eps = rng.normal(size=n)
    x = np.empty(n)
    x[0] = eps[0] / np.sqrt(1 - phi ** 2)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + eps[t]
    mean, err, length = dmc.reblock(3.0 + x)
    exact = np.sqrt(1.0 / (1 - phi ** 2) * (1 + phi) / (1 - phi) / n)
    naive = np.sqrt(x.var(ddof=1) / n)
    assert abs(mean - (3.0 + x.mean())) < 1e-12
    assert abs(err - exact) < 0.25 * exact, (err, exact)
    assert err > 3.0 * naive and length >= 32
    m, e, _ = dmc.reblock(rng.normal(size=4096))                # white noise: the naive error
    assert abs(e - 1 / 64) < 0.25 / 64
    assert np.isnan(dmc.reblock([1.0])[1])


def test_state_round_trip_and_refusals(tmp_path):
    from deepsolid_amd import dmc
    import torch
    arrays = dict(x=torch.arange(12.0, dtype=torch.float64).reshape(2, 6), logabs=torch.tensor([0.5, -1.0], dtype=torch.float64),
                  phase=torch.tensor([[1.0, 0.0], [0.6, 0.8]], dtype=torch.float64), drift=torch.ones(2, 6, dtype=torch.float64),
                  eloc=torch.tensor([-1.0, -2.0], dtype=torch.float64), weight=torch.tensor([1.0, 0.25], dtype=torch.float64))
    st = dmc.DmcState(arrays, e_trial=-1.25, e_ref=-1.5, tau_eff=0.0099, offset=2 ** 40 + 7, valid=True, sum_w=12.5, sum_we=-17.0)
    st.save(tmp_path / 's.npz')
    back = dmc.DmcState.load(tmp_path / 's.npz', device='cpu')
    for k in arrays:
        assert torch.equal(back.arrays[k], arrays[k]) and back.arrays[k].dtype == arrays[k].dtype
    assert (back.e_trial, back.e_ref, back.tau_eff, back.offset, back.valid, back.sum_w, back.sum_we) == \
        (-1.25, -1.5, 0.0099, 2 ** 40 + 7, True, 12.5, -17.0)
    assert abs(dmc.default_e_cut(4, 0.01) - 4.0) < 1e-12
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        dmc.make_dmc_step(None, None, 0.01, 10, pseudopotential=object())


# ------------------------------------------------------------------------------------ the conditions of the GPU replay fixtures
# What tools/find_dmc_seeds.py printed for the seeds in dmc_helpers.REPLAYS (seed 1 everywhere):
#   lih24        min |A - log u| 1.7e-02, min tooth distance 4.5e-05 W, 81 accepted, 15 rejected, 67 crossings, 86 clipped, 1 duplicated
#   bcc_li8      min |A - log u| 2.7e-01, min tooth distance 8.5e-03 W, 13 accepted, 3 rejected, 27 crossings, 14 clipped, 1 duplicated
@pytest.mark.parametrize('key', list(dh.REPLAYS))
def test_replay_fixture_conditions(key):
    """No undecidable accept decision (|A - log u| above the tolerance on A), no undecidable tooth (distance from every tooth to
    every cumulative edge, over W, above the weight tolerance), and every kind of event happens: an acceptance, a rejection, an
    electron brought back across a cell face, a clipped energy, a duplicated parent and a killed walker.  No decision is skipped."""
    c = dh.replay_reference(key)['cond']
    print(key, c)
    dh.assert_conditions(c)


def test_node_fixture_conditions():
    """At least one proposal of the node_mode fixture changes the sign of psi and would be accepted otherwise."""
    r = dh.node_reference()
    c = r['cond']
    print(c)
    assert c['undecidable'] == 0 and c['crossing_accepted'] >= 1, c
    free, fixed = r['free']['steps'][0], r['fixed']['steps'][0]
    w = c['walkers']
    assert free['acc'][w].all() and not fixed['acc'][w].any() and (fixed['p'][w] == 0).all()
    rest = np.setdiff1d(np.arange(r['B']), np.nonzero(free['overlap'] < 0)[0])
    assert np.array_equal(free['acc'][rest], fixed['acc'][rest])


def test_float32_fixture_conditions():
    c = dh.f32_reference()['cond']
    print(c, dh.f32_reference()['tol_a'])
    assert c['undecidable'] == 0 and c['accepted'] >= 1, c
