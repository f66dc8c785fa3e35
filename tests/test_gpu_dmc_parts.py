"""GPU tests of the kernels of one `ds_dmc_step` (csrc/ds_dmc.h) against tests/dmc_parts_helpers.py, which restates the step from
arrays: every input is the device's own (ds_local_energy, ds_logpsi_grad, ds_dmc_noise), so no CPU oracle is needed and the cases
are the ones the oracle replays of test_gpu_dmc.py cannot afford -- several stats groups and scan chunks, a last group of one
walker, more electrons than a wave has lanes, float32.  The uniforms are built so that every decision has the margin DELTA, which
the a-priori bound tol_A of `log_ratio` must stay ten times below; no decision is left out."""
import numpy as np
import pytest
import torch

import dmc_helpers as dh
import dmc_parts_helpers as ph
import sampler_helpers as sh
from test_gpu_dmc import KEYS, bits, clone, cu, same_bits, system

pytestmark = pytest.mark.gpu

DELTA = 0.01
SEED, OFFSET = 1, 0
# (case, dtype, B, tau, preset weights): what only this case runs is in the ids.  tau is the smallest of 0.1, 0.3, 0.5 at which the
# host's A rejects an odd walker (A + DELTA < 0): 0.1 in every case.  Above each the counts seen at that tau -- odd walkers with
# A + DELTA < 0, then accepted / rejected / clipped of the steered step -- and the largest tol_A.
CASES = [
    # 114 of 300; 483 / 117 / 551; tol_A 4.5e-13
    pytest.param('lih', torch.float64, 600, 0.1, 'ramp', id='lih-f64-600-three_groups_last_of_88-150_accept_workgroups-3_chunks'),
    # 40 of 128; 217 / 40 / 223; tol_A 3.9e-13
    pytest.param('lih_twist', torch.float64, 257, 0.1, 'ramp', id='lih_twist-f64-257-last_group_and_chunk_of_one-complex_phase'),
    # 12 of 18; 25 / 12 / 32; tol_A 4.3e-5 (float32: below DELTA / 10 = 1e-3 with DELTA as it is)
    pytest.param('bcc_li', torch.float32, 37, 0.1, None, id='bcc_li-f32-37-float_branch-72_coordinates'),
    # 1 of 1; 2 / 1 / 3; tol_A 9.4e-11
    pytest.param('diamond', torch.float64, 3, 0.1, None, id='diamond-f64-3-96_electrons_second_lane_pass_of_32'),
    # 1 of 1; 1 / 1 / 2; tol_A 6.3e-11
    pytest.param('bcc_li_333', torch.float64, 2, 0.1, None, id='bcc_li_333-f64-2-81_electrons_second_lane_pass_of_17'),
]
KEYS5 = KEYS[:5]


def np64(t):
    return t.detach().double().cpu().numpy()


def eps_of(dtype):
    return 2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23


def parts_of(sysd, dp, x):
    """logabs, phase, eloc, drift as the separate entries give them on x: ds_local_energy (Re ke + ewald in float64) and the real
    part of ds_logpsi_grad."""
    ke, ew, la, ph_ = sysd.local_energy(dp, x, want_logpsi=True)
    la_g, g = sysd.logpsi_grad(dp, x)
    assert torch.equal(bits(la_g), bits(la))
    return dict(logabs=la, phase=ph_, eloc=ke[:, 0].double() + ew.double(), drift=g.real.contiguous())


def rows_equal(a, b, rows, keys=KEYS5):
    return same_bits({k: a[k][rows] for k in keys}, {k: b[k][rows] for k in keys}, keys)


def initialise(sysd, dp, x0, w0):
    """state_valid = 0 read off a step whose proposals are all refused as non-finite (NaN normals) at tau_eff = 0."""
    B = x0.shape[0]
    st = sysd.dmc_state(x0, w0)
    nan = torch.full((1, B, 3 * sysd.n), float('nan'), dtype=sysd.dtype, device='cuda')
    out = sysd.dmc_step(dp, st, 1, 0.05, tau_eff=0.0, normals=nan, uniforms=torch.full((1, B), 0.5, dtype=sysd.dtype, device='cuda'),
                        comb_uniforms=torch.zeros(1, dtype=torch.float64, device='cuda'), branch_every=0, state_valid=False)
    return st, out['stats'].cpu().numpy()[0]


def prepare(name, dtype, B, tau, wk):
    """Steps 1 to 3: the initial state, the forced-accept clone, the host's A and its bound, all asserted."""
    sysd, dp = system(name, dtype)
    cell = sh.case(name)[1]
    npT = np.float64 if dtype == torch.float64 else np.float32
    x0 = cu(dh.start_walkers(name, B, SEED), dtype)
    w0 = cu(dh.preset_weights(wk, B))
    # 1. the initialisation
    init, row = initialise(sysd, dp, x0, w0)
    assert row[3] == 0 and row[6] == B and row[4] == 0
    assert torch.equal(init['x'], x0) and same_bits(init, parts_of(sysd, dp, x0), KEYS5[1:]) == []
    assert torch.equal(init['weight'], w0)
    # 2. every proposal accepted
    nz, un, xi = sysd.dmc_noise(B, 1, SEED, OFFSET)
    forced = clone(init)
    row = sysd.dmc_step(dp, forced, 1, tau, normals=nz, uniforms=torch.full_like(un, 2.0 ** -60), comb_uniforms=xi, branch_every=0,
                        state_valid=True)['stats'].cpu().numpy()[0]
    assert row[3] == B and row[6] == 0 and bool((forced['x'] != x0).any(1).all())
    want = ph.proposal(cell, np64(init['x']), np64(init['drift']), np64(nz[0]), tau, npT)
    dx = ph.min_image_distance(cell, np64(forced['x']), want)
    L = ph.longest_cell_vector(cell)
    print(f'{name} B {B} tau {tau}: max |x_after - proposal| {dx.max():.3e}, bound {16 * eps_of(dtype) * L:.3e}')
    assert dx.max() <= 16 * eps_of(dtype) * L
    assert same_bits(forced, parts_of(sysd, dp, forced['x']), KEYS5[1:]) == []
    # 3. the host's ratio from the device's arrays
    A, tol_A = ph.log_ratio(np64(init['logabs']), np64(forced['logabs']), np64(init['drift']), np64(forced['drift']), np64(nz[0]), tau, npT)
    odd = np.arange(B) % 2 == 1
    print(f'{name} B {B} tau {tau}: max tol_A {tol_A.max():.3e}, A in [{A.min():.3f}, {A.max():.3f}], '
          f'odd walkers with A + delta < 0: {int((A[odd] + DELTA < 0).sum())} of {int(odd.sum())}')
    assert np.isfinite(A).all() and tol_A.max() < DELTA / 10
    return dict(sysd=sysd, dp=dp, cell=cell, npT=npT, x0=x0, w0=w0, init=init, forced=forced, nz=nz, xi=xi, A=A, tol_A=tol_A)


def steered_uniforms(A, npT):
    """Even walkers u = exp(A - DELTA), capped below 1: accept.  Odd walkers u = exp(A + DELTA) where that is below 1: reject, else
    the largest u below 1.  Rounded to T; -> (u (B,) in T, log u of the rounded value)."""
    below_one = 1.0 - np.finfo(npT).epsneg
    odd = np.arange(len(A)) % 2 == 1
    with np.errstate(over='ignore'):
        u = np.where(odd, np.where(A + DELTA < 0, np.exp(A + DELTA), below_one), np.minimum(np.exp(A - DELTA), below_one))
    u = np.minimum(u.astype(npT), npT(below_one))
    with np.errstate(divide='ignore'):
        return u, np.log(u.astype(np.float64))


def steered_step(p, state, u, e_ref, e_cut, tau, **kw):
    out = p['sysd'].dmc_step(p['dp'], state, 1, tau, e_trial=e_ref, e_ref=e_ref, e_cut=e_cut, normals=p['nz'],
                             uniforms=cu(u[None, :], p['sysd'].dtype), comb_uniforms=p['xi'], **kw)
    return out, out['stats'].cpu().numpy()[0]


def check_row(row, state, e_ref, e_cut, accepted, nonfinite, B):
    """The integer columns, and columns 0, 1, 2, 7 bit for bit against the tree of dmc_parts_helpers."""
    cols, clipped = ph.stats_from_state(np64(state['weight']), np64(state['eloc']), e_ref, e_cut)
    assert (row[3], row[5], row[6], row[8]) == (accepted, clipped, nonfinite, B), (row, accepted, clipped, nonfinite)
    assert np.array_equal(row[[0, 1, 2, 7]].view(np.int64), cols.view(np.int64)), (row[[0, 1, 2, 7]], cols)
    return clipped


@pytest.mark.parametrize('name, dtype, B, tau, wk', CASES)
def test_step_against_its_parts(name, dtype, B, tau, wk):
    p = prepare(name, dtype, B, tau, wk)
    sysd, dp, init, forced, A, tol_A = p['sysd'], p['dp'], p['init'], p['forced'], p['A'], p['tol_A']
    # 4. steered decisions
    u, logu = steered_uniforms(A, p['npT'])
    expect = A > logu
    assert (np.abs(A - logu) > tol_A).all(), np.abs(A - logu).min()              # decidable (an odd walker with A near 0 could miss it)
    e0 = np64(init['eloc'])
    e_ref = float(np.round(e0.mean(), 3))
    e_cut = 0.05 * np.sqrt(sysd.n / tau)
    st = clone(init)
    _, row = steered_step(p, st, u, e_ref, e_cut, tau, branch_every=0, state_valid=True)
    mask = (st['x'] != init['x']).any(1).cpu().numpy()
    assert np.array_equal(mask, expect), (mask, expect, A, logu)
    acc, rej = cu(expect, torch.bool), cu(~expect, torch.bool)
    assert rows_equal(st, forced, acc) == [] and rows_equal(st, init, rej) == []
    w_want = ph.weights_after(np64(init['weight']), np64(st['eloc']), e0, tau, e_ref, e_ref, e_cut)
    assert (np.abs(np64(st['weight']) - w_want) <= 4 * ph.EPS * w_want).all()
    clipped = check_row(row, st, e_ref, e_cut, int(expect.sum()), 0, B)
    p_sum = np.minimum(1.0, np.exp(np.minimum(A, 0.0))).sum()
    assert abs(row[4] - p_sum) <= B * (tol_A.max() + 4 * ph.EPS), (row[4], p_sum)
    print(f'{name} B {B} tau {tau}: accepted {int(expect.sum())}, rejected {int((~expect).sum())}, clipped {clipped}')
    assert expect.any() and (~expect).any() and clipped >= 1
    if B == 600:
        for g0 in range(0, B, ph.GROUP):
            assert expect[g0:g0 + ph.GROUP].any() and (~expect[g0:g0 + ph.GROUP]).any(), g0
        # 5. two walkers with a NaN coordinate, one in the first group and the last walker of the partial group
        bad = p['x0'].clone()
        bad[5, 4] = float('nan')
        bad[599, 0] = float('nan')
        dirty = sysd.dmc_state(bad, p['w0'])
        _, drow = steered_step(p, dirty, u, e_ref, e_cut, tau, branch_every=0, state_valid=False)
        keep = np.ones(B, bool)
        keep[[5, 599]] = False
        assert float(dirty['weight'][5]) == 0.0 and float(dirty['weight'][599]) == 0.0 and np.isfinite(drow[:8]).all()
        assert rows_equal(dirty, st, cu(keep, torch.bool), KEYS) == []
        check_row(drow, dirty, e_ref, e_cut, int(expect[keep].sum()), 2, B)
        p_keep = np.minimum(1.0, np.exp(np.minimum(A[keep], 0.0))).sum()             # (a non-finite proposal has p = 0)
        assert abs(drow[4] - p_keep) <= B * (tol_A.max() + 4 * ph.EPS), (drow[4], p_keep)
    # 6. the same step with the comb fused
    fused = clone(init)
    out, frow = steered_step(p, fused, u, e_ref, e_cut, tau, branch_every=1, state_valid=True, want_parents=True)
    xi = float(p['xi'][0])
    c = dh.comb(np64(st['weight']), xi)
    parents = out['parents'].cpu().numpy()[0]
    assert c['run'] and np.array_equal(parents, c['parents'])
    split = clone(st)
    assert np.array_equal(sysd.dmc_branch(split, xi).cpu().numpy(), parents)
    assert same_bits(fused, split) == []
    assert frow[8] == len(np.unique(parents)) and np.array_equal(frow[:8].view(np.int64), row[:8].view(np.int64))
    if wk is not None:
        assert len(np.unique(parents)) < B
