"""GPU tests of DMC with a semi-local pseudopotential and Casula's T-moves: `ds_dmc_step_tmove` (csrc/ds_dmc.h, k_ecp_tmove of
csrc/ds_ecp.h; the algorithm as include/deepsolid_hip.h states it) against its parts -- `ds_dmc_step`, `ds_ecp_energy`,
`ds_local_energy`, `ds_dmc_branch` -- bit for bit, with the choice steered through `tmove_uniforms`, against the numpy model of
dmc_tmove_helpers.py on the CPU oracle, its bit identities, refusals and capacity semantics, and `inference.run_dmc(...,
tmoves=True)` end to end.  With the synthetic potential of ecp_helpers on lih and, for complex terms, on lih_twist and bcc_li."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import dmc_ecp_helpers as deh
import dmc_helpers as dh
import dmc_parts_helpers as ph
import dmc_tmove_helpers as th
import ecp_helpers as eh
import sampler_helpers as sh
from test_gpu_dmc import KEYS, TOL_X, bits, clone, cu, dev_params, phase_np, same_bits, system
from test_gpu_dmc_ecp import epp_of, midpoint_walkers, tables

pytestmark = pytest.mark.gpu

KEYS7 = deh.KEYS7
NAME = deh.NAME
B37 = 37                      # neither a multiple of the wave nor of the four-wave workgroup
KW = dict(e_trial=-8.0, e_ref=-8.0, e_cut=3.0)
F64 = dict(dtype=torch.float64, device='cuda')
PARTS = [('lih', B37, torch.float64), ('lih', B37, torch.float32), ('lih_twist', B37, torch.float64), ('bcc_li', 5, torch.float64)]
IDS = [f'{n}-{b}-{str(d)[6:]}' for n, b, d in PARTS]


def start(B, seed, dtype=torch.float64, name=NAME):
    return cu(dh.start_walkers(name, B, seed), dtype)


def device_rotations(sysd, dp, x, ecp, seed, counters):
    """The rotations a Philox-mode call draws for the counters (they depend on seed, counter and walker alone), from ds_ecp_energy."""
    return torch.stack([sysd.ecp_energy(dp, x, ecp, seed=seed, offset=c, want_rotations=True)['rotations'] for c in counters])


def explicit(sysd, B, steps, seed, o, rot, dtype=torch.float64, accept=None, tmove=None):
    """Explicit noise of `steps` steps from ds_dmc_noise(seed, o): `accept` True forces acceptance (u = 2^-60), False forces
    rejection (NaN normals: the proposal is not finite); `tmove`: the (steps, B) T-move uniforms (default: the Philox stream's)."""
    nz, un, xi = sysd.dmc_noise(B, steps, seed, o)
    if accept is True:
        un = torch.full_like(un, 2.0 ** -60)
    if accept is False:
        nz = torch.full_like(nz, float('nan'))
    tu = cu(th.tmove_uniforms(seed, o, steps, B)) if tmove is None else cu(tmove)
    return dict(normals=nz, uniforms=un, comb_uniforms=xi, rotations=rot, tmove_uniforms=tu)


def raw_step(sysd, ecp, dp, st, steps=1, tau=0.1, seed=0, offset=0, cap=None, state_valid=1, stats=None, skip=None, ecp_handle='tables',
             branch_every=0, noise=(None,) * 5):
    """The raw entry on a seven-array state -> (return code, steps_done, message)."""
    from deepsolid_amd.device import _ptr, _stream
    B = st['x'].shape[0]
    t = tables(sysd, ecp)
    cap = B * sysd.n * 2 if cap is None else cap
    ws = sysd._workspace('ds_dmc_tmove_workspace_bytes', t.handle, B, max(cap, 1))
    done = C.c_int(-1)
    ptrs = [None if k == skip else _ptr(st[k]) for k in KEYS7]
    rc = sysd.lib.ds_dmc_step_tmove(sysd.handle, t.handle if ecp_handle == 'tables' else ecp_handle, _ptr(sysd.pack_params(dp)), *ptrs, B,
                                    steps, tau, tau, KW['e_trial'], KW['e_ref'], KW['e_cut'], 0, branch_every, seed, offset,
                                    *[_ptr(t) for t in noise], cap, state_valid,
                                    _ptr(stats if stats is not None else torch.zeros(steps, 9, **F64)), None, None, None, None, None,
                                    C.byref(done), _ptr(ws), ws.numel(), _stream())
    return rc, done.value, sysd.lib.ds_last_error().decode()


def assert_same_call(a, ra, b, rb, keys=('stats', 'ecp_stats', 'energy')):
    assert same_bits(a, b, KEYS7) == []
    for k in keys:
        assert torch.equal(bits(ra[k]), bits(rb[k])), k
    for k in ('parents', 'pairs', 'tmoves'):
        assert (ra[k] is None and rb[k] is None) or torch.equal(ra[k], rb[k]), k


# ------------------------------------------------------------------------------------------ 1. one step against its parts
@pytest.mark.parametrize('name, B, dtype', PARTS, ids=IDS)
def test_a_forced_accept_step_has_the_bits_of_its_parts(name, B, dtype):
    """Explicit noise with forced acceptance and T-move uniforms 0 (theta = 0: nobody moves), no comb, from state_valid = 0.  Then x,
    logabs, phase, drift and eloc are those of ds_dmc_step on the same noise (eloc is the chain part alone); epp is
    ds_ecp_energy(x_after, the step's rotations) bit for bit and out_pairs its pair total; E = ((eloc + E_loc) + Re E_nl); the
    weight is the one-point formula (exp and one product: 4 ulp); the stats row and the four ecp_stats columns have the bits of
    the trees of dmc_parts_helpers."""
    sysd, dp = system(name, dtype)
    ecp = deh.potential(name)
    seed, o, tau = 7, 20, 0.1
    x0 = start(B, 2, dtype, name)
    rot = cu(eh.replay_rotations(seed, o + 1, B))[None]
    noise = explicit(sysd, B, 1, seed, o, rot, dtype, accept=True, tmove=np.zeros((1, B)))
    plain, st = sysd.dmc_state(x0), sysd.dmc_state(x0, ecp=True)
    st['epp'].fill_(-3.0)                                                           # (the initialisation sets it to 0; the step overwrites it)
    sysd.dmc_step(dp, plain, 1, tau, branch_every=0, state_valid=False, **{k: noise[k] for k in ('normals', 'uniforms', 'comb_uniforms')},
                  **KW)
    out = sysd.dmc_step(dp, st, 1, tau, branch_every=0, state_valid=False, ecp=ecp, tmoves=True, want_pairs=True, want_tmoves=True,
                        **noise, **KW)
    row = out['stats'].cpu().numpy()[0]
    assert row[3] == B and row[6] == 0 and bool((st['x'] != x0).any(1).all()) and bool((out['tmoves'] == -1).all())
    assert same_bits(plain, st, KEYS[:5]) == []
    e = sysd.ecp_energy(dp, st['x'], ecp, rotations=rot[0], want_pairs=True)
    assert torch.equal(bits(st['epp']), bits(epp_of(e))) and out['pairs'].tolist() == [int(e['pairs'].sum())] and int(out['pairs'][0]) > 0
    energy = (st['eloc'] + e['e_loc']) + e['e_nl'].real
    assert torch.equal(bits(out['energy'][0]), bits(energy))
    assert name == NAME or bool((st['epp'][:, 2] != 0).any())
    want = th.one_point_weights(np.ones(B), energy.cpu().numpy(), tau, KW['e_trial'], KW['e_ref'], KW['e_cut'])
    w = st['weight'].cpu().numpy()
    assert (np.abs(w - want) <= 4 * eh.EPS * want).all() and (want > 0).all()
    cols, n_clipped = ph.stats_from_state(w, energy.cpu().numpy(), KW['e_ref'], KW['e_cut'])
    assert np.array_equal(row[[0, 1, 2, 7]].view(np.int64), cols.view(np.int64)), (row, cols)
    assert row[5] == n_clipped and row[8] == B
    got, want4 = out['ecp_stats'].cpu().numpy()[0], th.tree_row4(w, st['epp'].cpu().numpy(), out['tmoves'][0].cpu().numpy())
    assert np.array_equal(got.view(np.int64), want4.view(np.int64)), (got, want4)


# ------------------------------------------------------------------------------------------ 2. the choice is steered
@pytest.mark.parametrize('name, B, dtype', PARTS, ids=IDS)
def test_the_choice_is_steered(name, B, dtype):
    """Every proposal is refused (NaN normals), so the pseudopotential is evaluated at the start walkers -- the rejected walker is
    evaluated where it stands.  The heat-bath intervals are built in numpy from the device's own ratios (ds_ecp_energy on the same
    walkers with the same rotations) and the weights of ecp_helpers.weights; walker w's uniform is the midpoint of the interval of
    no move (w % 4 = 0), of its first (1), last (2) or middle (3) configuration with Re term < 0.
    An interval is skipped when its half width is below 10 x the a-priori bound on the model-device difference of r_c (the walker
    then stays): n tau tol max |W / N_q| max(1, |q|) for the walker's n terms, tol = tol_q() -- the terms differ only by the
    rounding of W between numpy and the kernel and, in float32, by the rounding of the returned ratio to float32 (2^-23 is added
    to tol there); tol_q() is far above both.  At most a quarter of the walkers may be skipped
    (test_dmc_tmove_cpu.test_the_steered_inputs_stay_within_the_skip_cap checks the inputs on the oracle).
    out_tmove equals the targets; the moved electron is the wrapped quadrature point of the model to the rounding of k_ecp_propose
    and the wrap (16 ulp of the longest cell vector); every other electron and every unmoved walker is bit-identical; a moved
    walker's logabs, phase, drift and eloc are the chain's at its new position, an unmoved walker keeps its rows; weights stay."""
    sysd, dp = system(name, dtype)
    ecp = deh.potential(name)
    nq, tau = ecp.n_quad, th.STEER_TAU
    npdt = np.float64 if dtype == torch.float64 else np.float32
    x0 = start(B, th.STEER_WALKERS, dtype, name)
    xh = x0.cpu().numpy().astype(np.float64)
    rot_h = eh.replay_rotations(*th.STEER_ROT, B)
    rot = cu(rot_h)
    e = sysd.ecp_energy(dp, x0, ecp, rotations=rot, want_ratios=True, want_pairs=True)
    pl = eh.pair_list(ecp, xh)
    assert np.array_equal(pl['counts'], e['pairs'].cpu().numpy())
    q = e['ratios'].cpu().numpy().astype(np.complex128).reshape(-1, nq)
    Wn = eh.weights(ecp, pl, rot_h, nq)
    terms, scales = (Wn * q).reshape(-1), (np.abs(Wn) * np.maximum(1.0, np.abs(q))).reshape(-1)
    tol = deh.tol_q() + (0.0 if dtype == torch.float64 else ph.EPS32)
    target, u, skipped = th.steer_all(terms, scales, pl['counts'], nq, tau, tol)
    print('targets', target.tolist(), 'skipped', int(skipped.sum()))
    assert int(skipped.sum()) <= B // 4 and int((target >= 0).sum()) >= min(3, B - 2)
    noise = explicit(sysd, B, 1, 3, 0, rot[None], dtype, accept=False, tmove=u[None])
    st = sysd.dmc_state(x0, ecp=True)
    out = sysd.dmc_step(dp, st, 1, tau, tau_eff=0.0, branch_every=0, state_valid=False, ecp=ecp, tmoves=True, want_tmoves=True, **noise,
                        **KW)
    init = sysd.dmc_state(x0)
    sysd.dmc_step(dp, init, 1, tau, tau_eff=0.0, branch_every=0, state_valid=False,
                  **{k: noise[k] for k in ('normals', 'uniforms', 'comb_uniforms')}, **KW)
    assert float(out['stats'][0, 3]) == 0 and float(out['stats'][0, 6]) == B
    assert torch.equal(bits(st['epp']), bits(epp_of(e)))
    got = out['tmoves'][0].cpu().numpy()
    assert np.array_equal(got, target), (got, target)
    assert float(out['ecp_stats'][0, 3]) == int((target >= 0).sum())
    moved = cu(target >= 0, torch.bool)
    assert same_bits({k: v[~moved] for k, v in init.items()}, {k: st[k][~moved] for k in KEYS}, KEYS) == []
    assert torch.equal(st['weight'], torch.ones(B, **F64))
    x1 = st['x'].cpu().numpy().astype(np.float64)
    off = np.concatenate([[0], np.cumsum(pl['counts'])])
    U = eh.rotated_points(rot_h, nq)
    L = ph.longest_cell_vector(ecp.cell if hasattr(ecp, 'cell') else sh.case(name)[1])
    cell_ = sh.case(name)[1]
    for w in np.nonzero(target >= 0)[0]:
        p, k = off[w] + target[w] // nq, target[w] % nq
        el = int(pl['i'][p])
        same = np.ones(sysd.n, bool)
        same[el] = False
        assert np.array_equal(x1[w].reshape(-1, 3)[same], xh[w].reshape(-1, 3)[same]), w
        want = th.quadrature_point(cell_, xh[w, 3 * el:3 * el + 3], pl['r'][p], pl['dhat'][p], U[w, k], npdt)
        d = ph.min_image_distance(cell_, x1[w:w + 1, 3 * el:3 * el + 3], want[None])[0]
        assert d <= 16 * (eh.EPS if dtype == torch.float64 else ph.EPS32) * L, (w, d)
        assert not np.array_equal(x1[w, 3 * el:3 * el + 3], xh[w, 3 * el:3 * el + 3])
    # the second chain pass: the moved walkers' rows are the chain's at their new positions
    ke, ew, la, phs = sysd.local_energy(dp, st['x'], want_logpsi=True)
    assert torch.equal(bits(st['eloc'][moved]), bits((ke[:, 0].double() + ew.double())[moved]))
    assert torch.equal(bits(st['logabs'][moved]), bits(la[moved])) and torch.equal(bits(st['phase'][moved]), bits(phs[moved]))
    assert bool((st['drift'][moved] != init['drift'][moved]).any(1).all())


# ------------------------------------------------------------------------------------------ 3. replay against the model
@pytest.mark.parametrize('name', list(th.REPLAYS))
def test_replay_against_the_model(name):
    """The replays of dmc_tmove_helpers.REPLAYS (two steps, comb every step, Philox mode from state_valid = 0) against
    dmc_tmove_helpers.run_model on the CPU oracle: acceptances, T-move choices, parents, pair totals and the integer columns are
    equal; E of every walker within the tolerance of dmc_ecp_helpers; rows and weights within what that implies; the final state
    within the tolerances of test_gpu_dmc_ecp.py.  The lih replay has a walker with a NaN coordinate: it dies at the initialisation."""
    ref = th.replay_reference(name)
    th.assert_conditions(ref['cond'], died=name == NAME)
    B, tau, steps, seed = th.REPLAYS[name]
    sysd, dp = system(name)
    st = sysd.dmc_state(cu(ref['x0']), cu(ref['w0']), ecp=True)
    out = sysd.dmc_step(dp, st, steps, tau, branch_every=1, offset=0, state_valid=False, want_parents=True, want_pairs=True,
                        want_tmoves=True, tmoves=True, e_trial=ref['e_ref'], e_ref=ref['e_ref'], e_cut=ref['e_cut'], seed=seed,
                        ecp=ref['ecp'])
    rows, erows = out['stats'].cpu().numpy(), out['ecp_stats'].cpu().numpy()
    tol_e_all = 0.0
    for i, m in enumerate(ref['steps']):
        assert np.array_equal(out['tmoves'][i].cpu().numpy(), m['choice']), (i, out['tmoves'][i], m['choice'], m['tmargin'])
        assert np.array_equal(out['parents'][i].cpu().numpy(), m['parents']) and int(out['pairs'][i]) == m['pairs']
        for j in (3, 5, 6, 8):
            assert rows[i][j] == m['row'][j], (i, j, rows[i], m['row'])
        assert erows[i][3] == m['ecp_row'][3]
        live = m['w_commit'] != 0
        err = np.abs(out['energy'][i].cpu().numpy() - m['energy'])[live]
        assert (err <= m['tol_e'][live]).all(), (i, err, m['tol_e'][live])
        tol_e = float(np.nanmax(m['tol_e'][live]))
        tol_e_all = max(tol_e_all, tol_e)
        wsum, e_max = abs(m['row'][0]), float(np.nanmax(np.abs(m['energy'][live])))
        rel_w = tau * (i + 1) * tol_e_all + 1e-13
        assert abs(rows[i][0] - m['row'][0]) <= rel_w * wsum and abs(rows[i][7] - m['row'][7]) <= 2 * rel_w * m['row'][7]
        assert abs(rows[i][1] - m['row'][1]) <= wsum * (tol_e_all + rel_w * e_max)
        assert abs(rows[i][2] - m['row'][2]) <= wsum * (2 * e_max * tol_e_all + rel_w * e_max ** 2)
        assert abs(rows[i][4] - m['row'][4]) <= 1e-6 * B
        epp_max = float(np.nanmax(np.abs(m['epp'][live])))
        assert (np.abs(erows[i][:3] - m['ecp_row'][:3]) <= m['ecp_tol'] + rel_w * wsum * epp_max).all(), (i, erows[i], m['ecp_row'])
    s = ref['state']
    cell_ = sh.case(name)[1]
    assert ph.min_image_distance(cell_, st['x'].cpu().numpy(), s['x']).max() <= TOL_X
    assert np.abs(st['drift'].cpu().numpy() - s['drift']).max() <= 1e-8 * max(1.0, np.abs(s['drift']).max())
    assert np.abs(st['logabs'].cpu().numpy() - s['logabs']).max() <= 1e-9 * max(1.0, np.abs(s['logabs']).max())
    assert np.abs(phase_np(st) - s['phase']).max() <= 1e-8
    assert (np.abs(st['eloc'].cpu().numpy() - s['eloc']) <= 1e-8 * np.maximum(1.0, np.abs(s['ke'])) + 1e-9).all()
    assert np.abs(st['epp'].cpu().numpy() - s['epp']).max() <= tol_e_all
    w = st['weight'].cpu().numpy()
    assert (np.abs(w - s['weight']) <= (tau * steps * tol_e_all + 1e-13) * np.abs(s['weight']).max()).all(), (w, s['weight'])


# ------------------------------------------------------------------------------------------ 4. bit identities
def test_bit_identities():
    """lih, B = 37, 3 steps at tau = 0.3 (T-moves happen) with the comb every step.  Run to run; one call against step by step
    with the offset advanced and state_valid = 1; a workspace whose pseudopotential share holds two 80-configuration groups
    against the full one (the sizes read off the refusal, as test_gpu_dmc_ecp.py reads them); the fused comb against `dmc_branch`;
    Philox mode against explicit mode fed with ds_dmc_noise, the rotations the device draws for the counters offset + 1 + i, and the
    host replay of the stream-2 uniforms at index B + 1 + w."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    t = tables(sysd, ecp)
    x0 = start(B37, 3)
    steps, tau, seed, o = 3, 0.3, 3, 9
    cap = B37 * sysd.n * 2
    kw = dict(seed=seed, branch_every=1, ecp=ecp, tmoves=True, pair_capacity=cap, want_parents=True, want_pairs=True, want_tmoves=True, **KW)

    def run(**extra):
        st = sysd.dmc_state(x0, ecp=True)
        return st, sysd.dmc_step(dp, st, steps, tau, offset=o, state_valid=False, **kw, **extra)
    a, ra = run()
    assert int((ra['tmoves'] >= 0).sum()) >= 1 and 0 < float(ra['stats'][:, 3].sum()) < steps * B37
    assert torch.equal(ra['ecp_stats'][:, 3], (ra['tmoves'] >= 0).sum(1).double())
    with pytest.raises(RuntimeError, match='workspace too small') as err:
        sysd.ecp_energy(dp, x0, ecp, pair_capacity=cap, max_bytes=1)
    one = int(re.search(r'< (\d+) for one group', str(err.value)).group(1))
    full_e = int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, t.handle, B37, cap))
    per = (full_e - one) / ((cap * 12 + 79) // 80 - 1)
    with pytest.raises(RuntimeError, match='workspace too small for ds_dmc_step_tmove') as err:
        run(max_bytes=1)
    one11 = int(re.search(r'< (\d+) for one chain chunk', str(err.value)).group(1))
    full = int(sysd.lib.ds_dmc_tmove_workspace_bytes(sysd.handle, t.handle, B37, cap))
    assert per > 4096 and int(ra['pairs'].min()) * 12 > 160 and full > one11 + 3 * per
    assert full > int(sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, t.handle, B37, cap))
    two = one11 + int(per) + 2048                                               # room for two groups, not for three
    for st, out in (run(), run(max_bytes=two)):
        assert_same_call(a, ra, st, out)
    # step by step
    st = sysd.dmc_state(x0, ecp=True)
    outs = [sysd.dmc_step(dp, st, 1, tau, offset=o + i, state_valid=i > 0, **kw) for i in range(steps)]
    assert same_bits(a, st, KEYS7) == []
    for k in ('stats', 'ecp_stats', 'energy', 'parents', 'pairs', 'tmoves'):
        assert torch.equal(bits(torch.cat([r[k] for r in outs]).double()), bits(ra[k].double())), k
    # explicit mode
    rot = device_rotations(sysd, dp, x0, ecp, seed, [o + 1 + i for i in range(steps)])
    st = sysd.dmc_state(x0, ecp=True)
    out = sysd.dmc_step(dp, st, steps, tau, state_valid=False, **kw, **explicit(sysd, B37, steps, seed, o, rot))
    assert_same_call(a, ra, st, out)
    # the comb alone: one step without it, then dmc_branch with the step's xi, against the fused step
    w0 = cu(dh.preset_weights('ramp', B37))
    fused, split = sysd.dmc_state(x0, w0, ecp=True), sysd.dmc_state(x0, w0, ecp=True)
    rf = sysd.dmc_step(dp, fused, 1, tau, offset=o, state_valid=False, **kw)
    sysd.dmc_step(dp, split, 1, tau, offset=o, state_valid=False, **dict(kw, branch_every=0))
    before = split['epp'].clone()
    par = sysd.dmc_branch(split, float(sysd.dmc_noise(B37, 1, seed, o)[2][0]))
    assert torch.equal(par, rf['parents'][0]) and len(torch.unique(par)) < B37
    assert same_bits(fused, split, KEYS7) == [] and torch.equal(bits(split['epp']), bits(before[par.long()]))


# ------------------------------------------------------------------------------------------ 5. no non-local channel
@pytest.mark.parametrize('kind', ['local_only', 'zero'])
def test_without_negative_terms_nobody_moves(kind):
    """A potential without non-local channels has no pairs; the zero potential has pairs whose terms are all 0.  Either way out_tmove
    is all -1 and the fourth column of ecp_stats is 0; x, logabs, phase and drift have the bits of ds_dmc_step with the same seed
    (the weights differ: one-point against symmetric)."""
    sysd, dp = system(NAME)
    ecp = th.local_only_potential() if kind == 'local_only' else deh.zero_potential()
    x0 = start(B37, 3)
    kw = dict(seed=5, offset=9, branch_every=0, state_valid=False, **KW)
    plain, st = sysd.dmc_state(x0), sysd.dmc_state(x0, ecp=True)
    sysd.dmc_step(dp, plain, 2, 0.1, **kw)
    out = sysd.dmc_step(dp, st, 2, 0.1, ecp=ecp, tmoves=True, want_pairs=True, want_tmoves=True, **kw)
    assert bool((out['tmoves'] == -1).all()) and bool((out['ecp_stats'][:, 3] == 0).all())
    assert bool((out['pairs'] == 0).all()) if kind == 'local_only' else bool((out['pairs'] > 0).all())
    assert same_bits(plain, st, KEYS[:5]) == []
    assert bool((st['epp'][:, 1:] == 0).all()) and (bool((st['epp'][:, 0] != 0).any()) if kind == 'local_only' else bool((st['epp'] == 0).all()))


# ------------------------------------------------------------------------------------------ 6. two stats groups
def test_two_stats_groups():
    """lih, B = 300 (two rows of partials, the second of 44 walkers), one step at tau = 0.3 in Philox mode without a comb: the
    stats row and the four ecp_stats columns have the bits of the trees of dmc_parts_helpers on the weights, E and epp of the
    step, and the count column is the number of entries of out_tmove that are not -1 (some are)."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B, tau = 300, 0.3
    st = sysd.dmc_state(start(B, 3), cu(dh.preset_weights('ramp', B)), ecp=True)
    out = sysd.dmc_step(dp, st, 1, tau, seed=3, offset=9, branch_every=0, state_valid=False, ecp=ecp, tmoves=True, want_tmoves=True, **KW)
    w, energy, row = st['weight'].cpu().numpy(), out['energy'][0].cpu().numpy(), out['stats'].cpu().numpy()[0]
    choice = out['tmoves'][0].cpu().numpy()
    assert 0 < int((choice >= 0).sum()) < B and bool((st['weight'] > 0).all())
    cols, n_clipped = ph.stats_from_state(w, energy, KW['e_ref'], KW['e_cut'])
    assert np.array_equal(row[[0, 1, 2, 7]].view(np.int64), cols.view(np.int64)), (row, cols)
    assert row[5] == n_clipped and 0 < row[3] < B
    got, want = out['ecp_stats'].cpu().numpy()[0], th.tree_row4(w, st['epp'].cpu().numpy(), choice)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


# ------------------------------------------------------------------------------------------ 6b. one decision in three entries
@pytest.mark.parametrize('B, dtype', [(B37, torch.float64), (B37, torch.float32), (300, torch.float64)], ids=['37-float64', '37-float32', '300-float64'])
def test_the_three_entries_take_the_same_decision(B, dtype):
    """lih, one state initialised by the plain call (its first step included), then the same single step at tau = 0.1 without a
    comb or a clip through ds_dmc_step, ds_dmc_step_ecp and ds_dmc_step_tmove on the same explicit normals and uniforms.  The
    decision reads logabs, phase, drift and the noise alone, so the accepted count, sum p and the non-finite count (columns 3, 4
    and 6 of the stats row) have the same bits in the three calls, and x after the plain and the locality step is the same (the
    T-move step may move an electron afterwards).  A third of the uniforms forces acceptance (2^-60), a third are the Philox
    draws, a third are 1 (accepted only where A > 0): both outcomes occur.  B = 300: two stats groups, the second of 44."""
    sysd, dp = system(NAME, dtype)
    ecp = deh.potential()
    seed, o, tau = 11, 30, 0.1
    kw = dict(branch_every=0, e_cut=0.0)
    init = sysd.dmc_state(start(B, 4, dtype), ecp=True)
    sysd.dmc_step(dp, init, 1, tau, seed=seed, offset=o, state_valid=False, **kw)
    nz, un, xi = sysd.dmc_noise(B, 1, seed, o + 1)
    un[0, 0::3] = 2.0 ** -60
    un[0, 2::3] = 1.0
    noise = dict(normals=nz, uniforms=un, comb_uniforms=xi)
    rot = cu(eh.replay_rotations(seed, o + 2, B))[None]
    plain, loc, tm = clone(init), clone(init), clone(init)
    rows = [sysd.dmc_step(dp, plain, 1, tau, **noise, **kw)['stats'],
            sysd.dmc_step(dp, loc, 1, tau, ecp=ecp, rotations=torch.cat([rot, rot]), **noise, **kw)['stats'],
            sysd.dmc_step(dp, tm, 1, tau, ecp=ecp, tmoves=True, rotations=rot, tmove_uniforms=cu(th.tmove_uniforms(seed, o + 1, 1, B)),
                          **noise, **kw)['stats']]
    for r in rows[1:]:
        assert torch.equal(bits(r[0, [3, 4, 6]]), bits(rows[0][0, [3, 4, 6]])), (r, rows[0])
    assert torch.equal(bits(plain['x']), bits(loc['x']))
    assert 0 < float(rows[0][0, 3]) < B


# ------------------------------------------------------------------------------------------ 7. robustness
def test_a_walker_with_a_nan_coordinate_dies_and_disturbs_nobody():
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B = 12
    x0 = start(B, 6)
    bad = x0.clone()
    bad[5, 4] = float('nan')
    kw = dict(seed=6, state_valid=False, branch_every=0, ecp=ecp, tmoves=True, want_tmoves=True, **KW)
    clean, dirty = sysd.dmc_state(x0, ecp=True), sysd.dmc_state(bad, ecp=True)
    sysd.dmc_step(dp, clean, 2, 0.3, **kw)
    out = sysd.dmc_step(dp, dirty, 2, 0.3, **kw)
    rows = out['stats'].cpu().numpy()
    keep = torch.arange(B, device='cuda') != 5
    assert same_bits({k: v[keep] for k, v in clean.items()}, {k: v[keep] for k, v in dirty.items()}, KEYS7) == []
    assert float(dirty['weight'][5]) == 0.0 and bool(torch.isnan(dirty['epp'][5]).all()) and bool((out['tmoves'][:, 5] == -1).all())
    assert (rows[:, 6] == 1).all() and np.isfinite(rows).all() and bool(torch.isfinite(out['ecp_stats']).all())
    st = sysd.dmc_state(bad, ecp=True)
    par = sysd.dmc_step(dp, st, 2, 0.3, want_parents=True, **dict(kw, branch_every=2))['parents'].cpu().numpy()
    assert 5 not in par[1] and all(bool(torch.isfinite(st[k]).all()) for k in KEYS7)


def test_capacity_overflow_at_step_one_keeps_the_state_of_step_zero(monkeypatch):
    """B = 3 on the lih fixture walkers 2, 3, 4 (11 pairs), two steps of explicit noise with forced acceptance and no T-move.  Step
    0 has zero normals; step 1's normals carry the walkers to the midpoint walkers of test_gpu_dmc_ecp.py (24 pairs), so its
    evaluation at x_cur overflows a capacity of 12: the raw entry stops with steps_done = 1, the state exactly that of a call
    that took step 0 alone, and row 1 of the stats untouched.  The wrapper continues from the completed step with the capacity the
    message names and gives the bits of the call that was given 24."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B, tau, seed, o = 3, 0.01, 5, 40
    x0 = np.asarray(sh.case(NAME)[0]['x'], dtype=np.float64)[2:5]
    assert eh.pair_list(ecp, x0)['counts'].sum() == 11
    rot = cu(np.stack([eh.replay_rotations(seed, o + 1 + j, B) for j in range(2)]))
    un, xi, tu = torch.full((2, B), 2.0 ** -60, **F64), cu([0.3, 0.6]), torch.zeros(2, B, **F64)
    nz = torch.zeros(2, B, 3 * sysd.n, **F64)
    first = sysd.dmc_state(cu(x0), ecp=True)
    common = dict(branch_every=1, state_valid=False, ecp=ecp, tmoves=True, seed=seed, offset=o, **KW)
    sysd.dmc_step(dp, first, 1, tau, pair_capacity=24, normals=nz[:1], uniforms=un[:1], comb_uniforms=xi[:1], rotations=rot[:1],
                  tmove_uniforms=tu[:1], **common)
    x1, d1 = first['x'].cpu().numpy(), first['drift'].cpu().numpy()
    nz[1] = cu((midpoint_walkers() - x1 - tau * dh.limited(d1, tau)) / np.sqrt(tau))
    noise = dict(normals=nz, uniforms=un, comb_uniforms=xi, rotations=rot, tmove_uniforms=tu)
    c = sysd.dmc_state(cu(x0), ecp=True)
    stats = torch.full((2, 9), -7.0, **F64)
    rc, done, msg = raw_step(sysd, ecp, dp, c, steps=2, tau=tau, seed=seed, offset=o, cap=12, state_valid=0, stats=stats, branch_every=1,
                             noise=tuple(noise[k] for k in ('normals', 'uniforms', 'comb_uniforms', 'rotations', 'tmove_uniforms')))
    torch.cuda.synchronize()
    assert rc != 0 and done == 1 and 'pair capacity exceeded' in msg and 'the walkers have 24 pairs' in msg
    assert same_bits(first, c, KEYS7) == [] and bool((stats[1] == -7.0).all()) and bool((stats[0] != -7.0).all())
    monkeypatch.setattr(sysd, 'ECP_PAIR_BUDGET', 0)
    a, b = sysd.dmc_state(cu(x0), ecp=True), sysd.dmc_state(cu(x0), ecp=True)
    kw = dict(want_parents=True, want_pairs=True, want_tmoves=True, **noise, **common)
    ra = sysd.dmc_step(dp, a, 2, tau, **kw)
    rb = sysd.dmc_step(dp, b, 2, tau, pair_capacity=24, **kw)
    assert ra['pair_capacity'] == 24 and ra['pairs'].tolist() == [11, 24] and rb['pairs'].tolist() == [11, 24]
    assert_same_call(a, ra, b, rb)
    assert torch.equal(bits(stats[0]), bits(rb['stats'][0]))


def test_refusals_come_with_a_message_and_before_any_launch():
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B = 4
    st = sysd.dmc_state(start(B, 1), ecp=True)
    for k in KEYS7[1:5] + ('epp',):
        st[k].fill_(-3.0)                                                        # poison: a launch would show
    before = clone(st)
    ok = dict(steps=1, tau=0.1, tau_eff=0.1, e_trial=0.0, e_ref=0.0, e_cut=1.0, node_mode=0, branch_every=1, ecp=ecp, tmoves=True)
    nan = float('nan')
    cases = [(dict(steps=0), 'steps must be >= 1'), (dict(tau=0.0), 'tau must be > 0'), (dict(tau_eff=-0.1), 'tau_eff must be >= 0'),
             (dict(e_ref=nan), 'must be finite'), (dict(node_mode=2), 'node_mode must be 0'), (dict(branch_every=-1), 'branch_every must be >= 0'),
             (dict(pair_capacity=0), 'pair_capacity must be >= 1'), (dict(offset=2 ** 61 - 1), 'below 2^61'), (dict(offset=2 ** 63), 'below 2^61'),
             (dict(max_bytes=1), 'workspace too small for ds_dmc_step_tmove'),
             (dict(ecp=eh.fixture('bcc_li')['ecp']), 'simulation cell')]
    for kw, text in cases:
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=re.escape(text)) as err:
            sysd.dmc_step(dp, st, a.pop('steps'), a.pop('tau'), **a)
        assert 'ds_dmc_step_tmove' in str(err.value) or 'ds_ecp_energy' in str(err.value)
    nz, un, xi, rot, tu = (torch.zeros(s, **F64) for s in ((1, B, 3 * sysd.n), (1, B), (1,), (1, B, 3, 3), (1, B)))
    for part in (dict(tmove_uniforms=tu), dict(normals=nz, uniforms=un, comb_uniforms=xi, rotations=rot), dict(rotations=rot, tmove_uniforms=tu)):
        with pytest.raises(RuntimeError, match='ds_dmc_step_tmove: normals, uniforms, comb_uniforms, rotations and tmove_uniforms must be given together'):
            sysd.dmc_step(dp, st, 1, 0.1, ecp=ecp, tmoves=True, **part)
    stats = torch.full((1, 9), -7.0, **F64)
    for k in KEYS7[:6]:
        rc, done, msg = raw_step(sysd, ecp, dp, st, skip=k, stats=stats)
        assert rc == 1 and done == 0 and 'ds_dmc_step_tmove: null state pointer' in msg
    rc, _, msg = raw_step(sysd, ecp, dp, st, skip='epp', stats=stats)
    assert rc == 1 and 'epp is null' in msg
    rc, _, msg = raw_step(sysd, ecp, dp, st, ecp_handle=None, stats=stats)
    assert rc == 1 and 'null' in msg
    t = tables(sysd, ecp)
    assert sysd.lib.ds_dmc_tmove_workspace_bytes(sysd.handle, t.handle, 2 ** 20 + 1, 8) == -1
    assert sysd.lib.ds_dmc_tmove_workspace_bytes(sysd.handle, t.handle, B, 0) == -1
    assert sysd.lib.ds_dmc_tmove_workspace_bytes(sysd.handle, t.handle, B, 8) > sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, t.handle, B, 8)
    torch.cuda.synchronize()
    assert same_bits(before, st, KEYS7) == [] and bool((stats == -7.0).all())        # nothing was launched
    with pytest.raises(ValueError, match='needs a pseudopotential'):
        sysd.dmc_step(dp, sysd.dmc_state(start(B, 1)), 1, 0.1, tmoves=True)
    with pytest.raises(ValueError, match='go with tmoves=True'):
        sysd.dmc_step(dp, st, 1, 0.1, ecp=ecp, want_tmoves=True)


# ------------------------------------------------------------------------------------------ 8. run_dmc end to end
def test_run_dmc_with_tmoves(tmp_path):
    """lih, 16 walkers, 2 blocks of 2 steps at tau = 0.3: it runs, the CSV has finite `pseudopotential` and `tmoves` columns, and a
    save / load in the middle gives the bits of the uninterrupted run.  Without the option the schema is that of before."""
    from deepsolid_amd import dmc, inference, network
    _, cell, klist, net_kw, params = sh.case(NAME)
    dp = dev_params(params)
    slog, ld = (network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name=m, **net_kw) for m in ('eval_slogdet', 'eval_logdet'))
    ecp = deh.potential()
    x0 = start(16, 9)
    kw = dict(key=3, move_width=0.2, mcmc_steps=4, burn_in=3, vmc_iterations=2, tau=0.3, steps_per_block=2, pseudopotential=ecp, tmoves=True)
    state, rows, info = inference.run_dmc(slog, ld, dp, x0, cell, blocks=2, save_path=str(tmp_path), **kw)
    assert np.isfinite(info['vmc_energy']) and len(rows) == 2 and 'epp' in state.arrays
    for r in rows:
        assert np.isfinite(r['energy']) and np.isfinite(complex(r['pseudopotential']).real) and 0.0 <= r['tmoves'] <= 1.0
    text = (tmp_path / 'dmc_stats.csv').read_text().splitlines()
    assert text[0] == 'block,energy,variance,acceptance,tau_eff,e_trial,weight,killed,pseudopotential,tmoves' and len(text) == 3
    first, rows_a, _ = inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, save_path=str(tmp_path / 'a'), **kw)
    loaded = dmc.DmcState.load(tmp_path / 'a' / 'dmc_state.npz')
    second, rows_b, _ = inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, state=loaded, **kw)
    assert same_bits(state.arrays, second.arrays, KEYS7) == []
    assert (second.e_trial, second.e_ref, second.offset) == (state.e_trial, state.e_ref, state.offset)
    key = lambda r: (r['energy'], r['pseudopotential'], r['tmoves'])
    assert [key(r) for r in rows_a + rows_b] == [key(r) for r in rows]
    with pytest.raises(ValueError, match='needs a pseudopotential'):
        dmc.make_dmc_step(ld, cell, 0.01, 1, tmoves=True)
