"""GPU tests of DMC with a semi-local pseudopotential in the locality approximation: `ds_dmc_step_ecp` (csrc/ds_dmc.h, the algorithm
as include/deepsolid_hip.h states it) against its parts -- `ds_dmc_step`, `ds_ecp_energy`, `ds_local_energy`, `ds_dmc_branch` --
bit for bit, against the numpy model of dmc_ecp_helpers.py on the CPU oracle, its refusals, the pair capacity, and
`inference.run_dmc(..., pseudopotential=...)` end to end.  With the synthetic potential of ecp_helpers, on the lih case and, where a
test names them, on lih_twist and bcc_li, whose wavefunctions are complex: Im E_nl, the third column of epp, is live only there."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import dmc_ecp_helpers as deh
import dmc_helpers as dh
import dmc_parts_helpers as ph
import ecp_helpers as eh
import sampler_helpers as sh
from test_gpu_dmc import KEYS, TOL_X, assert_row_close, bits, clone, cu, dev_params, phase_np, same_bits, system

pytestmark = pytest.mark.gpu

KEYS7 = deh.KEYS7
NAME = deh.NAME
B37 = 37                      # neither a multiple of the wave nor of the four-wave workgroup
KW = dict(e_trial=-8.0, e_ref=-8.0, e_cut=3.0)
F64 = dict(dtype=torch.float64, device='cuda')


def tables(sysd, ecp):
    return sysd._ecp_tables(ecp)


def start(B, seed, dtype=torch.float64, name=NAME):
    return cu(dh.start_walkers(name, B, seed), dtype)


def ecp_row_bits(row, st):
    """A row of out_ecp_stats against dmc_parts_helpers.ecp_stats_from_state of the state it was formed from: bit for bit."""
    want = ph.ecp_stats_from_state(st['weight'].cpu().numpy(), st['epp'].cpu().numpy())
    got = row.cpu().numpy()
    return np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)


# (case, B) of the parts tests: B = 37 is neither a multiple of the wave nor of the four-wave workgroup; bcc_li has 24 electrons and
# about 15 pairs per walker
PARTS = [('lih', B37), ('lih_twist', B37), ('bcc_li', 5)]


def epp_of(e):
    """(B, 3) float64 as ds_dmc_step_ecp keeps it, from the output of `ecp_energy`."""
    return torch.stack([e['e_loc'], e['e_nl'].real, e['e_nl'].imag], dim=1).contiguous()


def plus_ecp(base, e):
    """((base + E_loc) + Re E_nl), each addition rounded in float64."""
    return (base + e['e_loc']) + e['e_nl'].real


def raw_step(sysd, ecp, dp, st, steps=1, tau=0.1, seed=0, offset=0, cap=None, state_valid=1, stats=None, ecp_stats=None, skip=None,
             ecp_handle='tables', branch_every=0, ws_bytes=None, noise=(None, None, None, None)):
    """The raw entry on a seven-array state, Philox mode or with `noise` = (normals, uniforms, comb_uniforms, rotations) float64
    -> (return code, steps_done, message)."""
    from deepsolid_amd.device import _ptr, _stream
    B = st['x'].shape[0]
    t = tables(sysd, ecp)
    cap = B * sysd.n * 2 if cap is None else cap
    ws = sysd._workspace('ds_dmc_ecp_workspace_bytes', t.handle, B, max(cap, 1))
    done = C.c_int(-1)
    ptrs = [None if k == skip else _ptr(st[k]) for k in KEYS7]
    rc = sysd.lib.ds_dmc_step_ecp(sysd.handle, t.handle if ecp_handle == 'tables' else ecp_handle, _ptr(sysd.pack_params(dp)), *ptrs, B,
                                  steps, tau, tau, KW['e_trial'], KW['e_ref'], KW['e_cut'], 0, branch_every, seed, offset,
                                  *[_ptr(t) for t in noise], cap, state_valid, _ptr(stats if stats is not None else torch.zeros(steps, 9, **F64)),
                                  _ptr(ecp_stats), None, None, C.byref(done), _ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                  _stream())
    return rc, done.value, sysd.lib.ds_last_error().decode()


# ------------------------------------------------------------------------------------------ 1. the initialisation and its parts
@pytest.mark.parametrize('name, B37, dtype', [pytest.param(n, b, torch.float64, id=f'{n}-{b}-float64') for n, b in PARTS] +
                         [pytest.param(n, b, torch.float32, id=f'{n}-{b}-float32') for n, b in (PARTS[0], PARTS[2])])
def test_initialisation_has_the_bits_of_its_parts(name, B37, dtype):
    """state_valid = 0: eloc = ((the plain initialisation) + E_loc) + Re E_nl of ds_ecp_energy(x, seed, offset), epp = its out_energy,
    out_pairs[0] = its pair total.  A call always takes a step, so the initial state is read off a step whose proposals are all
    refused as non-finite (NaN normals) at tau_eff = 0, as test_gpu_dmc.py reads it; the rotations of that explicit call are the
    ones the Philox-mode ds_ecp_energy drew.  A Philox-mode call then shows the same initial rows on the walkers it rejects.
    Off lih the third column of epp is live; everywhere the out_ecp_stats row has the bits of the tree of dmc_parts_helpers."""
    sysd, dp = system(name, dtype)
    ecp = deh.potential(name)
    seed, off = 11, 5
    x0 = start(B37, 4, dtype, name)
    e = sysd.ecp_energy(dp, x0, ecp, seed=seed, offset=off, want_pairs=True, want_rotations=True)
    rot = torch.stack([e['rotations'], e['rotations']])
    nan = torch.full((1, B37, 3 * sysd.n), float('nan'), dtype=dtype, device='cuda')
    noise = dict(normals=nan, uniforms=torch.full((1, B37), 0.5, dtype=dtype, device='cuda'), comb_uniforms=torch.zeros(1, **F64))
    plain, st = sysd.dmc_state(x0), sysd.dmc_state(x0, ecp=True)
    sysd.dmc_step(dp, plain, 1, 0.05, tau_eff=0.0, branch_every=0, state_valid=False, **noise)
    out = sysd.dmc_step(dp, st, 1, 0.05, tau_eff=0.0, branch_every=0, state_valid=False, ecp=ecp, rotations=rot, want_pairs=True, **noise)
    row = out['stats'].cpu().numpy()[0]
    assert row[3] == 0 and row[6] == B37
    assert same_bits(plain, st, KEYS[:4]) == [] and torch.equal(st['weight'], torch.ones(B37, **F64))
    assert torch.equal(bits(st['eloc']), bits(plus_ecp(plain['eloc'], e)))
    assert torch.equal(bits(st['epp']), bits(epp_of(e)))
    assert int(out['pairs'][0]) == int(e['pairs'].sum()) > 0 and int(out['pairs'][1]) == 0
    assert bool((e['e_nl'].abs() > 0).any()) and bool((e['e_loc'] != 0).any())
    assert name == NAME or bool((st['epp'][:, 2] != 0).any())
    same, rows = ecp_row_bits(out['ecp_stats'][0], st)
    assert same, rows
    # Philox mode: the rejected walkers still show the initialisation
    st2 = sysd.dmc_state(x0, ecp=True)
    out2 = sysd.dmc_step(dp, st2, 1, 0.3, branch_every=0, state_valid=False, ecp=ecp, seed=seed, offset=off, want_pairs=True, **KW)
    rej = (st2['x'] == x0).all(1)
    assert 0 < int(rej.sum()) < B37 and int(out2['pairs'][0]) == int(e['pairs'].sum())
    assert same_bits({k: st[k][rej] for k in KEYS7[:5] + ('epp',)}, {k: st2[k][rej] for k in KEYS7[:5] + ('epp',)}, KEYS7[:5] + ('epp',)) == []


# ------------------------------------------------------------------------------------------ 2. one forced-accept step
@pytest.mark.parametrize('name, B37', PARTS)
def test_a_forced_accept_step_equals_the_composition(name, B37):
    """Explicit noise from ds_dmc_noise with the uniforms replaced by 2^-60 (every finite proposal is accepted), rotations replayed
    for the counters o and o + 1, no comb: afterwards epp is ds_ecp_energy(x_after, rotations[1]) bit for bit -- the same call on
    the same array -- and eloc is Re ke + ewald of ds_local_energy(x_after) plus the two terms in the stated order."""
    sysd, dp = system(name)
    ecp = deh.potential(name)
    seed, o = 7, 20
    x0 = start(B37, 2, name=name)
    nz, un, xi = sysd.dmc_noise(B37, 1, seed, o)
    un = torch.full_like(un, 2.0 ** -60)
    rot = cu(np.stack([eh.replay_rotations(seed, o, B37), eh.replay_rotations(seed, o + 1, B37)]))
    st = sysd.dmc_state(x0, ecp=True)
    out = sysd.dmc_step(dp, st, 1, 0.1, branch_every=0, state_valid=False, ecp=ecp, normals=nz, uniforms=un, comb_uniforms=xi,
                        rotations=rot, want_pairs=True, **KW)
    row = out['stats'].cpu().numpy()[0]
    assert row[3] == B37 and row[6] == 0 and bool((st['x'] != x0).any(1).all())
    e = sysd.ecp_energy(dp, st['x'], ecp, rotations=rot[1], want_pairs=True)
    assert torch.equal(bits(st['epp']), bits(epp_of(e))) and int(out['pairs'][1]) == int(e['pairs'].sum()) > 0
    ke, ew, la, ph = sysd.local_energy(dp, st['x'], want_logpsi=True)
    assert torch.equal(bits(st['eloc']), bits(plus_ecp(ke[:, 0].double() + ew.double(), e)))
    assert torch.equal(bits(st['logabs']), bits(la)) and torch.equal(bits(st['phase']), bits(ph))
    # the ecp_stats row: sum w epp over the walkers, to the rounding of a sum of B terms
    want = (st['weight'][:, None] * st['epp']).sum(0).cpu().numpy()
    mag = (st['weight'][:, None] * st['epp']).abs().sum(0).cpu().numpy()
    assert (np.abs(out['ecp_stats'].cpu().numpy()[0] - want) <= B37 * eh.EPS * mag).all()
    # ... and to the bit in the order the kernels add them; off lih the third column is live
    same, rows = ecp_row_bits(out['ecp_stats'][0], st)
    assert same, rows
    assert name == NAME or bool((st['epp'][:, 2] != 0).any())


# ------------------------------------------------------------------------------------------ 3. replay against the model
@pytest.mark.parametrize('name', list(deh.REPLAYS))
def test_replay_against_the_model(name):
    """The replays of dmc_ecp_helpers.REPLAYS (lih: B = 12, 2 steps, tau = 0.1), comb every step, Philox mode from state_valid = 0
    against dmc_ecp_helpers.run_model on the CPU oracle: decisions, parents and the integer columns are equal; positions, log|psi|,
    phase and drift within the tolerances of test_gpu_dmc.py; eloc within eloc_bound(ke) + TOL_Q e_nl_scale + the E_loc bound;
    weights, rows and ecp_stats within what those imply.  lih_twist and bcc_li have a complex wavefunction: the third column of epp
    and of ecp_stats is compared against a model value that is not zero."""
    ref = deh.replay_reference(name)
    deh.assert_conditions(ref['cond'])
    assert name == NAME or ref['cond']['im_e_nl'] > 0
    B, tau, steps, seed = deh.REPLAYS[name]
    sysd, dp = system(name)
    kw = dict(e_trial=ref['e_ref'], e_ref=ref['e_ref'], e_cut=ref['e_cut'], seed=seed, ecp=ref['ecp'])
    st = sysd.dmc_state(cu(ref['x0']), cu(ref['w0']), ecp=True)
    out = sysd.dmc_step(dp, st, steps, tau, branch_every=1, offset=0, state_valid=False, want_parents=True, want_pairs=True, **kw)
    rows, parents, erows = out['stats'].cpu().numpy(), out['parents'].cpu().numpy(), out['ecp_stats'].cpu().numpy()
    pairs = out['pairs'].cpu().numpy()
    assert pairs[0] == ref['pairs0']
    # the decisions, read off a step-by-step run (its bits are those of the one call: test_bit_identities)
    st2 = sysd.dmc_state(cu(ref['x0']), cu(ref['w0']), ecp=True)
    tol_e_all = 0.0
    for i, m in enumerate(ref['steps']):
        before = clone(st2)
        sysd.dmc_step(dp, st2, 1, tau, branch_every=0, offset=i, state_valid=i > 0, **kw)
        mask = (st2['x'] != before['x']).any(1).cpu().numpy()
        assert np.array_equal(mask, m['acc']), (i, mask, m['acc'], m['margin'])
        par = sysd.dmc_branch(st2, m['xi']).cpu().numpy()
        assert np.array_equal(par, m['parents']) and np.array_equal(parents[i], m['parents']), (i, par, parents[i], m['parents'])
        assert pairs[i + 1] == m['pairs']
        for j in (3, 5, 6, 8):
            assert rows[i][j] == m['row'][j], (i, j, rows[i], m['row'])
        tol_e = float(np.nanmax(m['tol_prop']))
        tol_e_all = max(tol_e_all, tol_e)
        wsum = abs(m['row'][0])
        # sum w, sum w^2: the weights move by tau_eff (steps so far) tol_e relatively; sum w E, sum w E^2: that and tol_e on E
        rel_w = tau * (i + 1) * tol_e_all + 1e-13
        e_max = float(np.nanmax(np.abs(m['e_prop'])))
        assert abs(rows[i][0] - m['row'][0]) <= rel_w * wsum and abs(rows[i][7] - m['row'][7]) <= 2 * rel_w * m['row'][7]
        assert abs(rows[i][1] - m['row'][1]) <= wsum * (tol_e_all + rel_w * e_max)
        assert abs(rows[i][2] - m['row'][2]) <= wsum * (2 * e_max * tol_e_all + rel_w * e_max ** 2)
        assert abs(rows[i][4] - m['row'][4]) <= 1e-6 * B
        epp_max = float(np.nanmax(np.abs(m['epp_prop'])))
        assert (np.abs(erows[i] - m['ecp_row']) <= m['ecp_tol'] + rel_w * wsum * epp_max).all(), (i, erows[i], m['ecp_row'])
    assert same_bits(st, st2, KEYS7) == []
    s = ref['state']
    x, dr = st['x'].cpu().numpy(), st['drift'].cpu().numpy()
    assert np.abs(x - s['x']).max() <= TOL_X
    assert np.abs(dr - s['drift']).max() <= 1e-8 * max(1.0, np.abs(s['drift']).max())
    assert np.abs(st['logabs'].cpu().numpy() - s['logabs']).max() <= 1e-9 * max(1.0, np.abs(s['logabs']).max())
    assert np.abs(phase_np(st) - s['phase']).max() <= 1e-8
    err = np.abs(st['eloc'].cpu().numpy() - s['eloc'])
    print('eloc error', err.tolist(), 'tolerance', s['tol_eloc'].tolist())
    assert (err <= s['tol_eloc']).all()
    assert (np.abs(st['epp'].cpu().numpy() - s['epp']).max(1) <= s['tol_eloc']).all()
    w = st['weight'].cpu().numpy()
    assert (np.abs(w - s['weight']) <= (tau * steps * tol_e_all + 1e-13) * np.abs(s['weight']).max()).all(), (w, s['weight'])


# ------------------------------------------------------------------------------------------ 4. a potential that is zero
def test_zero_potential_changes_nothing():
    """Every coefficient 0 with the cutoffs given explicitly (pairs exist, the ratios are evaluated): three steps with a comb have the
    bits of ds_dmc_step with the same seed and offset in every array, the rows and the parents; epp is all zeros."""
    sysd, dp = system(NAME)
    zero = deh.zero_potential()
    x0 = start(B37, 3)
    kw = dict(seed=5, offset=9, branch_every=1, state_valid=False, want_parents=True, **KW)
    plain, st = sysd.dmc_state(x0), sysd.dmc_state(x0, ecp=True)
    ra = sysd.dmc_step(dp, plain, 3, 0.1, **kw)
    rb = sysd.dmc_step(dp, st, 3, 0.1, ecp=zero, want_pairs=True, **kw)
    assert same_bits(plain, st) == []
    assert torch.equal(bits(ra['stats']), bits(rb['stats'])) and torch.equal(ra['parents'], rb['parents'])
    assert bool((st['epp'] == 0).all()) and bool((rb['ecp_stats'] == 0).all()) and bool((rb['pairs'] > 0).all())
    assert 0 < float(ra['stats'][:, 3].sum()) < 3 * B37


# ------------------------------------------------------------------------------------------ 5. bit identities
def test_bit_identities():
    """Run to run; 3 steps in one call against 3 calls of one step with the offset advanced and state_valid = 1; a workspace whose
    pseudopotential share holds two 80-configuration groups, and one half way, against the full one (every evaluation has more than 160
    configurations, so chunks end inside walkers' segments; the condition of test_two_group_workspace_gives_identical_bits: the
    value chain picks the same kernels for 160 configurations as for all of them); the fused comb's epp against `dmc_branch` on a
    seven-array state."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    t = tables(sysd, ecp)
    x0 = start(B37, 3)
    steps, tau, seed, o = 3, 0.1, 3, 9
    cap = B37 * sysd.n * 2
    kw = dict(seed=seed, branch_every=1, ecp=ecp, pair_capacity=cap, want_parents=True, want_pairs=True, **KW)

    def run(**extra):
        st = sysd.dmc_state(x0, ecp=True)
        return st, sysd.dmc_step(dp, st, steps, tau, offset=o, state_valid=False, **kw, **extra)
    a, ra = run()
    # the per-group bytes from ds_ecp_energy's own sizes, as test_gpu_ecp.py takes them, and the bytes of one chain walker plus one
    # group from the refusal: a workspace of that plus one more group runs the chain walker by walker and the pseudopotential in
    # chunks of two groups (the split rule of the header: room for groups beside one walker first, then the chain, then the rest)
    with pytest.raises(RuntimeError, match='workspace too small') as err:
        sysd.ecp_energy(dp, x0, ecp, pair_capacity=cap, max_bytes=1)
    one = int(re.search(r'< (\d+) for one group', str(err.value)).group(1))
    full_e = int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, t.handle, B37, cap))
    groups = (cap * 12 + 79) // 80
    per = (full_e - one) / (groups - 1)
    with pytest.raises(RuntimeError, match='workspace too small for ds_dmc_step_ecp') as err:
        run(max_bytes=1)
    one11 = int(re.search(r'< (\d+) for one chain chunk', str(err.value)).group(1))
    full = int(sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, t.handle, B37, cap))
    assert per > 4096 and int(ra['pairs'].min()) * 12 > 160 and full > one11 + 3 * per
    two = one11 + int(per) + 2048                                               # room for two groups, not for three
    for st, out in (run(), run(max_bytes=two), run(max_bytes=(two + full) // 2)):
        assert same_bits(a, st, KEYS7) == []
        for k in ('stats', 'ecp_stats'):
            assert torch.equal(bits(ra[k]), bits(out[k])), k
        assert torch.equal(ra['parents'], out['parents']) and torch.equal(ra['pairs'], out['pairs'])
    with pytest.raises(RuntimeError, match='workspace too small for ds_dmc_step_ecp'):
        run(max_bytes=one11 - 1)
    # step by step
    st = sysd.dmc_state(x0, ecp=True)
    outs = [sysd.dmc_step(dp, st, 1, tau, offset=o + i, state_valid=i > 0, **kw) for i in range(steps)]
    assert same_bits(a, st, KEYS7) == []
    for k in ('stats', 'ecp_stats', 'parents'):
        assert torch.equal(bits(torch.cat([r[k] for r in outs])), bits(ra[k])), k
    assert torch.equal(torch.cat([outs[0]['pairs']] + [r['pairs'][1:] for r in outs[1:]]), ra['pairs'])
    assert 0 < float(ra['stats'][:, 3].sum()) < steps * B37
    # the comb alone: one step without it, then dmc_branch with the step's xi, against the fused step
    w0 = cu(dh.preset_weights('ramp', B37))                                      # (unequal weights: the comb duplicates walkers)
    fused, split = sysd.dmc_state(x0, w0, ecp=True), sysd.dmc_state(x0, w0, ecp=True)
    rf = sysd.dmc_step(dp, fused, 1, tau, offset=o, state_valid=False, **kw)
    sysd.dmc_step(dp, split, 1, tau, offset=o, state_valid=False, **dict(kw, branch_every=0))
    before = split['epp'].clone()
    xi = float(sysd.dmc_noise(B37, 1, seed, o)[2][0])
    par = sysd.dmc_branch(split, xi)
    assert torch.equal(par, rf['parents'][0]) and len(torch.unique(par)) < B37
    assert same_bits(fused, split, KEYS7) == [] and torch.equal(bits(split['epp']), bits(before[par.long()]))


# ------------------------------------------------------------------------------------------ 6. rejected walkers
def test_rejected_walkers_keep_everything():
    """Philox mode, tau = 0.3: both outcomes occur; a rejected walker's rows in all seven arrays are bit-identical to before the
    step, except its weight, which is the formula with E_new = E_old (to the rounding of exp and one product: 4 ulp)."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    x0 = start(B37, 6)
    tau = 0.3
    st = sysd.dmc_state(x0, ecp=True)
    kw = dict(seed=8, branch_every=0, ecp=ecp, **KW)
    sysd.dmc_step(dp, st, 1, tau, offset=0, state_valid=False, **kw)
    before = clone(st)
    sysd.dmc_step(dp, st, 1, tau, offset=1, state_valid=True, **kw)
    rej = (st['x'] == before['x']).all(1)
    assert 0 < int(rej.sum()) < B37
    keys = tuple(k for k in KEYS7 if k != 'weight')
    assert same_bits({k: before[k][rej] for k in keys}, {k: st[k][rej] for k in keys}, keys) == []
    acc = ~rej
    assert bool((st['epp'][acc] != before['epp'][acc]).any(1).all())
    e, w0 = before['eloc'][rej].cpu().numpy(), before['weight'][rej].cpu().numpy()
    c = KW['e_ref'] + np.clip(e - KW['e_ref'], -KW['e_cut'], KW['e_cut'])
    want = w0 * np.exp(-tau * (0.5 * (c + c) - KW['e_trial']))
    assert (np.abs(st['weight'][rej].cpu().numpy() - want) <= 4 * eh.EPS * want).all()


# ------------------------------------------------------------------------------------------ 7. the pair capacity
def test_capacity_overflow_fails_before_the_acceptance_and_keeps_the_state():
    sysd, dp = system(NAME)
    ecp = deh.potential()
    x0 = start(B37, 2)
    seed, tau = 4, 0.1
    kw = dict(seed=seed, branch_every=0, ecp=ecp, want_pairs=True, **KW)
    st = sysd.dmc_state(x0, ecp=True)
    p0 = int(sysd.dmc_step(dp, st, 1, tau, offset=0, state_valid=False, **kw)['pairs'][0])         # (default capacity: never fails)
    s1, s2 = clone(st), clone(st)
    p1 = int(sysd.dmc_step(dp, s1, 1, tau, offset=1, state_valid=True, **kw)['pairs'][1])
    assert p0 > 1 and p1 > 1 and same_bits(st, s1, KEYS7) != []
    stats = torch.full((1, 9), -7.0, **F64)
    rc, done, msg = raw_step(sysd, ecp, dp, s2, tau=tau, seed=seed, offset=1, cap=p1 - 1, state_valid=1, stats=stats)
    torch.cuda.synchronize()
    assert rc != 0 and done == 0 and f'the walkers have {p1} pairs' in msg and 'pair capacity exceeded' in msg
    assert same_bits(st, s2, KEYS7) == [] and bool((stats == -7.0).all())
    # with exactly the number needed it runs, and gives the bits of the default capacity
    rc, done, msg = raw_step(sysd, ecp, dp, s2, tau=tau, seed=seed, offset=1, cap=p1, state_valid=1)
    assert rc == 0 and done == 1 and same_bits(s1, s2, KEYS7) == []
    # the initialisation: all seven arrays untouched
    fresh = sysd.dmc_state(x0, ecp=True)
    for k in KEYS7[1:5] + ('epp',):
        fresh[k].fill_(-3.0)
    before = clone(fresh)
    rc, done, msg = raw_step(sysd, ecp, dp, fresh, tau=tau, seed=seed, offset=0, cap=p0 - 1, state_valid=0)
    torch.cuda.synchronize()
    assert rc != 0 and done == 0 and f'the walkers have {p0} pairs' in msg
    assert same_bits(before, fresh, KEYS7) == []


# ------------------------------------------------------------------------------------------ 7b. two stats groups
def test_two_stats_groups_with_a_pseudopotential():
    """lih, B = 300 (two rows of stats partials, the second of 44 walkers; two blocks of k_dmc_gather_epp), 2 steps in Philox mode
    with the comb every step, against the same steps taken one by one without the fused comb and `dmc_branch` after each: every
    ecp_stats row has the bits of dmc_parts_helpers.ecp_stats_from_state of the state before that step's comb, epp after the comb
    is before[parents], and stats, parents and pairs agree between the two paths."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B, steps, tau, seed, o = 300, 2, 0.1, 3, 9
    x0, w0 = start(B, 3), cu(dh.preset_weights('ramp', B))
    kw = dict(seed=seed, ecp=ecp, want_parents=True, want_pairs=True, **KW)
    fused, split = sysd.dmc_state(x0, w0, ecp=True), sysd.dmc_state(x0, w0, ecp=True)
    rf = sysd.dmc_step(dp, fused, steps, tau, offset=o, state_valid=False, branch_every=1, **kw)
    pairs = []
    for i in range(steps):
        r = sysd.dmc_step(dp, split, 1, tau, offset=o + i, state_valid=i > 0, branch_every=0, **kw)
        before = clone(split)
        for row in (rf['ecp_stats'][i], r['ecp_stats'][0]):
            same, rows = ecp_row_bits(row, before)
            assert same, (i, rows)
        xi = float(sysd.dmc_noise(B, 1, seed, o + i)[2][0])
        par = sysd.dmc_branch(split, xi)
        assert torch.equal(par, rf['parents'][i]) and len(torch.unique(par)) < B
        assert torch.equal(bits(split['epp']), bits(before['epp'][par.long()]))
        assert torch.equal(bits(r['stats'][0, :8]), bits(rf['stats'][i, :8])) and float(r['stats'][0, 8]) == B
        assert float(rf['stats'][i, 8]) == len(torch.unique(par))
        pairs += r['pairs'].tolist() if i == 0 else r['pairs'].tolist()[1:]
    assert same_bits(fused, split, KEYS7) == [] and pairs == rf['pairs'].tolist()
    assert 0 < float(rf['stats'][:, 3].sum()) < steps * B and bool((rf['ecp_stats'][:, :2] != 0).all())


# ------------------------------------------------------------------------------------------ 7c. the wrapper's continuation
def midpoint_walkers():
    """The three walkers of test_gpu_ecp.test_wrapper_retries_once_with_the_needed_capacity: all four electrons near the midpoint of
    Li and H, 8 pairs each, 24 > B N = 12."""
    ecp = deh.potential()
    rng = np.random.default_rng(4)
    mid = np.asarray([0.5 * ecp.atoms[1][0], 0.0, 0.0])
    x = (mid[None, None, :] + rng.uniform(-0.15, 0.15, (3, 4, 3))).reshape(3, 12)
    assert eh.pair_list(ecp, x)['counts'].tolist() == [8, 8, 8]
    return x


def assert_same_call(a, ra, b, rb):
    assert same_bits(a, b, KEYS7) == []
    for k in ('stats', 'ecp_stats'):
        assert torch.equal(bits(ra[k]), bits(rb[k])), k
    assert torch.equal(ra['parents'], rb['parents']) and torch.equal(ra['pairs'], rb['pairs'])


@pytest.mark.parametrize('mode', ['philox', 'explicit'])
def test_default_capacity_overflow_at_the_initialisation_is_retried(monkeypatch, mode):
    """With the pair budget at 0 the default capacity is B N = 12; the midpoint walkers have 24 pairs, so the initialisation overflows:
    the wrapper repeats the whole call (nothing was done) with the capacity the message names, and arrays and outputs have the bits
    of a call that was given it -- in Philox mode with the same offset, in explicit mode with the same rotations."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    monkeypatch.setattr(sysd, 'ECP_PAIR_BUDGET', 0)
    x0 = cu(midpoint_walkers())
    B, steps, tau, seed, o = 3, 2, 0.01, 5, 40
    kw = dict(seed=seed, offset=o, branch_every=1, state_valid=False, ecp=ecp, want_parents=True, want_pairs=True, **KW)
    if mode == 'explicit':
        nz, un, xi = sysd.dmc_noise(B, steps, seed + 1, 3)
        kw.update(normals=nz, uniforms=un, comb_uniforms=xi, rotations=cu(np.stack([eh.replay_rotations(seed, 7 + j, B) for j in range(steps + 1)])))
    a, b = sysd.dmc_state(x0, ecp=True), sysd.dmc_state(x0, ecp=True)
    ra = sysd.dmc_step(dp, a, steps, tau, **kw)
    rb = sysd.dmc_step(dp, b, steps, tau, pair_capacity=24, **kw)
    assert ra['pair_capacity'] == 24 and rb['pair_capacity'] == 24 and int(ra['pairs'][0]) == 24
    assert_same_call(a, ra, b, rb)
    assert bool((a['x'] != x0).any()) and bool(torch.isfinite(ra['stats']).all())


def overflow_inside(sysd, dp, ecp, branch_every):
    """B = 3 on the lih fixture walkers 2, 3, 4 (11 pairs, every electron-ion distance at least 0.5 Bohr from the non-local cutoff; a
    drift move is shorter than sqrt(2 tau) = 0.14), tau = 0.01, two steps of explicit noise.  Step 0 has zero normals: the pair total
    stays 11 whether or not it accepts.  Step 1's normals are chi = (target - x_1 - tau vbar_1) / sqrt(tau) with (x_1, drift_1) read
    off a clone that took step 0 alone with capacity 24 and target the midpoint walkers: its proposal has 24 pairs.
    -> (start state, noise dict, the step-0 clone)."""
    B, tau, seed, o = 3, 0.01, 5, 40
    x0 = np.asarray(sh.case(NAME)[0]['x'], dtype=np.float64)[2:5]
    r = eh.min_image(x0, ecp.atoms, ecp.a)[0]
    assert eh.pair_list(ecp, x0)['counts'].sum() == 11 and np.abs(r - deh.R_CUT).min() >= 0.5
    rot = cu(np.stack([eh.replay_rotations(seed, o + j, B) for j in range(3)]))
    un, xi = torch.full((2, B), 0.5, **F64), cu([0.3, 0.6])
    nz = torch.zeros(2, B, 3 * sysd.n, **F64)
    first = sysd.dmc_state(cu(x0), ecp=True)
    sysd.dmc_step(dp, first, 1, tau, branch_every=1 if branch_every == 1 else 0, state_valid=False, ecp=ecp, pair_capacity=24,
                  normals=nz[:1], uniforms=un[:1], comb_uniforms=xi[:1], rotations=rot[:2], **KW)
    x1, d1 = first['x'].cpu().numpy(), first['drift'].cpu().numpy()
    nz[1] = cu((midpoint_walkers() - x1 - tau * dh.limited(d1, tau)) / np.sqrt(tau))
    return sysd.dmc_state(cu(x0), ecp=True), dict(normals=nz, uniforms=un, comb_uniforms=xi, rotations=rot), first


def test_default_capacity_overflow_inside_the_call_continues_from_the_completed_steps(monkeypatch):
    """The second step's proposal overflows the default capacity of 12: the wrapper continues from the one completed step -- offset,
    noise, rotations and outputs advanced by one, state_valid set -- and everything has the bits of the call given capacity 24.
    The raw entry with capacity 12 stops with steps_done = 1, the state that of the step-0 clone and row 1 of the stats untouched."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    monkeypatch.setattr(sysd, 'ECP_PAIR_BUDGET', 0)
    tau, seed, o = 0.01, 5, 40
    st, noise, first = overflow_inside(sysd, dp, ecp, 1)
    kw = dict(seed=seed, offset=o, branch_every=1, state_valid=False, ecp=ecp, want_parents=True, want_pairs=True, **noise, **KW)
    a, b, c = clone(st), clone(st), clone(st)
    ra = sysd.dmc_step(dp, a, 2, tau, **kw)
    rb = sysd.dmc_step(dp, b, 2, tau, pair_capacity=24, **kw)
    assert ra['pair_capacity'] == 24 and ra['pairs'].tolist() == [11, 11, 24] and rb['pairs'].tolist() == [11, 11, 24]
    assert_same_call(a, ra, b, rb)
    stats = torch.full((2, 9), -7.0, **F64)
    rc, done, msg = raw_step(sysd, ecp, dp, c, steps=2, tau=tau, seed=seed, offset=o, cap=12, state_valid=0, stats=stats, branch_every=1,
                             noise=tuple(noise[k] for k in ('normals', 'uniforms', 'comb_uniforms', 'rotations')))
    torch.cuda.synchronize()
    assert rc != 0 and done == 1 and 'pair capacity exceeded' in msg and 'the walkers have 24 pairs' in msg
    assert same_bits(first, c, KEYS7) == []
    assert bool((stats[1] == -7.0).all()) and torch.equal(bits(stats[0]), bits(rb['stats'][0]))


def test_no_continuation_off_the_combs_schedule(monkeypatch):
    """branch_every = 2: a continuation from one completed step would shift the comb's schedule, so the overflow is raised, and the
    state is that after the one completed step."""
    sysd, dp = system(NAME)
    ecp = deh.potential()
    monkeypatch.setattr(sysd, 'ECP_PAIR_BUDGET', 0)
    st, noise, first = overflow_inside(sysd, dp, ecp, 2)
    with pytest.raises(RuntimeError, match='pair capacity exceeded: the walkers have 24 pairs'):
        sysd.dmc_step(dp, st, 2, 0.01, seed=5, offset=40, branch_every=2, state_valid=False, ecp=ecp, **noise, **KW)
    torch.cuda.synchronize()
    assert same_bits(first, st, KEYS7) == [] and bool((st['eloc'] != 0).all())


# ------------------------------------------------------------------------------------------ 8. non-finite input
def test_a_walker_with_a_nan_coordinate_dies_and_disturbs_nobody():
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B = 12
    x0 = start(B, 6)
    bad = x0.clone()
    bad[5, 4] = float('nan')
    kw = dict(seed=6, state_valid=False, branch_every=0, ecp=ecp, **KW)
    clean, dirty = sysd.dmc_state(x0, ecp=True), sysd.dmc_state(bad, ecp=True)
    sysd.dmc_step(dp, clean, 2, 0.1, **kw)
    out = sysd.dmc_step(dp, dirty, 2, 0.1, **kw)
    rows = out['stats'].cpu().numpy()
    keep = torch.arange(B, device='cuda') != 5
    assert same_bits({k: v[keep] for k, v in clean.items()}, {k: v[keep] for k, v in dirty.items()}, KEYS7) == []
    assert float(dirty['weight'][5]) == 0.0 and bool(torch.isnan(dirty['epp'][5]).all())
    assert (rows[:, 6] == 1).all() and np.isfinite(rows).all() and bool(torch.isfinite(out['ecp_stats']).all())
    # ... and is gone after the comb
    st = sysd.dmc_state(bad, ecp=True)
    par = sysd.dmc_step(dp, st, 2, 0.1, want_parents=True, **dict(kw, branch_every=2))['parents'].cpu().numpy()
    assert 5 not in par[1] and all(bool(torch.isfinite(st[k]).all()) for k in KEYS7)


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_come_with_a_message_and_before_any_launch():
    sysd, dp = system(NAME)
    ecp = deh.potential()
    B = 4
    st = sysd.dmc_state(start(B, 1), ecp=True)
    for k in KEYS7[1:5] + ('epp',):
        st[k].fill_(-3.0)                                                        # poison: a launch would show
    before = clone(st)
    ok = dict(steps=1, tau=0.1, tau_eff=0.1, e_trial=0.0, e_ref=0.0, e_cut=1.0, node_mode=0, branch_every=1, ecp=ecp)
    nan = float('nan')
    cases = [(dict(steps=0), 'steps must be >= 1'), (dict(tau=0.0), 'tau must be > 0'), (dict(tau_eff=-0.1), 'tau_eff must be >= 0'),
             (dict(e_ref=nan), 'must be finite'), (dict(node_mode=2), 'node_mode must be 0'), (dict(branch_every=-1), 'branch_every must be >= 0'),
             (dict(pair_capacity=0), 'pair_capacity must be >= 1'), (dict(offset=2 ** 61 - 1), 'below 2^61'), (dict(offset=2 ** 63), 'below 2^61'),
             (dict(max_bytes=1), 'workspace too small for ds_dmc_step_ecp'),
             (dict(ecp=eh.fixture('bcc_li')['ecp']), 'simulation cell')]
    for kw, text in cases:
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=re.escape(text)):
            sysd.dmc_step(dp, st, a.pop('steps'), a.pop('tau'), **a)
    nz, un, xi, rot = (torch.zeros(s, **F64) for s in ((1, B, 3 * sysd.n), (1, B), (1,), (2, B, 3, 3)))
    for part in (dict(rotations=rot), dict(normals=nz, uniforms=un, comb_uniforms=xi), dict(normals=nz, rotations=rot)):
        with pytest.raises(RuntimeError, match='must be given together'):
            sysd.dmc_step(dp, st, 1, 0.1, ecp=ecp, **part)
    stats = torch.full((1, 9), -7.0, **F64)
    for k in KEYS7[:6]:
        rc, done, msg = raw_step(sysd, ecp, dp, st, skip=k, stats=stats)
        assert rc == 1 and done == 0 and 'null state pointer' in msg
    rc, _, msg = raw_step(sysd, ecp, dp, st, skip='epp', stats=stats)
    assert rc == 1 and 'epp is null' in msg
    rc, _, msg = raw_step(sysd, ecp, dp, st, ecp_handle=None, stats=stats)
    assert rc == 1 and 'null' in msg
    t = tables(sysd, ecp)
    assert sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, t.handle, 2 ** 20 + 1, 8) == -1
    assert sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, t.handle, B, 0) == -1
    assert sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, t.handle, B, 8) > sysd.lib.ds_dmc_workspace_bytes(sysd.handle, B)
    torch.cuda.synchronize()
    assert same_bits(before, st, KEYS7) == [] and bool((stats == -7.0).all())        # nothing was launched
    with pytest.raises(ValueError, match="'epp'"):
        sysd.dmc_step(dp, sysd.dmc_state(start(B, 1)), 1, 0.1, ecp=ecp)
    with pytest.raises(ValueError, match='go with a pseudopotential'):
        sysd.dmc_step(dp, sysd.dmc_state(start(B, 1)), 1, 0.1, pair_capacity=5)


# ------------------------------------------------------------------------------------------ 10. run_dmc end to end
def test_run_dmc_with_a_pseudopotential(tmp_path):
    """lih, 16 walkers, 2 blocks of 2 steps: it runs, the CSV has a finite `pseudopotential` column (the DMC CSV does not split
    kinetic and Ewald, so there is no sum of columns to check), and a save / load in the middle gives the bits of the
    uninterrupted run."""
    from deepsolid_amd import dmc, inference, network
    _, cell, klist, net_kw, params = sh.case(NAME)
    dp = dev_params(params)
    slog, ld = (network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name=m, **net_kw) for m in ('eval_slogdet', 'eval_logdet'))
    ecp = deh.potential()
    x0 = start(16, 9)
    kw = dict(key=3, move_width=0.2, mcmc_steps=4, burn_in=3, vmc_iterations=2, tau=0.02, steps_per_block=2, pseudopotential=ecp)
    state, rows, info = inference.run_dmc(slog, ld, dp, x0, cell, blocks=2, save_path=str(tmp_path), **kw)
    assert np.isfinite(info['vmc_energy']) and len(rows) == 2 and 'epp' in state.arrays
    for r in rows:
        assert np.isfinite(r['energy']) and np.isfinite(complex(r['pseudopotential']).real) and np.isfinite(complex(r['pseudopotential']).imag)
        assert abs(complex(r['pseudopotential'])) > 0
    text = (tmp_path / 'dmc_stats.csv').read_text().splitlines()
    assert text[0] == 'block,energy,variance,acceptance,tau_eff,e_trial,weight,killed,pseudopotential' and len(text) == 3
    first, rows_a, _ = inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, save_path=str(tmp_path / 'a'), **kw)
    loaded = dmc.DmcState.load(tmp_path / 'a' / 'dmc_state.npz')
    assert 'epp' in loaded.arrays
    second, rows_b, _ = inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, state=loaded, **kw)
    assert same_bits(state.arrays, second.arrays, KEYS7) == []
    assert (second.e_trial, second.e_ref, second.offset) == (state.e_trial, state.e_ref, state.offset)
    assert [(r['energy'], r['pseudopotential']) for r in rows_a + rows_b] == [(r['energy'], r['pseudopotential']) for r in rows]
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, steps_per_block=1, tau=0.01, pseudopotential=object())
