"""GPU tests of the fixed-phase DMC: `ds_dmc_step` / `ds_dmc_branch` (csrc/ds_dmc.h) against the numpy model of
tests/dmc_helpers.py on the CPU oracle, their bit-identities, refusals, and `inference.run_dmc` end to end.  Every replay fixture
asserts its oracle-only conditions (dmc_helpers.assert_conditions) at run time: every decision is decidable and none is skipped."""
import re

import numpy as np
import pytest
import torch

import dmc_helpers as dh
import sampler_helpers as sh

pytestmark = pytest.mark.gpu

TOL_X = 1e-9                 # positions: what test_gpu_samplers.py holds the importance sampler to
KEYS = ('x', 'logabs', 'phase', 'drift', 'eloc', 'weight')


def cu(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device='cuda')


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(vv, dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v] for k, v in params.items()}


_SYSTEMS = {}


def system(name, dtype=torch.float64):
    """-> (DeviceSystem of the case, its device parameters)."""
    if (name, dtype) not in _SYSTEMS:
        from deepsolid_amd import network
        _, cell, klist, net_kw, params = sh.case(name)
        net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', dtype=dtype, **net_kw)
        _SYSTEMS[name, dtype] = (net.apply.system, dev_params(params, dtype))
    return _SYSTEMS[name, dtype]


def clone(st):
    return {k: v.clone() for k, v in st.items()}


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bits(a, b, keys=KEYS):
    return [k for k in keys if not torch.equal(bits(a[k]), bits(b[k]))]


def phase_np(st):
    p = st['phase'].cpu().numpy().astype(np.float64)
    return p[:, 0] + 1j * p[:, 1]


def eloc_bound(ke):
    """What test_local_energy_vs_oracle allows on E_L."""
    return 1e-8 * np.maximum(1.0, np.abs(ke)) + 1e-9


def assert_state_close(st, ref, tau_steps):
    x, dr = st['x'].cpu().numpy(), st['drift'].cpu().numpy()
    live = np.isfinite(ref['eloc'])
    assert np.abs(x - ref['x'])[live].max() <= TOL_X
    assert np.abs(dr - ref['drift'])[live].max() <= 1e-8 * max(1.0, np.abs(ref['drift'][live]).max())
    assert np.abs(st['logabs'].cpu().numpy() - ref['logabs'])[live].max() <= 1e-9 * max(1.0, np.abs(ref['logabs'][live]).max())
    assert np.abs(phase_np(st) - ref['phase'])[live].max() <= 1e-8
    bound = eloc_bound(ref['ke'][live])
    assert (np.abs(st['eloc'].cpu().numpy() - ref['eloc'])[live] <= bound).all()
    w = st['weight'].cpu().numpy()
    assert (np.abs(w - ref['weight']) <= (tau_steps * bound.max() + 1e-13) * np.abs(ref['weight']).max()).all(), (w, ref['weight'])


def assert_row_close(row, ref, B):
    for j in (3, 5, 6, 8):
        assert row[j] == ref[j], (j, row, ref)
    scale = max(1.0, abs(ref[0]))
    assert abs(row[0] - ref[0]) <= 1e-9 * scale and abs(row[7] - ref[7]) <= 1e-9 * max(1.0, ref[7])
    assert abs(row[1] - ref[1]) <= 1e-7 * max(1.0, abs(ref[1])) and abs(row[2] - ref[2]) <= 1e-7 * max(1.0, abs(ref[2]))
    assert abs(row[4] - ref[4]) <= 1e-6 * B


# ---------------------------------------------------------------------------------------------------- 1. replay against the model
@pytest.mark.parametrize('key', list(dh.REPLAYS))
def test_replay_against_the_model(key):
    """Philox mode, state_valid = 0, comb every step, once as ONE call and once step by step through the separate entries (one
    ds_dmc_step without comb, then ds_dmc_branch with the step's xi): accept masks (read off the rows that changed) and parents
    equal the model's, state and rows are within the tolerances, and both paths give the same bits."""
    ref = dh.replay_reference(key)
    dh.assert_conditions(ref['cond'])
    name, B, tau, steps, seed, _ = dh.REPLAYS[key]
    sysd, dp = system(name)
    kw = dict(e_trial=ref['e_ref'], e_ref=ref['e_ref'], e_cut=ref['e_cut'], seed=seed)
    st = sysd.dmc_state(cu(ref['x0']), cu(ref['w0']))
    out = sysd.dmc_step(dp, st, steps, tau, branch_every=1, offset=0, state_valid=False, want_parents=True, **kw)
    rows, parents = out['stats'].cpu().numpy(), out['parents'].cpu().numpy()
    st2 = sysd.dmc_state(cu(ref['x0']), cu(ref['w0']))
    for i, m in enumerate(ref['steps']):
        before = clone(st2)
        row = sysd.dmc_step(dp, st2, 1, tau, branch_every=0, offset=i, state_valid=i > 0, **kw)['stats'].cpu().numpy()[0]
        if i == 0:       # the initialisation: the step has already selected, so the rows it rejected show the initial E_L
            rej = ~m['acc']
            assert (np.abs(st2['eloc'].cpu().numpy() - ref['state0']['eloc'])[rej] <= eloc_bound(ref['state0']['ke'][rej])).all()
        mask = (st2['x'] != before['x']).any(1).cpu().numpy()
        assert np.array_equal(mask, m['acc']), (i, mask, m['acc'], m['margin'])
        assert row[8] == B and np.array_equal(row[:8], rows[i][:8]), (i, row, rows[i])
        par = sysd.dmc_branch(st2, m['xi']).cpu().numpy()
        assert np.array_equal(par, m['parents']) and np.array_equal(parents[i], m['parents']), (i, par, parents[i], m['parents'])
        assert_row_close(rows[i], m['row'], B)
    assert same_bits(st, st2) == []
    assert_state_close(st, ref['state'], tau * steps)


# ----------------------------------------------------------------------------------------------------------- 2. explicit noise
def philox_and_explicit(name, B, steps, tau, seed, offset=5, **kw):
    sysd, dp = system(name)
    x0 = cu(dh.start_walkers(name, B, seed))
    a, b = sysd.dmc_state(x0), sysd.dmc_state(x0)
    ra = sysd.dmc_step(dp, a, steps, tau, seed=seed, offset=offset, state_valid=False, want_parents=True, **kw)
    # the draws themselves, from the device (`ds_dmc_noise`): the host model of the normals agrees to a few ulp, not to the bit
    nz, un, xi = sysd.dmc_noise(B, steps, seed, offset)
    m_nz, m_un = sh.noise(seed, offset, steps, B, sysd.n)
    m_xi = np.array([sh.uniform(seed, offset, i, np.uint64(B)) for i in range(steps)]).reshape(steps)
    assert np.abs(nz.cpu().numpy() - m_nz).max() <= 1e-13 and np.array_equal(un.cpu().numpy(), m_un) and np.array_equal(xi.cpu().numpy(), m_xi)
    rb = sysd.dmc_step(dp, b, steps, tau, normals=nz, uniforms=un, comb_uniforms=xi, state_valid=False, want_parents=True, **kw)
    return a, ra, b, rb


def test_explicit_noise_replays_the_philox_draws_bit_for_bit():
    a, ra, b, rb = philox_and_explicit('lih', 24, 3, 0.1, 2, e_trial=-8.0, e_ref=-8.0, e_cut=3.0, branch_every=1)
    assert same_bits(a, b) == []
    assert torch.equal(bits(ra['stats']), bits(rb['stats'])) and torch.equal(ra['parents'], rb['parents'])
    assert float(ra['stats'][:, 3].sum()) > 0                                   # something moved


# ------------------------------------------------------------------------------------------------------------- 3. bit-identity
def one_chunk_bytes(sysd, dp, st):
    """dmc_bytes(B, one walker per chain chunk), from the message of the refusal."""
    with pytest.raises(RuntimeError, match='workspace too small for ds_dmc_step') as e:
        sysd.dmc_step(dp, clone(st), 1, 0.1, max_bytes=1)
    return int(re.search(r'< (\d+) for one chain chunk', str(e.value)).group(1))


def test_bit_identity_run_to_run_chunks_and_split_calls():
    name, B, steps, tau, seed = 'lih', 24, 4, 0.1, 3
    sysd, dp = system(name)
    x0 = cu(dh.start_walkers(name, B, seed))
    kw = dict(e_trial=-8.0, e_ref=-8.0, e_cut=3.0, seed=seed, branch_every=1)
    runs = []
    full = int(sysd.lib.ds_dmc_workspace_bytes(sysd.handle, B))
    one = one_chunk_bytes(sysd, dp, sysd.dmc_state(x0))
    per = (full - one) // (B - 1)
    for max_bytes in (None, None, one + 6 * per + 64, one):                   # whole batch twice, chunks of 7 (the last of 3), chunks of 1
        st = sysd.dmc_state(x0)
        out = sysd.dmc_step(dp, st, steps, tau, offset=9, state_valid=False, want_parents=True, max_bytes=max_bytes, **kw)
        runs.append((st, out))
    for st, out in runs[1:]:
        assert same_bits(runs[0][0], st) == []
        assert torch.equal(bits(runs[0][1]['stats']), bits(out['stats'])) and torch.equal(runs[0][1]['parents'], out['parents'])
    # 4 steps in one call against 4 calls of one step with the offset advanced and state_valid = 1
    st = sysd.dmc_state(x0)
    rows = [sysd.dmc_step(dp, st, 1, tau, offset=9 + i, state_valid=i > 0, **kw)['stats'][0] for i in range(steps)]
    assert same_bits(runs[0][0], st) == []
    assert torch.equal(bits(torch.stack(rows)), bits(runs[0][1]['stats']))
    assert len({int(r[3]) for r in rows} | {0}) > 1


# ------------------------------------------------------------------------------------- 4. the same bits as the separate entries
@pytest.mark.parametrize('name', ['lih', 'lih_twist', 'bcc_li'])
def test_initialisation_has_the_bits_of_local_energy_and_logpsi_grad(name):
    """After state_valid = 0, logabs, phase and eloc have the bits of ds_local_energy on the same walkers (Re ke + ewald in float64)
    and drift those of the real part of ds_logpsi_grad: all three run the same chain.  A call always takes a step, which selects in
    place, so the initial state is read off a step whose proposals are all refused as non-finite (NaN normals) at tau_eff = 0."""
    sysd, dp = system(name)
    B = 6
    x0 = cu(dh.start_walkers(name, B, 4))
    st = sysd.dmc_state(x0)
    nan = torch.full((1, B, 3 * sysd.n), float('nan'), dtype=torch.float64, device='cuda')
    out = sysd.dmc_step(dp, st, 1, 0.05, tau_eff=0.0, normals=nan, uniforms=torch.full((1, B), 0.5, dtype=torch.float64, device='cuda'),
                        comb_uniforms=torch.zeros(1, dtype=torch.float64, device='cuda'), branch_every=0, state_valid=False)
    row = out['stats'].cpu().numpy()[0]
    assert row[3] == 0 and row[6] == B and row[4] == 0                      # nothing accepted, every proposal non-finite, p = 0
    ke, ew, la, ph = sysd.local_energy(dp, x0, want_logpsi=True)
    la_g, g = sysd.logpsi_grad(dp, x0)
    assert torch.equal(st['x'], x0) and torch.equal(bits(st['logabs']), bits(la)) and torch.equal(bits(st['phase']), bits(ph))
    assert torch.equal(bits(st['eloc']), bits(ke[:, 0].double() + ew.double()))
    assert torch.equal(bits(st['drift']), bits(g.real.contiguous())) and torch.equal(bits(la_g), bits(la))
    assert torch.equal(st['weight'], torch.ones(B, dtype=torch.float64, device='cuda'))      # tau_eff = 0: exp(0) = 1


# ---------------------------------------------------------------------------------------------------- 5. ds_dmc_branch alone
def weight_pattern(kind, B, seed=0):
    rng = np.random.default_rng(1000 * B + seed)
    if kind == 'equal':
        return np.full(B, 0.75)
    if kind == 'one_hot':
        w = np.zeros(B)
        w[B // 3] = 2.0
        return w
    if kind == 'zeros':
        w = rng.random(B) + 0.1
        w[rng.random(B) < 0.4] = 0.0
        w[B - 1] = 0.0 if B > 1 else 1.0
        if not w.any():
            w[0] = 1.0
        return w
    return rng.lognormal(0.0, 1.0, B)


def random_state(sysd, B, w, seed=5):
    g = torch.Generator(device='cuda').manual_seed(seed + B)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, device='cuda', generator=g)
    return dict(x=r(B, 3 * sysd.n), logabs=r(B), phase=r(B, 2), drift=r(B, 3 * sysd.n), eloc=r(B), weight=cu(w))


@pytest.mark.parametrize('B', [1, 63, 64, 65, 257, 4097])
def test_branch_alone(B):
    """Parents equal the model (whose prefix sums are the device's bit for bit), gathered rows are bitwise the parents' rows,
    weights are the bits of W / B."""
    sysd, _ = system('lih')
    for kind, xi in (('equal', 0.0), ('equal', 1.0 - 2.0 ** -53), ('one_hot', 0.5), ('zeros', 0.3), ('lognormal', 0.123), ('lognormal', 0.9)):
        w = weight_pattern(kind, B)
        c = dh.comb(w, xi)
        assert c['run'] and (c['margin'] > 0 or kind != 'lognormal'), (kind, c['margin'])       # lognormal: no tooth on an edge
        st = random_state(sysd, B, w)
        before = clone(st)
        par = sysd.dmc_branch(st, xi)
        assert np.array_equal(par.cpu().numpy(), c['parents']), (kind, xi, B)
        idx = par.long()
        assert same_bits({k: before[k][idx] for k in KEYS[:5]}, st, KEYS[:5]) == []
        assert torch.equal(bits(st['weight']), bits(torch.full((B,), float(c['step']), dtype=torch.float64, device='cuda')))
        if kind == 'equal':
            assert np.array_equal(c['parents'], np.arange(B))


@pytest.mark.parametrize('B', [5, 300])
def test_branch_leaves_the_state_when_the_total_is_zero_or_not_a_number(B):
    sysd, _ = system('lih')
    for w in (np.zeros(B), np.where(np.arange(B) == B // 2, np.nan, 1.0)):
        st = random_state(sysd, B, w)
        before = clone(st)
        par = sysd.dmc_branch(st, 0.4)
        assert same_bits(before, st) == [] and np.array_equal(par.cpu().numpy(), np.arange(B))


# ------------------------------------------------------------------------------------------------------------- 6. node_mode = 1
def test_fixed_node_refuses_a_sign_change_that_fixed_phase_accepts():
    ref = dh.node_reference()
    c = ref['cond']
    assert c['undecidable'] == 0 and c['crossing_accepted'] >= 1, c
    sysd, dp = system(ref['name'])
    got = {}
    for mode, tag in ((0, 'free'), (1, 'fixed')):
        st = sysd.dmc_state(cu(ref['x0']))
        before = st['x'].clone()
        out = sysd.dmc_step(dp, st, 1, ref['tau'], e_trial=ref['e_ref'], e_ref=ref['e_ref'], e_cut=0.0, node_mode=mode, branch_every=0,
                            seed=ref['seed'], state_valid=False)
        got[tag] = (st['x'] != before).any(1).cpu().numpy()
        m = ref[tag]['steps'][0]
        assert np.array_equal(got[tag], m['acc']), (tag, got[tag], m['acc'], m['margin'], m['overlap'])
        assert_row_close(out['stats'].cpu().numpy()[0], m['row'], ref['B'])
    w = c['walkers']
    assert got['free'][w].all() and not got['fixed'][w].any()


# ---------------------------------------------------------------------------------------------------------- 7. non-finite input
def test_a_walker_with_a_nan_coordinate_dies_and_disturbs_nobody():
    name, B, tau, seed = 'lih', 12, 0.1, 6
    sysd, dp = system(name)
    x0 = cu(dh.start_walkers(name, B, seed))
    bad = x0.clone()
    bad[5, 4] = float('nan')
    kw = dict(e_trial=-8.0, e_ref=-8.0, e_cut=3.0, seed=seed, state_valid=False)
    clean, dirty = sysd.dmc_state(x0), sysd.dmc_state(bad)
    sysd.dmc_step(dp, clean, 2, tau, branch_every=0, **kw)
    rows = sysd.dmc_step(dp, dirty, 2, tau, branch_every=0, **kw)['stats'].cpu().numpy()
    keep = torch.arange(B, device='cuda') != 5
    assert same_bits({k: v[keep] for k, v in clean.items()}, {k: v[keep] for k, v in dirty.items()}) == []
    assert float(dirty['weight'][5]) == 0.0 and (rows[:, 6] == 1).all() and np.isfinite(rows).all()
    assert abs(rows[-1, 0] - float(clean['weight'][keep].sum())) <= 1e-12 * rows[-1, 0]
    # ... and is gone after the comb
    st = sysd.dmc_state(bad)
    out = sysd.dmc_step(dp, st, 2, tau, branch_every=2, want_parents=True, **kw)
    par = out['parents'].cpu().numpy()
    assert 5 not in par[1] and np.array_equal(par[0], np.arange(B)) and out['stats'].cpu().numpy()[1, 8] == len(np.unique(par[1]))
    assert all(bool(torch.isfinite(st[k]).all()) for k in KEYS)


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_come_with_a_message_and_before_any_launch():
    sysd, dp = system('lih')
    B = 4
    x0 = cu(dh.start_walkers('lih', B, 1))
    st = sysd.dmc_state(x0)
    ok = dict(steps=1, tau=0.1, tau_eff=0.1, e_trial=0.0, e_ref=0.0, e_cut=1.0, node_mode=0, branch_every=1)
    nan = float('nan')
    cases = [(dict(steps=0), 'steps must be >= 1'), (dict(tau=0.0), 'tau must be > 0'), (dict(tau=-1.0), 'tau must be > 0'),
             (dict(tau_eff=-0.1), 'tau_eff must be >= 0'), (dict(tau=nan), 'must be finite'), (dict(e_trial=float('inf')), 'must be finite'),
             (dict(e_ref=nan), 'must be finite'), (dict(e_cut=nan), 'must be finite'), (dict(node_mode=2), 'node_mode must be 0'),
             (dict(node_mode=-1), 'node_mode must be 0'), (dict(branch_every=-1), 'branch_every must be >= 0')]
    before = clone(st)
    for kw, text in cases:
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=re.escape(text)):
            sysd.dmc_step(dp, st, a.pop('steps'), a.pop('tau'), **a)
    nz, un, xi = (torch.zeros(s, dtype=torch.float64, device='cuda') for s in ((1, B, 3 * sysd.n), (1, B), (1,)))
    for part in (dict(normals=nz), dict(normals=nz, uniforms=un), dict(comb_uniforms=xi), dict(uniforms=un, comb_uniforms=xi)):
        with pytest.raises(RuntimeError, match='must be given together'):
            sysd.dmc_step(dp, st, 1, 0.1, **part)
    with pytest.raises(RuntimeError, match='workspace too small for ds_dmc_step'):
        sysd.dmc_step(dp, st, 1, 0.1, max_bytes=one_chunk_bytes(sysd, dp, st) - 1)
    # null state pointers, B out of range: the raw entry
    from deepsolid_amd.device import _ptr, _stream
    p = sysd.pack_params(dp)
    ws = sysd.workspace(B)
    stats = torch.zeros(1, 9, dtype=torch.float64, device='cuda')

    def raw(B_=B, skip=None, stats_=stats):
        ptrs = [None if k == skip else _ptr(st[k]) for k in KEYS]
        return sysd.lib.ds_dmc_step(sysd.handle, _ptr(p), *ptrs, B_, 1, 0.1, 0.1, 0.0, 0.0, 0.0, 0, 0, 1, 0, None, None, None, 1,
                                    _ptr(stats_), None, _ptr(ws), ws.numel(), _stream())
    for k in KEYS:
        assert raw(skip=k) == 1 and b'null state pointer' in sysd.lib.ds_last_error()
    assert raw(stats_=None) == 1 and b'out_stats is null' in sysd.lib.ds_last_error()
    for B_ in (0, -3, 2 ** 20 + 1):
        assert raw(B_=B_) == 1 and b'B must be in 1..1048576' in sysd.lib.ds_last_error()
    assert sysd.lib.ds_dmc_workspace_bytes(sysd.handle, 2 ** 20 + 1) == -1 and sysd.lib.ds_dmc_workspace_bytes(sysd.handle, 2 ** 20) > 0
    torch.cuda.synchronize()
    assert same_bits(before, st) == [] and float(stats.abs().sum()) == 0.0            # nothing was launched
    with pytest.raises(ValueError, match='DMC state entry'):
        sysd.dmc_step(dp, dict(st, eloc=st['eloc'].float()), 1, 0.1)


# ------------------------------------------------------------------------------------------------------------------- 9. float32
def test_float32_step_within_the_oracles_own_float32_loss():
    """One step on lih, B = 8, float32: log|psi| and E_L of the start walkers and of the accepted proposals within 3 x what the
    oracle's own float32 run loses (common.float32_tolerance); every decision is decidable under that budget and equals the
    float64 model's."""
    ref = dh.f32_reference()
    assert ref['cond']['undecidable'] == 0 and ref['cond']['accepted'] >= 1, ref['cond']
    sysd, dp = system(ref['name'], torch.float32)
    B, m = ref['B'], ref['steps'][0]
    st = sysd.dmc_state(cu(ref['x0'], torch.float32))
    before = st['x'].clone()
    out = sysd.dmc_step(dp, st, 1, ref['tau'], e_trial=ref['e_ref'], e_ref=ref['e_ref'], e_cut=0.0, branch_every=0, seed=ref['seed'],
                        state_valid=False)
    mask = (st['x'] != before).any(1).cpu().numpy()
    assert np.array_equal(mask, m['acc']), (mask, m['acc'], m['margin'], ref['tol_a'])
    # Both oracles at the points where the device's walkers now sit (an accepted walker sits at the device's own float32 proposal,
    # which is the model's only to float32 rounding: E_L moves by more than the budget over that distance, so the comparison is
    # made at the same point, as the budget rule requires)
    from common import float32_tolerance
    xs = st['x'].double().cpu().numpy()
    assert np.abs(xs - ref['state']['x']).max() <= 1e-5 * max(1.0, float(np.abs(xs).max()))
    a64, a32 = dh.dmc_oracle(ref['name']).evaluate(xs), dh.dmc_oracle(ref['name'], True).evaluate(xs)
    la, el = st['logabs'].double().cpu().numpy(), st['eloc'].cpu().numpy()
    for q, idx, got in (('logabs', 0, la), ('eloc', 3, el)):
        scale = np.maximum(1.0, np.abs(a64[idx]))
        loss = (np.abs(a32[idx] - a64[idx]) / scale).tolist()
        tol = np.array([float32_tolerance(loss, w) for w in range(B)]) * scale
        err = np.abs(got - a64[idx])
        print(q, 'error', err.tolist(), 'budget', tol.tolist(), 'oracle float32 loss', loss)
        assert (err <= tol).all(), (q, err, tol)
    assert out['stats'].cpu().numpy()[0, 3] == mask.sum()


# ------------------------------------------------------------------------------------------- 10. the variational bound, end to end
def test_run_dmc_energy_is_not_above_the_vmc_energy(tmp_path):
    """h2, fixture parameters, B = 512, tau = 0.01, a few hundred steps after equilibration through `inference.run_dmc`: the
    fixed-phase energy is bounded by the trial energy as tau -> 0, so E_DMC <= E_VMC + 3 sigma, sigma = the two reblocked errors in
    quadrature.  The sign and nothing more.  A resumed run continues bit-identically."""
    from deepsolid_amd import dmc, inference, init_guess, network
    _, cell, klist, net_kw, params = sh.case('h2')
    dp = dev_params(params)
    slog, ld = (network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name=m, **net_kw) for m in ('eval_slogdet', 'eval_logdet'))
    x0 = torch.as_tensor(init_guess.init_electrons(5, cell, cell.a, cell.nelec, 512, init_width=0.8), device='cuda')
    kw = dict(key=7, move_width=0.3, mcmc_steps=10, burn_in=20, vmc_iterations=64)
    state, rows, info = inference.run_dmc(slog, ld, dp, x0, cell, blocks=32, steps_per_block=10, tau=0.01, save_path=str(tmp_path), **kw)
    warm = 8                                                           # blocks left out: the projection time to leave the VMC distribution
    e_dmc, err_dmc, _ = dmc.reblock([r['energy'] for r in rows[warm:]])
    sigma = float(np.hypot(err_dmc, info['vmc_error']))
    print(f"h2: E_VMC {info['vmc_energy']:.6f} +- {info['vmc_error']:.6f}, E_DMC {e_dmc:.6f} +- {err_dmc:.6f}, "
          f"acceptance {np.mean([r['acceptance'] for r in rows]):.4f}, tau_eff {rows[-1]['tau_eff']:.6f}")
    assert all(np.isfinite(r['energy']) and 0.9 < r['acceptance'] <= 1.0 and r['weight'] > 0 for r in rows)
    assert e_dmc <= info['vmc_energy'] + 3.0 * sigma, (e_dmc, err_dmc, info['vmc_energy'], info['vmc_error'])
    text = (tmp_path / 'dmc_stats.csv').read_text().splitlines()
    assert text[0] == 'block,energy,variance,acceptance,tau_eff,e_trial,weight,killed' and len(text) == 33
    # resume: 16 + 16 blocks give the bits of 32
    first, rows_a, _ = inference.run_dmc(slog, ld, dp, x0, cell, blocks=16, steps_per_block=10, tau=0.01, save_path=str(tmp_path / 'a'), **kw)
    loaded = dmc.DmcState.load(tmp_path / 'a' / 'dmc_state.npz')
    second, rows_b, _ = inference.run_dmc(slog, ld, dp, x0, cell, blocks=16, steps_per_block=10, tau=0.01, state=loaded, **kw)
    assert same_bits(state.arrays, second.arrays) == [] and (second.e_trial, second.e_ref, second.offset) == (state.e_trial, state.e_ref, state.offset)
    assert [r['energy'] for r in rows_a + rows_b] == [r['energy'] for r in rows]
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, steps_per_block=1, tau=0.01, pseudopotential=object())
    with pytest.raises(ValueError, match='multiple of branch_every'):
        inference.run_dmc(slog, ld, dp, x0, cell, blocks=1, steps_per_block=3, tau=0.01, branch_every=2, accumulators=(object(),))
