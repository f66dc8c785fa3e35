"""GPU tests of `ds_ecp_energy` (csrc/ds_ecp.h) against the numpy model of ecp_helpers.py: pair counts, the
Philox rotations, E_loc, the ratios and E_nl with the float64 CPU oracle's ratios (Philox and explicit rotations, both rules,
float32), a plane-wave determinant in closed form, chunked workspaces (bit-identical), the pair capacity, translations by cell
vectors, a NaN coordinate, the refusals of the C ABI, and the pseudopotential inside `train.make_loss` / `run_inference`.

Float64 tolerance on a ratio: TOL_Q max(1, |q_ref|) with TOL_Q = 2 (1e-9 + 1e-8), the bound test_gpu_onebody.py uses for the same
quantity; on a walker's E_nl the sum over its configurations of |W / N_q| TOL_Q max(1, |q_ref|).  E_loc: float64 arithmetic on
identical inputs, (8 + terms added) 2^-52 sum |term|."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

import ecp_helpers as eh
import onebody_helpers as oh
import sampler_helpers as sh
from test_gpu_onebody import TOL_Q, TOL_Q_F32, complex_np, cu, dev_params, system

pytestmark = pytest.mark.gpu

EPS = eh.EPS
CASES = list(eh.CASES)
RULES = [(name, 12) for name in CASES] + [('lih', 6)]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(name, n_quad=12, f32=False, mode='philox', **kw):
    """-> (reference of the case, output of `ecp_energy` on its walkers with the rotations of (SEED, OFFSET))."""
    ref = eh.reference(name, n_quad, f32)
    dtype = torch.float32 if f32 else torch.float64
    sysd, dp, _ = system(name, dtype)
    rot = dict(rotations=cu(ref['rot'])) if mode == 'explicit' else dict(seed=eh.SEED, offset=eh.OFFSET)
    out = sysd.ecp_energy(dp, cu(ref['x'], dtype), ref['ecp'], want_pairs=True, want_ratios=True, want_rotations=True, **rot, **kw)
    return ref, out


def e_loc_bound(ref):
    return (8 + ref['e_loc_terms']) * EPS * ref['e_loc_mag']


# ------------------------------------------------------------------------------------------------ 1. pairs
@pytest.mark.parametrize('name', CASES)
def test_pair_counts_equal_the_table_and_the_model(name):
    ref, out = run(name)
    pairs = out['pairs'].cpu().numpy()
    assert pairs.dtype == np.int64 and pairs.tolist() == eh.CASES[name][1]
    assert np.array_equal(pairs, ref['pairs']['counts'])
    assert out['ratios'].shape == (pairs.sum() * 12,)


# ------------------------------------------------------------------------------------------------ 2. rotations
def test_philox_rotations_equal_the_replay_and_are_orthogonal():
    """B = 37: the rotations equal the numpy replay of Philox stream 4 to 1e-15 absolute (sin and cos differ between libm and the
    device, so not bit for bit) and are orthogonal to 1e-15; another offset or seed gives other rotations; explicit rotations
    come back as given."""
    fx, cell, _, _, _ = sh.case('lih')
    sysd, dp, _ = system('lih')
    ecp = eh.fixture('lih')['ecp']
    B = 37
    x = cu(sh.tiled_walkers(cell, fx['x'], B))
    want = eh.replay_rotations(eh.SEED, eh.OFFSET, B)
    got = sysd.ecp_energy(dp, x, ecp, seed=eh.SEED, offset=eh.OFFSET, want_rotations=True)['rotations'].cpu().numpy()
    assert got.shape == (B, 3, 3) and got.dtype == np.float64
    print(f'max |Rot - replay| = {np.abs(got - want).max():.2e}, max |Rot Rot^T - 1| = {np.abs(got @ got.transpose(0, 2, 1) - np.eye(3)).max():.2e}')
    assert np.abs(got - want).max() <= 1e-15
    assert np.abs(got @ got.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-15
    assert np.abs(got.transpose(0, 2, 1) @ got - np.eye(3)).max() <= 1e-15
    assert np.all(np.abs(np.linalg.det(got) - 1) < 1e-14)
    for kw in (dict(seed=eh.SEED, offset=eh.OFFSET + 1), dict(seed=eh.SEED + 1, offset=eh.OFFSET)):
        other = sysd.ecp_energy(dp, x, ecp, want_rotations=True, **kw)['rotations'].cpu().numpy()
        assert np.abs(other - eh.replay_rotations(kw['seed'], kw['offset'], B)).max() <= 1e-15
        assert np.abs(other - got).max() > 0.1
    back = sysd.ecp_energy(dp, x, ecp, rotations=cu(want), want_rotations=True)['rotations']
    assert torch.equal(back, cu(want))


# ------------------------------------------------------------------------------------------------ 3. E_loc
@pytest.mark.parametrize('name,n_quad', RULES)
def test_e_loc_vs_model(name, n_quad):
    ref, out = run(name, n_quad)
    got = out['e_loc'].cpu().numpy()
    err, bound = np.abs(got - ref['e_loc']), e_loc_bound(ref)
    print(f'{name}: E_loc = {got}, max |E_loc - model| = {err.max():.2e}, bounds {bound}')
    assert ref['e_loc_terms'].sum() > 0 and out['e_loc'].dtype == torch.float64
    assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------ 4. ratios and E_nl
def check_against_reference(ref, out, tol, n_quad):
    q, q_ref = complex_np(out['ratios']), ref['q']
    assert q.shape == q_ref.shape and np.all(np.isfinite(q_ref))
    if len(q):
        err = np.abs(q - q_ref) / np.maximum(1.0, np.abs(q_ref))
        print(f'max scaled |q - q_ref| = {err.max():.3e} (tolerance {tol:.1e}), |q| in [{np.abs(q_ref).min():.3g}, {np.abs(q_ref).max():.3g}]')
        assert err.max() <= tol
    e = complex_np(out['e_nl'])
    bound = tol * ref['e_nl_scale']
    print(f'E_nl = {e}, max |E_nl - model| = {np.abs(e - ref["e_nl"]).max():.3e}, bounds {bound}')
    assert np.all(np.abs(e - ref['e_nl']) <= bound)
    empty = ref['pairs']['counts'] == 0
    assert np.all(e[empty] == 0)                                                  # no pair: exactly 0
    # the energy is the sum of the call's own terms: the model's weights times the call's ratios, to the rounding of the sum
    # (float64 ratios) or of the ratios as returned (float32)
    mine, scale = eh.energy(q, ref['Wn'], ref['pairs'], len(e), n_quad)
    assert np.all(np.abs(e - mine) <= (64 * EPS if out['ratios'].dtype == torch.complex128 else 2.0 ** -23) * scale)


@pytest.mark.parametrize('mode', ['philox', 'explicit'])
@pytest.mark.parametrize('name,n_quad', RULES)
def test_ratios_and_e_nl_vs_oracle(name, n_quad, mode):
    ref, out = run(name, n_quad, mode=mode)
    assert out['e_nl'].dtype == torch.complex128 and out['ratios'].dtype == torch.complex128
    assert np.abs(out['rotations'].cpu().numpy() - ref['rot']).max() <= 1e-15
    check_against_reference(ref, out, TOL_Q, n_quad)
    if name == 'li_polarized':
        assert ref['pairs']['counts'][0] == 0
    if name == 'lih_twist':
        assert ref['pairs']['counts'][2] == 0


# ------------------------------------------------------------------------------------------------ 5. float32
def test_float32_system_vs_float32_oracle():
    """The float32 system reads float32 positions and widens them: pairs and E_loc are those of the model on the rounded walkers
    (the same float64 bound), ratios and E_nl meet the float32 oracle within TOL_Q_F32."""
    ref, out = run('lih', f32=True)
    assert out['ratios'].dtype == torch.complex64 and out['e_nl'].dtype == torch.complex128 and out['e_loc'].dtype == torch.float64
    assert out['pairs'].tolist() == eh.CASES['lih'][1]
    assert np.all(np.abs(out['e_loc'].cpu().numpy() - ref['e_loc']) <= e_loc_bound(ref))
    check_against_reference(ref, out, TOL_Q_F32, 12)


# ------------------------------------------------------------------------------------------------ 6. plane waves
def test_plane_wave_determinant_ratios_equal_the_closed_form():
    """The plane-wave network of onebody_helpers on LiH with a twist, independent of the oracle: q from positions alone."""
    fx, cell, klist, _, _ = sh.case('lih_twist')
    pw_klist, net_kw, params, _, _ = oh.plane_wave_case(cell, klist)
    sysd, dp, _ = system('lih_twist', klist=pw_klist, net_kw=net_kw, params=params)
    f = eh.fixture('lih_twist')
    x, ecp, pl = f['x'], f['ecp'], f['pairs']
    rot = eh.replay_rotations(eh.SEED, eh.OFFSET, len(x))
    want = eh.plane_wave_config_ratios(x, pl, rot, 12, pw_klist, (2, 2))
    out = sysd.ecp_energy(dp, cu(x), ecp, seed=eh.SEED, offset=eh.OFFSET, want_ratios=True)
    q = complex_np(out['ratios'])
    err = np.abs(q - want) / np.maximum(1.0, np.abs(want))
    print(f'plane waves: max scaled |q - q_closed| = {err.max():.3e}, |q| up to {np.abs(want).max():.3g}')
    assert len(q) == 72 and err.max() <= TOL_Q
    e, scale = eh.energy(want, eh.weights(ecp, pl, rot, 12), pl, len(x), 12)
    assert np.all(np.abs(complex_np(out['e_nl']) - e) <= TOL_Q * scale)


# ------------------------------------------------------------------------------------------------ 7. chunks
def test_two_group_workspace_gives_identical_bits():
    """lih tiled to B = 37, N_q = 12: 135 pairs, 1620 configurations = 21 groups of 80.  A workspace cut to two groups runs chunks
    of 160 configurations, so walkers' segments straddle chunk borders; out_energy and out_ratio are bit-identical to the
    one-chunk run.  Below one group the call fails."""
    fx, cell, _, _, _ = sh.case('lih')
    sysd, dp, _ = system('lih')
    ecp = eh.fixture('lih')['ecp']
    B = 37
    x = cu(sh.tiled_walkers(cell, fx['x'], B))
    kw = dict(seed=eh.SEED, offset=eh.OFFSET, want_pairs=True, want_ratios=True)
    big = sysd.ecp_energy(dp, x, ecp, **kw)
    with pytest.raises(RuntimeError, match='workspace too small') as e:
        sysd.ecp_energy(dp, x, ecp, max_bytes=1, **kw)
    one = int(re.search(r'< (\d+) for one group', str(e.value)).group(1))
    full = int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, ecp.__dict__['_ds_tables'].handle, B, B * 4))
    groups = (B * 4 * 12 + 79) // 80                                              # what the full workspace holds: 23
    per = (full - one) / (groups - 1)
    assert per > 4096
    two = one + int(per) + 2048                                                   # room for two groups, not for three
    small = sysd.ecp_energy(dp, x, ecp, max_bytes=two, **kw)
    off = np.concatenate([[0], np.cumsum(big['pairs'].cpu().numpy())]) * 12
    assert off[-1] == 1620
    borders = np.arange(160, off[-1], 160)
    assert any(np.any((borders > lo) & (borders < hi)) for lo, hi in zip(off[:-1], off[1:]))       # a segment straddles a border
    assert torch.equal(torch.view_as_real(small['ratios']), torch.view_as_real(big['ratios']))
    assert torch.equal(small['e_loc'], big['e_loc']) and torch.equal(torch.view_as_real(small['e_nl']), torch.view_as_real(big['e_nl']))
    assert torch.equal(small['pairs'], big['pairs'])
    again = sysd.ecp_energy(dp, x, ecp, max_bytes=two, **kw)
    assert torch.equal(torch.view_as_real(again['e_nl']), torch.view_as_real(small['e_nl']))
    assert bool(big['e_nl'].abs().min() > 0)
    with pytest.raises(RuntimeError, match='workspace too small'):
        sysd.ecp_energy(dp, x, ecp, max_bytes=one - 1, **kw)


# ------------------------------------------------------------------------------------------------ 8. capacity
def raw_call(sysd, tables, p, x, B, cap, energy, ws, ws_bytes=None, rotations=None):
    return sysd.lib.ds_ecp_energy(sysd.handle, tables.handle, ptr(p), ptr(x), B, eh.SEED, eh.OFFSET, ptr(rotations), cap, ptr(energy),
                                  ptr(None), ptr(None), ptr(None), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, stream())


def test_capacity_one_below_the_need_fails_with_the_number_and_writes_no_energy():
    from deepsolid_amd.device import EcpTables
    ref = eh.reference('lih')
    sysd, dp, _ = system('lih')
    tables = EcpTables(ref['ecp'])
    x = cu(ref['x'])
    B, need = len(ref['x']), int(ref['pairs']['counts'].sum())
    assert need == 22
    p = sysd.pack_params(dp)
    energy = torch.full((B, 3), 7.0, dtype=torch.float64, device='cuda')
    ws = sysd._workspace('ds_ecp_workspace_bytes', tables.handle, B, need)
    assert raw_call(sysd, tables, p, x, B, need - 1, energy, ws) != 0
    msg = sysd.lib.ds_last_error().decode()
    assert 'pair capacity exceeded' in msg and f'{need} pairs' in msg and str(need - 1) in msg, msg
    torch.cuda.synchronize()
    assert bool((energy == 7.0).all())
    assert raw_call(sysd, tables, p, x, B, need, energy, ws) == 0                 # exactly the need runs
    torch.cuda.synchronize()
    assert np.all(np.abs(energy[:, 0].cpu().numpy() - ref['e_loc']) <= e_loc_bound(ref))
    assert np.all(np.abs(complex_np(torch.complex(energy[:, 1], energy[:, 2])) - ref['e_nl']) <= TOL_Q * ref['e_nl_scale'])


def test_wrapper_retries_once_with_the_needed_capacity():
    """Three walkers with all four electrons near the midpoint of Li and H (1.89 Bohr from both, inside both spheres): 8 pairs per
    walker, 24 > B N = 12, the default capacity.  The wrapper reads the number from the message and succeeds on its second call;
    a given capacity that is too small is raised the same way."""
    f = eh.fixture('lih')
    ecp = f['ecp']
    sysd, dp, _ = system('lih')
    rng = np.random.default_rng(4)
    mid = np.asarray([0.5 * ecp.atoms[1][0], 0.0, 0.0])                           # H has an image at (a / 2, 0, 0)
    assert np.all(np.abs(eh.min_image(mid[None, :], ecp.atoms, ecp.a)[0] - 1.89) < 0.01)
    x = (mid[None, None, :] + rng.uniform(-0.15, 0.15, (3, 4, 3))).reshape(3, 12)
    pl = eh.pair_list(ecp, x)
    assert pl['counts'].tolist() == [8, 8, 8]
    out = sysd.ecp_energy(dp, cu(x), ecp, seed=eh.SEED, offset=eh.OFFSET, want_pairs=True, want_ratios=True)
    assert out['pairs'].tolist() == [8, 8, 8] and out['pair_capacity'] == 24 and out['ratios'].shape == (24 * 12,)
    assert bool(torch.isfinite(torch.view_as_real(out['e_nl'])).all())
    low = sysd.ecp_energy(dp, cu(x), ecp, seed=eh.SEED, offset=eh.OFFSET, pair_capacity=5)
    assert low['pair_capacity'] == 24 and torch.equal(torch.view_as_real(low['e_nl']), torch.view_as_real(out['e_nl']))


# ------------------------------------------------------------------------------------------------ 9. translation
@pytest.mark.parametrize('name', ['lih_twist', 'bcc_li'])
def test_translation_by_cell_vectors_leaves_the_outputs(name):
    """All electrons of walker w moved by a simulation-cell vector n_w . a: the minimum image, and with it E_loc and the pairs, is
    the same up to the rounding of the coordinates, and psi only takes the twist phase, which cancels in every ratio."""
    ref, out = run(name)
    sysd, dp, _ = system(name)
    a = np.asarray(ref['cell'].a, dtype=np.float64).reshape(3, 3)
    n = np.asarray([[1, 0, 0], [-1, 2, 0], [0, -1, 1], [2, 1, -2]])[:len(ref['x'])]
    xt = (ref['x'].reshape(len(n), -1, 3) + (n @ a)[:, None, :]).reshape(len(n), -1)
    assert eh.pair_list(ref['ecp'], xt)['counts'].tolist() == eh.CASES[name][1]
    moved = sysd.ecp_energy(dp, cu(xt), ref['ecp'], seed=eh.SEED, offset=eh.OFFSET, want_pairs=True)
    assert torch.equal(moved['pairs'], out['pairs'])
    # E_loc: r moves by the rounding of coordinates of size |x| + |n . a| <= 40 Bohr, 40 x 2^-52 relative to r >= 0.1: take the
    # model's own E_loc on the moved walkers as the reference of the float64 bound
    e_loc, mag, cnt = eh.local_energy(ref['ecp'], xt)
    assert np.all(np.abs(moved['e_loc'].cpu().numpy() - e_loc) <= (8 + cnt) * EPS * mag)
    assert np.all(np.abs(e_loc - ref['e_loc']) <= 1e-12 * mag)
    assert np.all(np.abs(complex_np(moved['e_nl']) - ref['e_nl']) <= TOL_Q * ref['e_nl_scale'])


# ------------------------------------------------------------------------------------------------ 10. NaN
def test_nan_coordinate_gives_nan_for_that_walker_only():
    ref, out = run('lih')
    sysd, dp, _ = system('lih')
    x = np.array(ref['x'])
    x[2, 7] = np.nan
    bad = sysd.ecp_energy(dp, cu(x), ref['ecp'], seed=eh.SEED, offset=eh.OFFSET, want_pairs=True, want_ratios=True)
    e_loc, e_nl = bad['e_loc'].cpu().numpy(), complex_np(bad['e_nl'])
    assert np.isnan(e_loc[2]) and np.isnan(e_nl[2].real) and np.isnan(e_nl[2].imag)
    counts = list(eh.CASES['lih'][1])
    counts[2] = 0
    assert bad['pairs'].tolist() == counts
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(bad['e_loc'][keep], out['e_loc'][keep])
    assert torch.equal(torch.view_as_real(bad['e_nl'])[keep], torch.view_as_real(out['e_nl'])[keep])
    assert bad['ratios'].shape == ((22 - 3) * 12,) and bool(torch.isfinite(torch.view_as_real(bad['ratios'])).all())


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_refusals_launch_nothing():
    import test_ecp_cpu as cpu
    from deepsolid_amd.device import EcpTables
    from deepsolid_amd.pseudopotential import SemiLocalECP
    cpu.test_library_repeats_the_creation_refusals_before_touching_a_device()    # the creation-time refusals, on this device too
    ref = eh.reference('lih')
    sysd, dp, _ = system('lih')
    tables = EcpTables(ref['ecp'])
    x = cu(ref['x'])
    B, cap = len(ref['x']), 24
    p = sysd.pack_params(dp)
    energy = torch.full((B, 3), 7.0, dtype=torch.float64, device='cuda')
    ws = sysd._workspace('ds_ecp_workspace_bytes', tables.handle, B, cap)
    other_atoms = EcpTables(eh.fixture('bcc_li')['ecp'])
    cell = ref['cell']
    scaled = types.SimpleNamespace(a=1.001 * np.asarray(cell.a), atom_coords=cell.atom_coords, atom_charges=cell.atom_charges)
    sp = dict(local=[(2, 1.0, 1.0)], channels=[[(2, 1.0, 1.0)]], r_cut_loc=1.0, r_cut_nl=1.0)
    other_cell = EcpTables(SemiLocalECP(scaled, [sp], [0, 0]))
    bad = [('B must be', dict(B=0)), ('out_energy', dict(energy=None)), ('pair_capacity must be', dict(cap=0)),
           ('workspace too small', dict(ws_bytes=4096)), ('atoms', dict(tables=other_atoms)), ('cell differs', dict(tables=other_cell))]
    good = dict(tables=tables, B=B, cap=cap, energy=energy, ws_bytes=None)
    for word, kw in bad:
        a = {**good, **kw}
        assert raw_call(sysd, a['tables'], p, x, a['B'], a['cap'], a['energy'], ws, a['ws_bytes']) != 0, kw
        msg = sysd.lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
    assert sysd.lib.ds_ecp_workspace_bytes(sysd.handle, other_atoms.handle, B, cap) == -1
    with pytest.raises(ValueError):
        sysd.ecp_energy(dp, x, tables, rotations=torch.zeros(B, 9, dtype=torch.float64, device='cuda'))
    torch.cuda.synchronize()
    assert bool((energy == 7.0).all())
    assert raw_call(sysd, tables, p, x, B, cap, energy, ws) == 0                  # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not bool((energy == 7.0).any())


# ------------------------------------------------------------------------------------------------ 12. make_loss, run_inference
def test_make_loss_with_pseudopotential():
    """aux.local_energy == ke + ew + E_loc + E_nl elementwise and the loss is its mean; the packed gradient equals `logpsi_vjp`
    called by hand with the cotangent built from that E_L; without the keyword, loss and gradient are bit-identical to a
    `make_loss` built without it."""
    from deepsolid_amd import hamiltonian, network, train
    ref = eh.reference('lih')
    _, cell, kl, kw, p = sh.case('lih')
    net = network.make_solid_fermi_net(klist=kl, simulation_cell=cell, method_name='eval_logdet', **kw)
    sysd, dp = net.apply.system, dev_params(p)
    x = cu(ref['x'])
    B = len(ref['x'])
    total = train.make_loss(net.apply, None, cell, clip_local_energy=0.0, pseudopotential=ref['ecp'], key=eh.SEED)
    assert total.pseudopotential_energy.seed == eh.SEED and total.pseudopotential_energy.offset == 0
    loss, aux = total(dp, x)
    assert total.pseudopotential_energy.offset == 1
    ke, ew = hamiltonian.local_energy_seperate(net.apply, cell)(dp, x)
    pp = sysd.ecp_energy(dp, x, ref['ecp'], seed=eh.SEED, offset=0)
    e_l = ke + ew + (pp['e_loc'] + pp['e_nl'])
    assert torch.equal(torch.view_as_real(aux.local_energy), torch.view_as_real(e_l))
    assert torch.equal(torch.view_as_real(aux.pseudopotential), torch.view_as_real(pp['e_loc'] + pp['e_nl']))
    assert bool(aux.pseudopotential.abs().min() > 1e-3) and torch.equal(torch.view_as_real(aux.kinetic), torch.view_as_real(ke)) and torch.equal(aux.ewald, ew)
    assert abs(float(loss) - float(e_l.real.mean())) <= B * EPS * float(e_l.abs().sum())
    assert abs(float(aux.imaginary) - float(e_l.imag.mean())) <= B * EPS * float(e_l.abs().sum())
    assert float(aux.n_nonfinite) == 0.0
    # gradient (second call: offset 1)
    (loss2, aux2), flat = total.value_and_grad_packed(dp, x)
    assert total.pseudopotential_energy.offset == 2
    assert not torch.equal(torch.view_as_real(aux2.local_energy), torch.view_as_real(aux.local_energy))   # other rotations
    cot = (aux2.local_energy - loss2) / B
    by_hand, _, _ = sysd.logpsi_vjp(dp, x, cot)
    assert torch.equal(flat, by_hand) and bool(flat.abs().sum() > 0)
    # without the keyword: the same bits as a make_loss that never heard of it
    plain = train.make_loss(net.apply, None, cell)
    none = train.make_loss(net.apply, None, cell, pseudopotential=None)
    (l0, a0), g0 = plain.value_and_grad_packed(dp, x)
    (l1, a1), g1 = none.value_and_grad_packed(dp, x)
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(torch.view_as_real(a0.local_energy), torch.view_as_real(a1.local_energy))
    assert a1.pseudopotential is None and none.pseudopotential_energy is None
    assert torch.equal(torch.view_as_real(a0.local_energy), torch.view_as_real(ke + ew))


def test_run_inference_writes_the_pseudopotential_column(tmp_path):
    import csv
    import realspace_helpers as rh
    from deepsolid_amd import inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(16)
    ecp = eh.make_ecp(cell, eh.CASES['lih'][0])
    kw = dict(iterations=2, key=17, move_width=0.3, mcmc_steps=4, burn_in=2)
    _, _, rows = inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(tmp_path / 'pp'), pseudopotential=ecp, **kw)
    assert len(rows) == 2 and all(np.isfinite(complex(r['pseudopotential'])) for r in rows)
    with open(tmp_path / 'pp' / 'train_stats.csv') as f:
        table = list(csv.DictReader(f))
    assert len(table) == 2 and 'pseudopotential' in table[0] and complex(table[1]['pseudopotential']) == rows[1]['pseudopotential']
    _, _, plain = inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(tmp_path / 'plain'), **kw)
    with open(tmp_path / 'plain' / 'train_stats.csv') as f:
        assert 'pseudopotential' not in f.readline()
    assert 'pseudopotential' not in plain[0]
    # the walkers do not depend on the Hamiltonian, so the energy differs by the pseudopotential's mean alone
    for r, q in zip(rows, plain):
        assert abs(r['energy'] - q['energy'] - r['pseudopotential'].real) <= 1e-10 * max(1.0, abs(r['energy']))
