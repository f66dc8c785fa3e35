"""GPU tests of `ds_ecp_forces` (csrc/ds_ecp_force.h) against the numpy model of ecp_force_helpers.py: F^loc
and F^nl with the float64 CPU oracle's ratios and walker gradients (both rules, a twist, full determinants, one spin channel, bcc-Li,
float32), central differences of `ds_ecp_energy` in the ion positions on the device, bit identity (repeat, one-group workspace,
batch of 300, Philox rotations), `sums` and `base` against a float64 replay of the documented order, the edges (NaN coordinate, no
pair, capacity, refusals) and `estimator.PseudopotentialForces` inside `run_inference`.

Tolerances are the project's own for the two quantities involved: TOL_Q (test_gpu_onebody.py) on a ratio and grad_tolerance_f64
(test_gpu_samplers.py) on a walker gradient.  F^nl per (walker, ion, component): the sum over the ion's configurations of
(1 / N_q) [ TOL_Q max(1, |rho|) (|D_q| + |W_q| |J g_q|) + 2 |W_q| |rho| TOL_G ].  F^loc: float64 arithmetic on identical inputs,
(8 + terms added) 2^-52 sum |term|, the bound of test_gpu_ecp.py for E_loc."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

import ecp_force_helpers as fh
import ecp_helpers as eh
import force_helpers
import sampler_helpers as sh
from test_gpu_onebody import TOL_Q, TOL_Q_F32, complex_np, cu, system
from test_gpu_samplers import grad_tolerance_f64

pytestmark = pytest.mark.gpu

EPS = eh.EPS
MODEL_CASES = [('lih', 12), ('lih_twist', 12), ('lih', 6), ('lih_fulldet', 12), ('li_polarized', 12)]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(name, n_quad=12, f32=False, n_walkers=None, **kw):
    """-> (reference of the case, output of `ecp_forces` on its walkers with the explicit rotations of the reference)."""
    ref = fh.reference(name, n_quad, f32, n_walkers)
    dtype = torch.float32 if f32 else torch.float64
    sysd, dp, _ = system(name, dtype)
    return ref, sysd.ecp_forces(dp, cu(ref['x'], dtype), ref['ecp'], rotations=cu(ref['rot']), **kw)


def tol_g_f64(ref):
    g = torch.as_tensor(ref['g_all'])
    return max(grad_tolerance_f64(g.real), grad_tolerance_f64(g.imag)) if g.numel() else 0.0


def check_against_model(ref, out, tol_q, tol_g, n_quad):
    B, A = len(ref['x']), len(ref['ecp'].atoms)
    loc, nl = out['loc'].cpu().numpy(), complex_np(out['nl'])
    assert loc.shape == (B, A, 3) and nl.shape == (B, A, 3) and out['loc'].dtype == torch.float64 and out['nl'].dtype == torch.complex128
    assert out['pairs'].tolist() == ref['pairs']['counts'].tolist() and int(out['n_bad']) == 0
    err_loc, bound_loc = np.abs(loc - ref['f_loc']), ((8 + ref['f_loc_terms']) * EPS * ref['f_loc_mag'])[..., None]
    print(f'max |F_loc - model| = {err_loc.max():.2e} (largest bound {bound_loc.max():.2e}), max |F_loc| = {np.abs(loc).max():.3f}')
    assert ref['f_loc_terms'].sum() > 0 and np.all(err_loc <= bound_loc)
    bound = fh.nonlocal_scale(ref['pairs'], B, A, n_quad, ref['q'], ref['D'], ref['W'], ref['Jg'], tol_q, tol_g)[..., None]
    err = np.abs(nl - ref['f_nl'])
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.nan))
    print(f'max |F_nl - model| = {err.max():.3e}, largest error / bound = {worst:.3e}, max |F_nl| = {np.abs(nl).max():.3f}, tol_g = {tol_g:.2e}')
    assert np.all(err <= bound)
    assert np.abs(ref['f_nl']).max() > 0.1
    empty = ref['pairs']['counts'] == 0
    assert np.all(nl[empty] == 0)                                                 # no pair: exactly 0


# ------------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize('name,n_quad', MODEL_CASES)
def test_forces_vs_model(name, n_quad):
    ref, out = run(name, n_quad)
    assert np.abs(out['rotations'].cpu().numpy() - ref['rot']).max() == 0
    check_against_model(ref, out, TOL_Q, tol_g_f64(ref), n_quad)
    if name == 'li_polarized':
        assert ref['pairs']['counts'][0] == 0
    if name == 'lih_twist':
        assert ref['pairs']['counts'][2] == 0 and np.abs(ref['f_nl'].imag).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 2. bcc_li
def test_bcc_li_first_two_walkers_vs_model():
    """24 electrons, 8 ions, 15 and 14 pairs: several electrons per ion, all eight ions of the walker kernel's two rounds, and several
    slot tiles in the chain."""
    ref, out = run('bcc_li', n_walkers=2)
    assert ref['pairs']['counts'].tolist() == eh.CASES['bcc_li'][1][:2] and len(ref['ecp'].atoms) == 8
    assert len(set(ref['pairs']['I'].tolist())) == 8
    check_against_model(ref, out, TOL_Q, tol_g_f64(ref), 12)


# ------------------------------------------------------------------------------------------------ 3. float32
def test_float32_system_vs_float32_oracle():
    """The float32 system reads float32 positions and widens them: F^loc is that of the model on the rounded walkers (the same
    float64 bound); F^nl meets the float32 oracle within TOL_Q_F32 on the ratios and TOL_G_F32 (4 x the measured loss of the
    float32 oracle's own gradient, ecp_force_helpers.py) on the gradients."""
    ref, out = run('lih', f32=True)
    check_against_model(ref, out, TOL_Q_F32, fh.TOL_G_F32, 12)


# ------------------------------------------------------------------------------------------------ 4. consistency with the energy
def test_central_differences_of_the_device_energy_equal_the_device_force():
    """`ds_ecp_energy` with descriptors whose atom I is displaced by +-1e-4 Bohr along each axis, the same rotations: the central
    difference of E_loc + E_nl meets -(F^loc + F^nl) within the Richardson bound of the CPU test plus 2 TOL_Q e_nl_scale / h for the
    rounding of the two energies."""
    ref, out = run('lih')
    sysd, dp, _ = system('lih')
    d = fh.energy_differences('lih')
    x, rot = cu(ref['x']), cu(ref['rot'])
    f = out['loc'].cpu().numpy() + complex_np(out['nl'])
    fh.assert_no_pair_flips(ref['ecp'], ref['x'], fh.H)
    worst = 0.0
    for I in range(f.shape[1]):
        for c in range(3):
            e = []
            for sign in (1, -1):
                o = sysd.ecp_energy(dp, x, fh.moved(ref['ecp'], I, c, sign * fh.H), rotations=rot)
                e.append(o['e_loc'].cpu().numpy() + complex_np(o['e_nl']))
            diff = -(e[0] - e[1]) / (2 * fh.H)
            bound = d['bound'][:, I, c] + 2 * TOL_Q * ref['e_nl_scale'] / fh.H
            err = np.abs(diff - f[:, I, c])
            worst = max(worst, float(err.max()))
            assert np.all(err <= bound), (I, c, err, bound)
    print(f'max |central difference of the device energy + force| = {worst:.3e}, max |F| = {np.abs(f).max():.3f}')
    assert np.abs(f).max() > 1.0


# ------------------------------------------------------------------------------------------------ 5. bit identity
def same_bits(a, b):
    return torch.equal(a['loc'], b['loc']) and torch.equal(torch.view_as_real(a['nl']), torch.view_as_real(b['nl']))


def lih_batch(B):
    """The six lih fixture walkers repeated to B rows (not wrapped: the first six rows are the fixture's bits) and their rotations."""
    ref = fh.reference('lih')
    n = (B + 5) // 6
    return ref, cu(np.tile(ref['x'], (n, 1))[:B]), cu(np.tile(ref['rot'], (n, 1, 1))[:B])


def test_two_calls_and_a_one_group_workspace_give_identical_bits():
    """lih, N_q = 12: 22 pairs, 264 configurations, 36-60 per walker.  A workspace of exactly one 80-configuration group runs four
    chunks, so walkers' configurations straddle chunk borders; the forces are bit-identical to the default workspace and to a second
    call.  Below one group the call fails."""
    ref, out = run('lih')
    _, again = run('lih')
    assert same_bits(out, again)
    sysd, dp, _ = system('lih')
    x, rot = cu(ref['x']), cu(ref['rot'])
    with pytest.raises(RuntimeError, match='workspace too small') as e:
        sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, max_bytes=1)
    one = int(re.search(r'< (\d+) for one group of 80', str(e.value)).group(1))
    full = int(sysd.lib.ds_ecp_forces_workspace_bytes(sysd.handle, ref['ecp'].__dict__['_ds_tables'].handle, 6, 24))
    assert full > one + 4096                                                      # the default holds more than one group
    small = sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, max_bytes=one)
    off = np.concatenate([[0], np.cumsum(ref['pairs']['counts'])]) * 12
    borders = np.arange(80, off[-1], 80)
    assert off[-1] == 264 and any(np.any((borders > lo) & (borders < hi)) for lo, hi in zip(off[:-1], off[1:]))
    assert same_bits(small, out) and torch.equal(small['pairs'], out['pairs'])
    assert bool(out['nl'].abs().max() > 0.1)
    with pytest.raises(RuntimeError, match='workspace too small'):
        sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, max_bytes=one - 1)


def test_six_walkers_inside_a_batch_of_300_give_identical_bits():
    """B = 300 crosses the 256-walker group of the sums and runs 13200 configurations in several chunks: the first six walkers are
    those of the B = 6 call, bit for bit, and every copy of a walker equals the first."""
    ref, out = run('lih')
    sysd, dp, _ = system('lih')
    _, x, rot = lih_batch(300)
    big = sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot)
    assert big['pairs'].sum().item() == 50 * 22
    assert torch.equal(big['loc'][:6], out['loc']) and torch.equal(torch.view_as_real(big['nl'][:6]), torch.view_as_real(out['nl']))
    assert torch.equal(big['loc'][294:], out['loc']) and torch.equal(torch.view_as_real(big['nl'][294:]), torch.view_as_real(out['nl']))


def test_philox_rotations_equal_the_replay_and_those_of_the_energy_call():
    ref = fh.reference('lih')
    sysd, dp, _ = system('lih')
    x = cu(ref['x'])
    out = sysd.ecp_forces(dp, x, ref['ecp'], seed=eh.SEED, offset=eh.OFFSET)
    got = out['rotations'].cpu().numpy()
    assert np.abs(got - eh.replay_rotations(eh.SEED, eh.OFFSET, len(ref['x']))).max() <= 1e-15
    energy = sysd.ecp_energy(dp, x, ref['ecp'], seed=eh.SEED, offset=eh.OFFSET, want_rotations=True)
    assert torch.equal(out['rotations'], energy['rotations'])
    # the same points, given back explicitly: the same bits
    assert same_bits(sysd.ecp_forces(dp, x, ref['ecp'], rotations=out['rotations']), out)
    other = sysd.ecp_forces(dp, x, ref['ecp'], seed=eh.SEED, offset=eh.OFFSET + 1)
    assert np.abs(other['rotations'].cpu().numpy() - got).max() > 0.1 and not same_bits(other, out)


# ------------------------------------------------------------------------------------------------ 6. sums and base
def test_sums_equal_the_replay_of_the_documented_order_and_are_added_to():
    """B = 300 (two groups of the sums, the second partial): `sums` equals the float64 replay -- per group the tree over the 256
    walkers, the groups in order -- of F^pp = F^loc + Re F^nl and F^tot = F^pp + base, to the last bit; without a base F^tot = F^pp;
    a second call adds to the first; a one-group workspace gives the same sums."""
    ref, x, rot = lih_batch(300)
    sysd, dp, _ = system('lih')
    A = 2
    base = cu(np.random.default_rng(7).standard_normal((300, A, 3)))
    sums = torch.zeros(12 * A + 1, dtype=torch.float64, device='cuda')
    out = sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, base=base, sums=sums)
    assert out['sums'] is sums
    f_pp = out['loc'].cpu().numpy() + out['nl'].real.cpu().numpy()
    f_tot = f_pp + base.cpu().numpy()
    want = force_helpers.sums_model(np.zeros(12 * A + 1), f_pp, f_tot)
    assert want[12 * A] == 300 and np.array_equal(sums.cpu().numpy(), want)
    # added to, never zeroed; the walker outputs are not needed for the sums
    sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, base=base, sums=sums, want_walker=False)
    assert np.array_equal(sums.cpu().numpy(), force_helpers.sums_model(want, f_pp, f_tot))
    plain = torch.zeros_like(sums)
    sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, sums=plain, want_walker=False)
    assert np.array_equal(plain.cpu().numpy(), force_helpers.sums_model(np.zeros(12 * A + 1), f_pp, f_pp))
    with pytest.raises(RuntimeError, match='workspace too small') as e:
        sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, sums=plain, max_bytes=1)
    one = int(re.search(r'< (\d+) for one group of 80', str(e.value)).group(1))
    small = torch.zeros_like(sums)
    sysd.ecp_forces(dp, x, ref['ecp'], rotations=rot, base=base, sums=small, want_walker=False, max_bytes=one)
    assert np.array_equal(small.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 7. edges
def test_nan_coordinate_gives_nan_for_that_walker_only_and_is_counted():
    ref, out = run('lih')
    sysd, dp, _ = system('lih')
    x = np.array(ref['x'])
    x[2, 7] = np.nan
    sums = torch.zeros(25, dtype=torch.float64, device='cuda')
    bad = sysd.ecp_forces(dp, cu(x), ref['ecp'], rotations=cu(ref['rot']), sums=sums)
    assert bool(torch.isnan(bad['loc'][2]).all()) and bool(torch.isnan(torch.view_as_real(bad['nl'][2])).all())
    assert int(bad['n_bad']) == 1 and float(sums[24]) == 5
    counts = list(eh.CASES['lih'][1])
    counts[2] = 0
    assert bad['pairs'].tolist() == counts
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(bad['loc'][keep], out['loc'][keep])
    assert torch.equal(torch.view_as_real(bad['nl'])[keep], torch.view_as_real(out['nl'])[keep])
    f_pp = bad['loc'].cpu().numpy() + bad['nl'].real.cpu().numpy()
    assert np.array_equal(sums.cpu().numpy(), force_helpers.sums_model(np.zeros(25), f_pp, f_pp))


def test_no_pair_at_all_gives_zero_nonlocal_force_and_the_local_force_of_the_model():
    """A non-local cutoff below every distance of the batch (the local one as usual): no chunk is launched, F^nl is exactly 0 and
    F^loc is the model's."""
    from deepsolid_amd.pseudopotential import SemiLocalECP
    ref = fh.reference('lih')
    sysd, dp, cell = system('lih')
    r_cut = eh.CASES['lih'][0]
    species = [dict(local=s['local'], channels=s['channels'], r_cut_loc=eh.LOCAL_FRACTION * r_cut, r_cut_nl=0.05)
               for s in (eh.SPECIES_A, eh.SPECIES_B)]
    ecp = SemiLocalECP(cell, species, [0, 1])
    assert eh.min_image(ref['x'], ecp.atoms, ecp.a)[0].min() > 0.06
    out = sysd.ecp_forces(dp, cu(ref['x']), ecp, seed=1, offset=2)
    assert out['pairs'].tolist() == [0] * 6 and int(out['n_bad']) == 0
    assert bool((torch.view_as_real(out['nl']) == 0).all())
    f_loc, mag, cnt = fh.local_force(ecp, ref['x'])
    assert np.abs(f_loc).max() > 0.1
    assert np.all(np.abs(out['loc'].cpu().numpy() - f_loc) <= ((8 + cnt) * EPS * mag)[..., None])


def raw_call(sysd, tables, p, x, B, cap, force, ws, ws_bytes=None, sums=None, rotations=None):
    return sysd.lib.ds_ecp_forces(sysd.handle, tables.handle, ptr(p), ptr(x), B, eh.SEED, eh.OFFSET, ptr(rotations), cap, ptr(None),
                                  ptr(force), ptr(sums), ptr(None), ptr(None), ptr(None), ptr(ws),
                                  ws.numel() if ws_bytes is None else ws_bytes, stream())


def test_capacity_overflow_message_and_the_retry_of_the_wrapper():
    """Capacity one below the need: the message carries the number and nothing is written.  Three walkers with all four electrons
    inside both spheres (8 pairs each, 24 > B N = 12, the default capacity): the wrapper reads the number and succeeds on its second
    call; a given capacity that is too small is raised the same way."""
    from deepsolid_amd.device import EcpTables
    ref = fh.reference('lih')
    sysd, dp, _ = system('lih')
    ecp = ref['ecp']
    tables = EcpTables(ecp)
    x = cu(ref['x'])
    B, need = 6, 22
    p = sysd.pack_params(dp)
    force = torch.full((B, 2, 3, 3), 7.0, dtype=torch.float64, device='cuda')
    ws = sysd._workspace('ds_ecp_forces_workspace_bytes', tables.handle, B, need)
    assert raw_call(sysd, tables, p, x, B, need - 1, force, ws) != 0
    msg = sysd.lib.ds_last_error().decode()
    assert 'pair capacity exceeded' in msg and f'{need} pairs' in msg and str(need - 1) in msg, msg
    torch.cuda.synchronize()
    assert bool((force == 7.0).all())
    assert raw_call(sysd, tables, p, x, B, need, force, ws, rotations=cu(ref['rot'])) == 0    # exactly the need runs
    torch.cuda.synchronize()
    _, out = run('lih')
    assert torch.equal(force[..., 0], out['loc']) and torch.equal(force[..., 1], out['nl'].real)
    rng = np.random.default_rng(4)
    mid = np.asarray([0.5 * ecp.atoms[1][0], 0.0, 0.0])
    xs = (mid[None, None, :] + rng.uniform(-0.15, 0.15, (3, 4, 3))).reshape(3, 12)
    assert eh.pair_list(ecp, xs)['counts'].tolist() == [8, 8, 8]
    got = sysd.ecp_forces(dp, cu(xs), ecp, seed=eh.SEED, offset=eh.OFFSET)
    assert got['pairs'].tolist() == [8, 8, 8] and got['pair_capacity'] == 24
    assert bool(torch.isfinite(torch.view_as_real(got['nl'])).all()) and int(got['n_bad']) == 0
    low = sysd.ecp_forces(dp, cu(xs), ecp, seed=eh.SEED, offset=eh.OFFSET, pair_capacity=5)
    assert low['pair_capacity'] == 24 and same_bits(low, got)


def test_refusals_launch_nothing():
    from deepsolid_amd.device import EcpTables
    from deepsolid_amd.pseudopotential import SemiLocalECP
    ref = fh.reference('lih')
    sysd, dp, _ = system('lih')
    tables = EcpTables(ref['ecp'])
    x = cu(ref['x'])
    B, cap = len(ref['x']), 24
    p = sysd.pack_params(dp)
    force = torch.full((B, 2, 3, 3), 7.0, dtype=torch.float64, device='cuda')
    sums = torch.full((25,), 7.0, dtype=torch.float64, device='cuda')
    ws = sysd._workspace('ds_ecp_forces_workspace_bytes', tables.handle, B, cap)
    other_atoms = EcpTables(eh.fixture('bcc_li')['ecp'])
    cell = ref['cell']
    scaled = types.SimpleNamespace(a=1.001 * np.asarray(cell.a), atom_coords=cell.atom_coords, atom_charges=cell.atom_charges)
    sp = dict(local=[(2, 1.0, 1.0)], channels=[[(2, 1.0, 1.0)]], r_cut_loc=1.0, r_cut_nl=1.0)
    other_cell = EcpTables(SemiLocalECP(scaled, [sp], [0, 0]))
    bad = [('B must be', dict(B=0)), ('nothing to write', dict(force=None)), ('pair_capacity must be', dict(cap=0)),
           ('workspace too small', dict(ws_bytes=4096)), ('workspace too small', dict(ws_bytes=4096, force=None, sums=sums)),
           ('atoms', dict(tables=other_atoms)), ('cell differs', dict(tables=other_cell)), ('null', dict(p=None)), ('null', dict(x=None))]
    good = dict(tables=tables, B=B, cap=cap, force=force, ws_bytes=None, sums=None, p=p, x=x)
    for word, kw in bad:
        a = {**good, **kw}
        assert raw_call(sysd, a['tables'], a['p'], a['x'], a['B'], a['cap'], a['force'], ws, a['ws_bytes'], a['sums']) != 0, kw
        msg = sysd.lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
    assert sysd.lib.ds_ecp_forces_workspace_bytes(sysd.handle, other_atoms.handle, B, cap) == -1
    for kw in (dict(rotations=torch.zeros(B, 9, dtype=torch.float64, device='cuda')),
               dict(base=torch.zeros(B, 2, dtype=torch.float64, device='cuda')),
               dict(sums=torch.zeros(24, dtype=torch.float64, device='cuda')), dict(want_walker=False)):
        with pytest.raises(ValueError):
            sysd.ecp_forces(dp, x, tables, **kw)
    torch.cuda.synchronize()
    assert bool((force == 7.0).all()) and bool((sums == 7.0).all())
    assert raw_call(sysd, tables, p, x, B, cap, force, ws) == 0                   # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not bool((force == 7.0).any())


# ------------------------------------------------------------------------------------------------ 8. the accumulator
class _Recorder:
    """An accumulator that keeps the walkers it is shown."""

    def __init__(self):
        self.seen = []

    def update(self, data):
        self.seen.append(data.clone())

    def reduce(self):
        return self

    def save(self, path, results=False):
        pass


def test_pseudopotential_forces_in_run_inference(tmp_path):
    """Two iterations of 16 walkers: n_walkers adds up; pp is the mean of direct `ecp_forces` calls with the accumulator's seed and
    the offsets 0 and 1; total = pp + the mean of out_hf of a direct `ion_forces` call on the same walkers; save / load / merge."""
    import realspace_helpers as rh
    from deepsolid_amd import estimator, inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(16)
    sysd = ld.apply.system
    ecp = eh.make_ecp(cell, eh.CASES['lih'][0])
    rec, acc = _Recorder(), estimator.PseudopotentialForces(ld, dp, ecp, key=11)
    inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(tmp_path), accumulators=(rec, acc), pseudopotential=ecp,
                            iterations=2, key=17, move_width=0.3, mcmc_steps=4, burn_in=2)
    assert acc.reduced and acc.n_walkers == 32 and acc.offset == 2 and len(rec.seen) == 2
    r = acc.forces()
    assert r['n_bad'] == 0 and r['n_walkers'] == 32 and float(acc.sums[24]) == 32
    direct = [sysd.ecp_forces(dp, xs, ecp, seed=11, offset=k) for k, xs in enumerate(rec.seen)]
    pp = torch.cat([o['loc'] + o['nl'].real for o in direct]).cpu().numpy()
    hf = torch.cat([sysd.ion_forces(xs)['hf'] for xs in rec.seen]).cpu().numpy()
    scale = max(1.0, np.abs(pp).max(), np.abs(hf).max())
    assert np.abs(r['pp'] - pp.mean(axis=0)).max() <= 1e-12 * scale
    assert np.abs(r['total'] - (r['pp'] + hf.mean(axis=0))).max() <= 1e-12 * scale
    np.testing.assert_allclose(r['total_error'], (pp + hf).std(axis=0) / np.sqrt(31), rtol=1e-6)
    assert np.isfinite(r['pp_error']).all() and (r['pp_error'] > 0).all()
    with np.load(str(tmp_path / 'realspace_1.npz')) as f:
        for k in ('sums', 'n_bad', 'n_walkers', 'atoms', 'charges', 'latvec', 'seed', 'offset', 'ecp_term_c', 'pp', 'pp_error', 'total',
                  'total_error'):
            assert k in f.files, k
        assert int(f['n_walkers']) == 32
    loaded = estimator.PseudopotentialForces.load(str(tmp_path / 'realspace_1.npz'))
    np.testing.assert_array_equal(loaded.forces()['total'], r['total'])
    fresh = estimator.PseudopotentialForces(ld, dp, ecp, key=11)
    fresh.update(rec.seen[0])
    fresh.merge(loaded)
    assert fresh.n_walkers == 48 and float(fresh.sums[24].cpu()) == 48 and np.isfinite(fresh.forces()['total']).all()
