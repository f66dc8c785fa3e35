"""GPU tests of `ds_stress` (csrc/ds_stress.h), `DeviceSystem.stress` and `estimator.StressTensor`: the four rows
per walker against the float64 closed form of stress_helpers.py (itself checked against central differences of the oracle's energy on
strained cells in test_stress_cpu.py) on the cells that reach every branch of the kernel, the direct sincos path against the phase
tables, a float32 handle, the packed sums against a numpy model of their order (bit for bit, also with a one-group workspace), bad
walkers, the refusals of the C ABI, and the accumulator end to end.

Float64 tolerance: 1e-9 max(1, |ref|) per component, that of test_gpu_force.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sampler_helpers as sh
import stress_helpers as sth
from common import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(vv, dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v] for k, v in params.items()}


def make_system(cell, klist, net_kw, params, dtype=torch.float64):
    from deepsolid_amd import network
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', dtype=dtype, **net_kw)
    return net.apply.system, dev_params(params, dtype), net


def system(name, dtype=torch.float64):
    """-> (DeviceSystem of the case, device parameters, net, fixture, cell)."""
    fx, cell, kl, kw, p = sh.case(name)
    return make_system(cell, kl, kw, p, dtype) + (fx, cell)


def cu(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device='cuda')


def scaled_error(got, ref):
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


@functools.lru_cache(maxsize=None)
def evaluated(name, nb):
    """The first `nb` fixture walkers of a case through the call and through the helper, once:
    -> dict(x, grad (numpy complex, `logpsi_grad` of the fixture parameters), parts (the call), ref (B, 4, 6))."""
    sysd, dp, _, fx, cell = system(name)
    x = cu(fx['x'][:nb])
    grad = sysd.logpsi_grad(dp, x)[1]
    out = sysd.stress(x, grad)
    assert out['n_bad'].tolist() == [0] and out['sums'] is None
    g = grad.cpu().numpy()
    return dict(x=x.cpu().numpy(), grad=g, parts=out['parts'].cpu().numpy(), ref=sth.reference_parts(sth.ewald(cell), x.cpu().numpy(), g))


# ------------------------------------------------------------------------------------------------ 1. per-walker rows vs the helper
@pytest.mark.parametrize('name,nb', [('h2', 3), ('lih', 3), ('lih_twist', 3), ('li_polarized', 3), ('graphene_hex', 2), ('bcc_li', 2)])
def test_rows_vs_helper(name, nb):
    """h2: fewer pairs than threads, 307 024 G points (300 chunks); lih: the diagonal minimal image; lih_twist: a complex gradient, both
    halves enter kin; li_polarized: the fractional wrap of the bcc cell (dist_mode 1), A = 1; graphene_hex: the general 27-shift
    image of a non-orthogonal, anisotropic cell; bcc_li: 24 electrons, more pairs than threads.  The fixture walkers include
    electrons outside the cell.  The kin row is checked against the numpy contraction of the very gradient passed in."""
    e = evaluated(name, nb)
    sysd, _, _, fx, cell = system(name)
    assert e['parts'].shape == (nb, 4, 6) and e['parts'].dtype == np.float64
    lat = np.asarray(cell.a, np.float64)
    frac = e['x'].reshape(nb, -1, 3) @ np.linalg.inv(lat)
    assert (frac < 0).any() and (frac > 1).any()                 # electrons outside the cell are among them
    if name == 'lih_twist':
        assert np.abs(e['grad'].imag).max() > 1e-3
    for k, row in enumerate(('kin', 'ee', 'ei', 'total')):
        err = scaled_error(e['parts'][:, k], e['ref'][:, k]).max()
        print(f'{name} {row}: max scaled error {err:.3e} (tolerance {TOL:.1e}); max |ref| = {np.abs(e["ref"][:, k]).max():.4g}')
        assert err <= TOL
    assert np.abs(e['ref'][:, 0]).max() > 1e-3 and np.abs(e['ref'][:, 2, 3:]).max() > 1e-6       # kin is there; so are off-diagonal terms
    # without a gradient: the kinetic row is zero, ee and ei are the same bits, total is the Ewald part with the ion-ion constant
    alone = sysd.stress(cu(e['x']))['parts'].cpu().numpy()
    assert not alone[:, 0].any() and np.array_equal(alone[:, 1:3], e['parts'][:, 1:3])
    assert scaled_error(alone[:, 3], e['ref'][:, 3] - e['ref'][:, 0]).max() <= TOL


def test_direct_sincos_path(monkeypatch):
    """bcc_li on a handle made with DS_EWALD_DIRECT=1 (no phase tables: g_len = 0, the switch reaches this kernel through the handle):
    the helper within 1e-9 max(1, |ref|), and the table path of the cached handle within the same 1e-9 max(1, |ref|): both paths sum
    NG x N unit phases of relative error a few eps into S(G) (eps N NG^(1/2) w |S| ~ 1e-13 here).  Measured: 1.8e-15 between the
    paths, 1.6e-14 (tables) and 1.4e-14 (direct) against the helper."""
    tab = evaluated('bcc_li', 2)
    fx, cell, kl, kw, p = load_case('bcc_li')                  # a fresh cell: the handle is cached on the cell
    monkeypatch.setenv('DS_EWALD_DIRECT', '1')
    sysd, dp, _ = make_system(cell, kl, kw, p)
    monkeypatch.delenv('DS_EWALD_DIRECT')
    got = sysd.stress(cu(tab['x']), cu(tab['grad'], torch.complex128))['parts'].cpu().numpy()
    e_tab, e_dir = scaled_error(tab['parts'], tab['ref']).max(), scaled_error(got, tab['ref']).max()
    between = scaled_error(got, tab['parts']).max()
    print(f'bcc_li: max scaled error tables {e_tab:.3e}, direct {e_dir:.3e}; max scaled |direct - tables| = {between:.3e}')
    assert e_tab <= TOL and e_dir <= TOL and between <= TOL
    assert np.abs(got[:, 1:3] - tab['parts'][:, 1:3]).max() > 0.0        # two different code paths ran
    assert np.array_equal(got[:, 0], tab['parts'][:, 0])                # (the kinetic row does not depend on the path)


# ------------------------------------------------------------------------------------------------ 2. float32
@pytest.mark.parametrize('name,nb', [('lih', 3), ('diamond', 1)])
def test_float32_handle(name, nb):
    """A float32 handle: x and the gradient (float32 `logpsi_grad` of the float32 parameters) are float32, the arithmetic is float64 on
    the handle's float32 tables.  Reference: the float64 helper at the same rounded inputs.  Tolerance per walker and row, as in
    test_gpu_force.py: 3 x the scaled deviation of the helper with ITS tables rounded to float32 from the helper with float64 tables
    (that walker's, or the mean over the walkers where it is larger) + 1e-6.  The ion-ion constant comes from the host in float64
    in both.  diamond: 96 electrons, 16 ions; its phase tables do not fit the kernel's LDS cap, so this is the direct path too."""
    sysd, dp, _, fx, cell = system(name, torch.float32)
    x = cu(np.array(fx['x'], np.float64)[:nb], torch.float32)
    grad = sysd.logpsi_grad(dp, x)[1]
    assert grad.dtype == torch.complex64
    out = sysd.stress(x, grad)
    assert out['parts'].dtype == torch.float64 and out['n_bad'].tolist() == [0]
    xr, gr = x.double().cpu().numpy(), grad.to(torch.complex128).cpu().numpy()
    ref = sth.reference_parts(sth.ewald(cell), xr, gr)
    m32 = sth.reference_parts(sth.ewald(cell, tables32=True), xr, gr)
    ii64 = sth.to_voigt(sth.closed_form(sth.ewald(cell), xr[:1])[2])
    m32[:, 3] = m32[:, 0] + m32[:, 1] + m32[:, 2] + ii64[None]
    got = out['parts'].cpu().numpy()
    for k, row in enumerate(('kin', 'ee', 'ei', 'total')):
        dev = scaled_error(m32[:, k], ref[:, k]).max(axis=1)
        err = scaled_error(got[:, k], ref[:, k]).max(axis=1)
        tol = 3 * np.maximum(dev, dev.mean()) + 1e-6
        print(f'{name} float32 {row}: table deviation per walker {np.array2string(dev, precision=3)}, error of the call '
              f'{np.array2string(err, precision=3)}, tolerance {np.array2string(tol, precision=3)}')
        assert np.all(err <= tol)


# ------------------------------------------------------------------------------------------------ 3. sums
def lih_batch():
    sysd, dp, _, fx, cell = system('lih')
    x = cu(np.concatenate([fx['x'], fx['x'][:2] + 0.05]))
    return sysd, dp, x, sysd.logpsi_grad(dp, x)[1]


def test_sums_bit_for_bit_and_one_group_workspace():
    """Two calls, B = 5 then B = 3, into one buffer: the numpy model of the order bit for bit; the same with the workspace capped to one
    group; B = 600 walkers (three groups) with a one-group workspace (three passes) against a full one and the model."""
    sysd, dp, x, g = lih_batch()
    one_group = 8 * (256 * 24 + 49)
    assert int(sysd.lib.ds_stress_workspace_bytes(sysd.handle, 8)) == one_group
    assert int(sysd.lib.ds_stress_workspace_bytes(sysd.handle, 600)) == 3 * one_group
    for cap in (None, one_group):
        sums = torch.zeros(49, dtype=torch.float64, device='cuda')
        model = np.zeros(49)
        for sl in (slice(0, 5), slice(5, 8)):
            out = sysd.stress(x[sl], g[sl], sums=sums, max_bytes=cap)
            assert out['sums'] is sums
            model = sth.sums_model(model, out['parts'].cpu().numpy())
        assert np.array_equal(sums.cpu().numpy(), model) and model[48] == 8
    # sums alone: the same bits without the walker outputs
    alone = torch.zeros_like(sums)
    for sl in (slice(0, 5), slice(5, 8)):
        assert sysd.stress(x[sl], g[sl], sums=alone, want_walker=False)['parts'] is None
    assert torch.equal(alone, sums)
    # several groups, several passes
    big = x.repeat(75, 1) + torch.linspace(0, 0.2, 600, dtype=torch.float64, device='cuda')[:, None]
    gbig = sysd.logpsi_grad(dp, big)[1]
    full, capped = torch.zeros_like(sums), torch.zeros_like(sums)
    of = sysd.stress(big, gbig, sums=full)
    oc = sysd.stress(big, gbig, sums=capped, max_bytes=one_group + 100)
    assert torch.equal(full, capped) and torch.equal(of['parts'], oc['parts'])
    assert np.array_equal(full.cpu().numpy(), sth.sums_model(np.zeros(49), of['parts'].cpu().numpy())) and float(full[48]) == 600
    # run to run
    again = torch.zeros_like(sums)
    oa = sysd.stress(big, gbig, sums=again)
    assert torch.equal(again, full) and torch.equal(oa['parts'], of['parts'])


def test_bad_walker_is_nan_left_out_and_counted():
    sysd, dp, x, g = lih_batch()
    x[3, 4] = float('nan')
    sums = torch.zeros(49, dtype=torch.float64, device='cuda')
    out = sysd.stress(x, g, sums=sums)
    parts = out['parts'].cpu().numpy()
    good = np.arange(8) != 3
    assert np.isnan(parts[3]).all() and np.isfinite(parts[good]).all()
    assert out['n_bad'].tolist() == [1] and float(sums[48]) == 7
    assert np.array_equal(sums.cpu().numpy(), sth.sums_model(np.zeros(49), parts))
    # a non-finite gradient: the same
    x[3, 4] = 0.1
    g[5, 0] = complex(0.0, float('inf'))
    out = sysd.stress(x, g)
    parts = out['parts'].cpu().numpy()
    assert out['n_bad'].tolist() == [1] and np.isnan(parts[5]).all() and np.isfinite(parts[np.arange(8) != 5]).all()
    # two electrons at one point: a non-finite result, the same
    g[5, 0] = 0.0
    x[6, 3:6] = x[6, 0:3]
    out = sysd.stress(x, g)
    assert out['n_bad'].tolist() == [1] and np.isnan(out['parts'].cpu().numpy()[6]).all()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing():
    """Every refusal of the header comment but one returns an error with a message and launches nothing.  The one left out, a kernel
    LDS layout above 64 KB, cannot be reached: the layout without phase tables is 49.6 KB at the largest electron number a handle can
    be created with (128)."""
    sysd, dp, x, g = lih_batch()
    lib, B = sysd.lib, x.shape[0]
    gr = torch.view_as_real(g).contiguous()
    parts = torch.full((B, 4, 6), 7.0, dtype=torch.float64, device='cuda')
    sums = torch.zeros(49, dtype=torch.float64, device='cuda')
    n_bad = torch.zeros(1, dtype=torch.int64, device='cuda')
    ws = sysd._workspace('ds_stress_workspace_bytes', B)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(h=sysd.handle, x=x, g=gr, B=B, out=parts, sums=sums, ws=ws, ws_bytes=ws.numel())

    def call(**kw):
        a = {**good, **kw}
        return lib.ds_stress(a['h'], ptr(a['x']), ptr(a['g']), a['B'], None, ptr(a['out']), ptr(a['sums']), ptr(n_bad), ptr(a['ws']),
                             a['ws_bytes'], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [('null', dict(h=None)), ('null', dict(x=None)), ('B must be', dict(B=0)), ('B must be', dict(B=-3)),
           ('nothing to write', dict(out=None, sums=None)), ('need the gradient', dict(g=None)), ('need the gradient', dict(g=None, out=None)),
           ('workspace too small', dict(ws_bytes=8 * (256 * 24 + 49) - 1)), ('workspace too small', dict(ws=None))]
    for word, kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
    with pytest.raises(ValueError, match='grad'):
        sysd.stress(x, None, sums=sums)
    with pytest.raises(ValueError, match='sums'):
        sysd.stress(x, g, sums=torch.zeros(3, dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='grad'):
        sysd.stress(x, g.real.contiguous())
    with pytest.raises(ValueError, match='nothing'):
        sysd.stress(x, g, want_walker=False)
    torch.cuda.synchronize()
    assert not sums.any() and bool((parts == 7.0).all()) and n_bad.tolist() == [0]
    # B = 0 through the wrapper: empty tensors, no library call
    empty = sysd.stress(x[:0], g[:0], sums=sums)
    assert empty['parts'].shape == (0, 4, 6) and empty['n_bad'].tolist() == [0] and not sums.any()
    assert call() == 0                                                     # the same arguments, unbroken, run
    assert call(g=None, sums=None, ws=None, ws_bytes=0) == 0               # the Ewald rows alone need neither a gradient nor a workspace
    torch.cuda.synchronize()
    assert float(sums[48]) == B and bool((parts[:, 1:] != 7.0).all()) and not parts[:, 0].any()


# ------------------------------------------------------------------------------------------------ 5. the accumulator
def test_stress_tensor_accumulator_end_to_end(tmp_path):
    """Two updates of 150 walkers, save / load: `stress()` equals the per-walker output of `DeviceSystem.stress` reduced in numpy (means
    to 1e-12 of the largest entry, naive errors to 1e-6 relative); a merge doubles the walkers and keeps the means; `run_inference`
    takes the accumulator for two iterations."""
    import realspace_helpers as rh
    from deepsolid_amd import constants, estimator, inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(300)
    sysd = ld.apply.system
    acc = estimator.StressTensor(ld, dp)
    acc.update(x0[:150])
    acc.update(x0[150:])
    path = str(tmp_path / 'stress.npz')
    acc.save(path)
    loaded = estimator.StressTensor.load(path)
    per = sysd.stress(x0, sysd.logpsi_grad(dp, x0)[1])['parts'].cpu().numpy()
    V = abs(np.linalg.det(np.asarray(cell.a, np.float64)))
    r = loaded.stress()
    assert r['n_walkers'] == 300 and r['n_bad'] == 0 and abs(r['volume'] - V) <= 1e-12 * V
    want = estimator.voigt_to_matrix(per.mean(axis=0)) / V
    scale = np.abs(per).max() / V
    assert np.abs(r['sigma'] - want[3]).max() <= 1e-12 * scale
    for k, name in enumerate(('kin', 'ee', 'ei')):
        assert np.abs(r['parts'][name] - want[k]).max() <= 1e-12 * scale
    ii = sth.to_voigt(sth.closed_form(sth.ewald(cell), x0[:1].cpu().numpy())[2]) / V
    assert np.abs(r['parts']['ii'] - estimator.voigt_to_matrix(ii)).max() <= 1e-9 * max(1.0, np.abs(ii).max())
    np.testing.assert_allclose(r['sigma_error'], estimator.voigt_to_matrix(per[:, 3].std(axis=0, ddof=1) / np.sqrt(300)) / V, rtol=1e-6)
    tr = per[:, 3, :3].sum(axis=1)
    assert abs(r['pressure'] + tr.mean() / (3 * V)) <= 1e-12 * scale
    np.testing.assert_allclose(r['pressure_error'], tr.std(ddof=1) / np.sqrt(300) / (3 * V), rtol=1e-6)
    assert r['pressure_gpa'] == r['pressure'] * constants.HARTREE_PER_BOHR3_IN_GPA
    np.testing.assert_array_equal(acc.stress()['sigma'], r['sigma'])
    second = estimator.StressTensor(ld, dp)
    second.update(x0)
    merged = second.merge(loaded).stress()
    assert merged['n_walkers'] == 600 and np.abs(merged['sigma'] - r['sigma']).max() <= 1e-12 * scale
    run = estimator.StressTensor(ld, dp)
    inference.run_inference(slog, ld, dp, x0[:12].clone(), cell, save_path=str(tmp_path), accumulators=(run,), iterations=2, key=17,
                            move_width=0.3, mcmc_steps=4, burn_in=2)
    assert run.reduced and run.n_walkers == 24
    rr = run.stress()
    assert rr['n_bad'] == 0 and np.isfinite(rr['sigma']).all() and (rr['sigma_error'] > 0).all() and np.isfinite(rr['pressure_gpa'])
    with np.load(str(tmp_path / 'realspace.npz')) as f:
        for k in ('sums', 'trace_sums', 'n_bad', 'n_walkers', 'atoms', 'charges', 'latvec', 'sigma', 'sigma_error', 'pressure',
                  'pressure_error', 'pressure_gpa', 'volume'):
            assert k in f.files, k
        assert int(f['n_walkers']) == 24 and float(f['sums'][48]) == 24
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        estimator.StressTensor(ld, dp, pseudopotential=object())


# ------------------------------------------------------------------------------------------------ 6. the wave-function term
@pytest.mark.parametrize('name', ['lih', 'lih_twist'])
def test_strain_log_derivative_vs_oracle_network(name):
    """O = d log psi_eps((1 + eps) x) / d eps from the twelve strained handles against the same central differences (the same h) of
    the ORACLE network on the cells of `supercell.strained`, three fixture walkers.  Both sides make the same truncation error, so
    what is left is the error of the forwards: the parity bounds of test_gpu_parity.py for log|psi| (1e-9) and the phase (1e-8),
    each entering twice over 2h: 1e-9 / h for Re O and 1e-8 / h for Im O."""
    from deepsolid_amd import estimator
    sysd, dp, net, fx, cell = system(name)
    _, _, kl, kw, p = sh.case(name)
    acc = estimator.StressTensor(net, dp, wavefunction_term=True)
    assert acc.vmc_only and acc.strain_step == 1e-4
    x = cu(fx['x'][:3])
    O = acc.strain_log_derivative(x).cpu().numpy()
    handles = acc.strained_systems()
    assert len(handles) == 6 and len({id(h[0]) for h in handles} | {id(h[2]) for h in handles}) == 12
    assert acc.strained_systems() is handles                                    # built once
    ref, _ = sth.oracle_log_derivative(cell, kl, kw, p, fx['x'][:3], acc.strain_step)
    h = acc.strain_step
    print(f'{name}: max |O| = {np.abs(ref).max():.4g}; max |Re O - oracle| = {np.abs(O.real - ref.real).max():.3e} (bound {1e-9 / h:.1e}), '
          f'max |Im O - oracle| = {np.abs(O.imag - ref.imag).max():.3e} (bound {1e-8 / h:.1e})')
    assert O.shape == (3, 6) and np.abs(O.real - ref.real).max() <= 1e-9 / h and np.abs(O.imag - ref.imag).max() <= 1e-8 / h
    assert np.abs(ref.real).max() > 1e-2


def test_wavefunction_term_block_row_and_drivers(tmp_path):
    """One block of 40 lih walkers against its numpy restatement from `local_energy`, `stress` and `strain_log_derivative`
    (1e-11 of the row's largest entry); passing the energies in gives the same row; `stress()` has the total; `run_inference` takes
    the accumulator for two iterations (two blocks); `run_dmc` refuses it."""
    import realspace_helpers as rh
    from deepsolid_amd import estimator, inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(40)
    sysd = ld.apply.system
    acc, given = estimator.StressTensor(ld, dp, wavefunction_term=True), estimator.StressTensor(ld, dp, wavefunction_term=True)
    acc.update(x0)
    ke, ew, _, _ = sysd.local_energy(dp, x0)
    E = (ke[:, 0] + ew).cpu().numpy() + 1j * ke[:, 1].cpu().numpy()
    given.update(x0, energies=torch.as_tensor(E))
    total = sysd.stress(x0, sysd.logpsi_grad(dp, x0)[1])['parts'][:, 3].cpu().numpy()
    O = acc.strain_log_derivative(x0).cpu().numpy()
    dE = E - E.mean()
    model = np.concatenate([[40.0, E.real.sum(), E.imag.sum()], total.sum(axis=0), (np.conj(dE)[:, None] * O).real.sum(axis=0)])
    row = acc.rows.cpu().numpy()
    assert row.shape == (1, 15)
    dev = np.abs(row[0] - model).max() / np.abs(model).max()
    print(f'block row against the model: largest deviation {dev:.3e} of the largest entry; sum t = {row[0, 9:]}')
    assert dev <= 1e-11 and np.abs(row[0, 9:]).max() > 1e-6
    assert np.abs(given.rows.cpu().numpy() - row).max() <= 1e-11 * np.abs(model).max()
    acc.update(x0 + 0.01)
    r = acc.stress()
    V = r['volume']
    rows = acc.rows.cpu().numpy()
    want = ((rows[:, 3:9] / 40 + 2 * rows[:, 9:] / 39) / V).mean(axis=0)
    np.testing.assert_allclose(r['sigma_total'], estimator.voigt_to_matrix(want), rtol=1e-12, atol=1e-15)
    assert r['n_blocks'] == 2 and np.isfinite(r['sigma_total_error']).all() and np.isfinite(r['pressure_total_gpa'])
    np.testing.assert_allclose(r['sigma_total'] - r['wavefunction'], r['sigma'], rtol=1e-9, atol=1e-12)
    acc.save(str(tmp_path / 'stress_total.npz'))
    np.testing.assert_array_equal(estimator.StressTensor.load(str(tmp_path / 'stress_total.npz')).stress()['sigma_total'], r['sigma_total'])
    run = estimator.StressTensor(ld, dp, wavefunction_term=True)
    inference.run_inference(slog, ld, dp, x0[:12].clone(), cell, save_path=str(tmp_path), accumulators=(run,), iterations=2, key=17,
                            move_width=0.3, mcmc_steps=4, burn_in=2)
    rr = run.stress()
    assert run.reduced and rr['n_blocks'] == 2 and run.n_walkers == 24 and np.isfinite(rr['sigma_total']).all()
    with pytest.raises(ValueError, match='VMC'):
        inference.run_dmc(slog, ld, dp, x0[:12].clone(), cell, blocks=1, steps_per_block=4, tau=0.01,
                          accumulators=(estimator.StressTensor(ld, dp, wavefunction_term=True),))
    with pytest.raises(ValueError, match='float64'):
        estimator.StressTensor(system('lih', torch.float32)[2], None, wavefunction_term=True)
