"""GPU tests of `ds_ion_forces` (csrc/ds_force.h), `DeviceSystem.ion_forces` and `estimator.IonForces`: the
Hellmann-Feynman and the zero-variance force per walker against the float64 CPU references of force_helpers.py (autograd of the
oracle's Ewald sum; grad and Laplacian of Q by autograd) on the smallest cells that reach every branch of the kernel, the direct
sincos path against the phase tables, a walker 1e-3 bohr from a nucleus, a float32 handle, the packed sums against a numpy model of
their order (bit for bit, also with a one-group workspace), the refusals of the C ABI, and the accumulator end to end.

Float64 tolerance: 1e-9 max(1, |ref|) per component, the scale of the Ewald parity tolerance of test_gpu_parity.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import force_helpers as fh
import sampler_helpers as sh
from common import load_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
EPS = 2.0 ** -52


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


def drift_of(sysd, dp, x):
    return sysd.logpsi_grad(dp, x)[1].real.contiguous()


def scaled_error(got, ref):
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


@functools.lru_cache(maxsize=None)
def evaluated(name, nb):
    """The first `nb` fixture walkers of a case through the call and through the helper, once:
    -> dict(x, drift (numpy, from `logpsi_grad` of the fixture parameters), hf, zv (the call), hf_ref, zv_ref, r_c)."""
    sysd, dp, _, fx, cell = system(name)
    x = cu(fx['x'][:nb])
    d = drift_of(sysd, dp, x)
    out = sysd.ion_forces(x, d)
    assert out['n_bad'].tolist() == [0] and out['sums'] is None
    r_c = sysd.force_cutoff()
    hf_ref, zv_ref = fh.reference(fh.ewald(cell), x.cpu().numpy(), d.cpu().numpy(), r_c)
    return dict(x=x.cpu().numpy(), drift=d.cpu().numpy(), hf=out['hf'].cpu().numpy(), zv=out['zv'].cpu().numpy(), hf_ref=hf_ref,
                zv_ref=zv_ref, r_c=r_c)


# ------------------------------------------------------------------------------------------------ 1. per-walker forces vs the helper
@pytest.mark.parametrize('name,nb', [('h2', 3), ('lih_2x1x1', 3), ('graphene_hex', 2), ('lih_fcc', 3), ('li_polarized', 3), ('diamond', 1)])
def test_forces_vs_helper(name, nb):
    """h2, B = 3: fewer pairs than threads; lih_2x1x1: N A 27 and NG beyond one stride of 256 threads; graphene_hex, lih_fcc: the
    general 27-shift minimal image; li_polarized: A = 1; diamond, one walker: the largest A (16) and N (96) of the fixtures (its
    electron phase tables exceed the kernel's LDS cap: the structure factors take the direct path there without DS_EWALD_DIRECT)."""
    from deepsolid_amd import estimator
    e = evaluated(name, nb)
    sysd, _, _, _, cell = system(name)
    A = len(cell.atom_charges())
    assert e['hf'].shape == e['zv'].shape == (nb, A, 3) and e['hf'].dtype == np.float64
    assert e['r_c'] == estimator.wigner_seitz_radius(cell.a)
    inside = fh.min_ion_distance(fh.ewald(cell), e['x']).min() < e['r_c']
    assert inside == (name != 'h2')      # (the h2 walkers are spread over a 4 x 100 x 100 bohr cell: none within 2 bohr of an ion)
    assert (np.abs(e['zv_ref'] - e['hf_ref']).max() > 1e-3) == inside            # the zero-variance term is there
    err_hf, err_zv = scaled_error(e['hf'], e['hf_ref']).max(), scaled_error(e['zv'], e['zv_ref']).max()
    print(f'{name}: max scaled error hf {err_hf:.3e}, zv {err_zv:.3e} (tolerance {TOL:.1e}); max |hf| = {np.abs(e["hf_ref"]).max():.3g}, '
          f'max |zv| = {np.abs(e["zv_ref"]).max():.3g}')
    assert err_hf <= TOL and err_zv <= TOL
    # hf alone needs no drift and is the same bits; a smaller cutoff changes zv only
    x = cu(e['x'])
    alone = sysd.ion_forces(x)
    assert alone['zv'] is None and np.array_equal(alone['hf'].cpu().numpy(), e['hf'])
    half = sysd.ion_forces(x, cu(e['drift']), cutoff=0.5 * e['r_c'])
    assert np.array_equal(half['hf'].cpu().numpy(), e['hf'])
    # (reference: the closed form of the term, equal to autograd to 1e-10 in test_force_cpu.py, on the autograd HF force above)
    zv_half = e['hf_ref'] + fh.zv_delta_closed(fh.ewald(cell), e['x'], e['drift'], 0.5 * e['r_c'])
    assert scaled_error(half['zv'].cpu().numpy(), zv_half).max() <= TOL


def test_direct_sincos_path(monkeypatch):
    """bcc_li on a handle made with DS_EWALD_DIRECT=1 (no phase tables: g_len = 0): the helper within 1e-9 max(1, |ref|), and
    the table path of the cached handle within 1e-9."""
    tab = evaluated('bcc_li', 2)
    fx, cell, kl, kw, p = load_case('bcc_li')                  # a fresh cell: the handle is cached on the cell
    monkeypatch.setenv('DS_EWALD_DIRECT', '1')
    sysd, dp, _ = make_system(cell, kl, kw, p)
    monkeypatch.delenv('DS_EWALD_DIRECT')
    out = sysd.ion_forces(cu(tab['x']), cu(tab['drift']))
    hf, zv = out['hf'].cpu().numpy(), out['zv'].cpu().numpy()
    e_tab = max(scaled_error(tab['hf'], tab['hf_ref']).max(), scaled_error(tab['zv'], tab['zv_ref']).max())
    e_dir = max(scaled_error(hf, tab['hf_ref']).max(), scaled_error(zv, tab['zv_ref']).max())
    between = max(np.abs(hf - tab['hf']).max(), np.abs(zv - tab['zv']).max())
    print(f'bcc_li: max scaled error tables {e_tab:.3e}, direct {e_dir:.3e}; max |direct - tables| = {between:.3e}')
    assert e_tab <= TOL and e_dir <= TOL and between <= 1e-9
    assert between > 0.0                                        # two different code paths ran


# ------------------------------------------------------------------------------------------------ 2. a walker near a nucleus
def near_nucleus_walkers(fx, cell):
    """The lih fixture walkers with electron 0 of walker 0 moved to 1e-3 bohr from the Li nucleus (ion 0)."""
    x = np.array(fx['x'], np.float64).reshape(len(fx['x']), -1, 3)
    u = np.array([0.6, -0.64, 0.48])
    x[0, 0] = np.asarray(cell.atom_coords())[0] + 1e-3 * u / np.linalg.norm(u)
    return x.reshape(len(x), -1)


def test_near_nucleus_walker():
    """Electron 0 at r = 1e-3 bohr from Li (Z = 3): F^hf is of size Z / r^2 = 3e6 there, F^zv stays O(1).  zv within
    4 eps Z / r^2 + 1e-9 of the helper (which forms the cancellation as a difference of two numbers of that size and loses that
    much), and |zv| at least 100 x smaller than |hf| on that ion."""
    sysd, dp, _, fx, cell = system('lih')
    assert cell.atom_charges()[0] == 3
    x = cu(near_nucleus_walkers(fx, cell)[:2])
    d = drift_of(sysd, dp, x)
    out = sysd.ion_forces(x, d)
    assert out['n_bad'].tolist() == [0]
    hf, zv = out['hf'].cpu().numpy(), out['zv'].cpu().numpy()
    hf_ref, zv_ref = fh.reference(fh.ewald(cell), x.cpu().numpy(), d.cpu().numpy(), sysd.force_cutoff())
    bound = 4 * EPS * 3 / 1e-3 ** 2 + 1e-9
    print(f'lih near nucleus: |hf| = {np.linalg.norm(hf[0, 0]):.4e}, |zv| = {np.linalg.norm(zv[0, 0]):.4e}, '
          f'max |zv - ref| = {np.abs(zv - zv_ref).max():.3e} (bound {bound:.3e}), max scaled hf error = {scaled_error(hf, hf_ref).max():.3e}')
    assert np.abs(zv - zv_ref).max() <= bound
    assert scaled_error(hf, hf_ref).max() <= TOL
    assert np.linalg.norm(hf[0, 0]) > 1e6 and 100 * np.linalg.norm(zv[0, 0]) <= np.linalg.norm(hf[0, 0])


# ------------------------------------------------------------------------------------------------ 3. float32
@pytest.mark.parametrize('name,nb', [('lih', 3), ('diamond', 1)])
def test_float32_handle(name, nb):
    """A float32 handle: x and the drift (float32 `logpsi_grad` of the float32 parameters) are float32, the arithmetic is float64
    on the handle's float32 tables.  Reference: the float64 helper at the same rounded inputs.  Tolerance per walker, the pattern of
    `common.float32_tolerance`: 3 x the scaled deviation of the helper with ITS tables rounded to float32 from the helper with
    float64 tables (that walker's, or the mean over the walkers where it is larger) + 1e-6.  The table deviation is taken with
    the closed form of the zero-variance term (test_force_cpu.py: equal to autograd to 1e-10).  lih includes the walker 1e-3 bohr
    from the Li nucleus."""
    sysd, dp, _, fx, cell = system(name, torch.float32)
    x64 = near_nucleus_walkers(fx, cell) if name == 'lih' else np.array(fx['x'], np.float64)
    x = cu(x64[:nb], torch.float32)
    d = drift_of(sysd, dp, x)
    assert d.dtype == torch.float32
    out = sysd.ion_forces(x, d)
    assert out['hf'].dtype == torch.float64 and out['n_bad'].tolist() == [0]
    xr, dr = x.double().cpu().numpy(), d.double().cpu().numpy()
    r_c = sysd.force_cutoff()
    ew, ew32 = fh.ewald(cell), fh.ewald(cell, tables32=True)
    hf_ref, zv_ref = fh.reference(ew, xr, dr, r_c)
    hf_64 = fh.hf_force(ew, xr)
    hf_32 = fh.hf_force(ew32, xr)
    zv_64 = hf_64 + fh.zv_delta_closed(ew, xr, dr, r_c)
    zv_32 = hf_32 + fh.zv_delta_closed(ew32, xr, dr, r_c)
    for what, got, ref, a64, a32 in (('hf', out['hf'], hf_ref, hf_64, hf_32), ('zv', out['zv'], zv_ref, zv_64, zv_32)):
        dev = scaled_error(a32, a64).reshape(nb, -1).max(axis=1)
        err = scaled_error(got.cpu().numpy(), ref).reshape(nb, -1).max(axis=1)
        tol = 3 * np.maximum(dev, dev.mean()) + 1e-6
        print(f'{name} float32 {what}: table deviation per walker {np.array2string(dev, precision=3)}, error of the call '
              f'{np.array2string(err, precision=3)}, tolerance {np.array2string(tol, precision=3)}')
        assert np.all(err <= tol)


# ------------------------------------------------------------------------------------------------ 4. sums
def test_sums_bit_for_bit_and_one_group_workspace():
    """Two calls, B = 5 then B = 3, into one buffer: the numpy model of the order bit for bit; the same with the workspace capped
    to one group; B = 600 walkers (three groups) with a one-group workspace (three passes) against a full one and the model."""
    sysd, dp, _, fx, cell = system('lih')
    A = 2
    x = cu(np.concatenate([fx['x'], fx['x'][:2] + 0.05]))
    d = drift_of(sysd, dp, x)
    one_group = 8 * (256 * 6 * A + 12 * A + 1)
    assert int(sysd.lib.ds_ion_forces_workspace_bytes(sysd.handle, 8)) == one_group
    assert int(sysd.lib.ds_ion_forces_workspace_bytes(sysd.handle, 600)) == 3 * one_group
    for cap in (None, one_group):
        sums = torch.zeros(12 * A + 1, dtype=torch.float64, device='cuda')
        model = np.zeros(12 * A + 1)
        for sl in (slice(0, 5), slice(5, 8)):
            out = sysd.ion_forces(x[sl], d[sl], sums=sums, max_bytes=cap)
            assert out['sums'] is sums
            model = fh.sums_model(model, out['hf'].cpu().numpy(), out['zv'].cpu().numpy())
        assert np.array_equal(sums.cpu().numpy(), model) and model[12 * A] == 8
    # sums alone: the same bits without the walker outputs
    alone = torch.zeros_like(sums)
    for sl in (slice(0, 5), slice(5, 8)):
        o = sysd.ion_forces(x[sl], d[sl], sums=alone, want_walker=False)
        assert o['hf'] is None and o['zv'] is None
    assert torch.equal(alone, sums)
    # several groups, several passes
    big = x.repeat(75, 1) + torch.linspace(0, 0.2, 600, dtype=torch.float64, device='cuda')[:, None]
    dbig = drift_of(sysd, dp, big)
    full, capped = torch.zeros_like(sums), torch.zeros_like(sums)
    of = sysd.ion_forces(big, dbig, sums=full)
    oc = sysd.ion_forces(big, dbig, sums=capped, max_bytes=one_group + 100)
    assert torch.equal(full, capped) and torch.equal(of['hf'], oc['hf']) and torch.equal(of['zv'], oc['zv'])
    assert np.array_equal(full.cpu().numpy(), fh.sums_model(np.zeros(12 * A + 1), of['hf'].cpu().numpy(), of['zv'].cpu().numpy()))
    # run to run
    again = torch.zeros_like(sums)
    oa = sysd.ion_forces(big, dbig, sums=again)
    assert torch.equal(again, full) and torch.equal(oa['zv'], of['zv'])


def test_bad_walker_is_nan_left_out_and_counted():
    sysd, dp, _, fx, cell = system('lih')
    A = 2
    x = cu(np.concatenate([fx['x'], fx['x'][:2] + 0.05]))
    d = drift_of(sysd, dp, x)
    x[3, 4] = float('nan')
    sums = torch.zeros(12 * A + 1, dtype=torch.float64, device='cuda')
    out = sysd.ion_forces(x, d, sums=sums)
    hf, zv = out['hf'].cpu().numpy(), out['zv'].cpu().numpy()
    good = np.arange(8) != 3
    assert np.isnan(hf[3]).all() and np.isnan(zv[3]).all() and np.isfinite(hf[good]).all() and np.isfinite(zv[good]).all()
    assert out['n_bad'].tolist() == [1] and float(sums[12 * A]) == 7
    assert np.array_equal(sums.cpu().numpy(), fh.sums_model(np.zeros(12 * A + 1), hf, zv))
    # a non-finite drift: the same
    x[3, 4] = 0.1
    d[5, 0] = float('inf')
    out = sysd.ion_forces(x, d)
    assert out['n_bad'].tolist() == [1] and np.isnan(out['zv'].cpu().numpy()[5]).all() and np.isnan(out['hf'].cpu().numpy()[5]).all()
    assert np.isfinite(out['zv'].cpu().numpy()[np.arange(8) != 5]).all()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing():
    sysd, dp, _, fx, cell = system('lih')
    lib, A = sysd.lib, 2
    x = cu(fx['x'])
    B = x.shape[0]
    d = drift_of(sysd, dp, x)
    r_ws = sysd.force_cutoff()
    hf = torch.full((B, A, 3), 7.0, dtype=torch.float64, device='cuda')
    zv = torch.full((B, A, 3), 7.0, dtype=torch.float64, device='cuda')
    sums = torch.zeros(12 * A + 1, dtype=torch.float64, device='cuda')
    n_bad = torch.zeros(1, dtype=torch.int64, device='cuda')
    ws = sysd._workspace('ds_ion_forces_workspace_bytes', B)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(x=x, d=d, B=B, r_c=r_ws, hf=hf, zv=zv, sums=sums, ws_bytes=ws.numel())

    def call(**kw):
        a = {**good, **kw}
        return lib.ds_ion_forces(sysd.handle, ptr(a['x']), ptr(a['d']), a['B'], a['r_c'], None, ptr(a['hf']), ptr(a['zv']), ptr(a['sums']),
                                 ptr(n_bad), ptr(ws), a['ws_bytes'], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [('cutoff', dict(r_c=1.001 * r_ws)), ('cutoff', dict(r_c=0.0)), ('cutoff', dict(r_c=float('nan'))), ('drift', dict(d=None)),
           ('drift', dict(d=None, zv=None)), ('B must be', dict(B=0)), ('null', dict(x=None)),
           ('nothing to write', dict(hf=None, zv=None, sums=None)), ('workspace too small', dict(ws_bytes=4096))]
    for word, kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
    with pytest.raises(ValueError, match='cutoff'):
        sysd.ion_forces(x, d, cutoff=1.001 * r_ws)
    with pytest.raises(ValueError, match='drift'):
        sysd.ion_forces(x, None, sums=sums)
    with pytest.raises(ValueError, match='sums'):
        sysd.ion_forces(x, d, sums=torch.zeros(3, dtype=torch.float64, device='cuda'))
    torch.cuda.synchronize()
    assert not sums.any() and bool((hf == 7.0).all()) and bool((zv == 7.0).all()) and n_bad.tolist() == [0]
    # B = 0 through the wrapper: empty tensors, no library call
    empty = sysd.ion_forces(x[:0], d[:0], sums=sums)
    assert empty['hf'].shape == (0, A, 3) and empty['zv'].shape == (0, A, 3) and empty['n_bad'].tolist() == [0] and not sums.any()
    assert call() == 0                                                     # the same arguments, unbroken, run
    assert call(d=None, zv=None, sums=None) == 0                           # hf alone needs neither a drift nor a workspace
    torch.cuda.synchronize()
    assert float(sums[12 * A]) == B and bool((hf != 7.0).all()) and bool((zv != 7.0).all())


# ------------------------------------------------------------------------------------------------ 6. the accumulator
def test_ion_forces_accumulator_end_to_end(tmp_path):
    """Two updates of 4 walkers, a merge with a second accumulator, save / load: the means of `forces()` equal the mean of the
    per-walker output of `DeviceSystem.ion_forces` to 1e-12; `run_inference` takes the accumulator for two iterations."""
    import realspace_helpers as rh
    from deepsolid_amd import estimator, inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(12)
    sysd = ld.apply.system
    acc = estimator.IonForces(ld, dp)
    acc.update(x0[:4])
    acc.update(x0[4:8])
    second = estimator.IonForces(ld, dp)
    second.update(x0[8:])
    acc.merge(second)
    path = str(tmp_path / 'forces.npz')
    acc.save(path)
    loaded = estimator.IonForces.load(path)
    per = sysd.ion_forces(x0, drift_of(sysd, dp, x0))
    r = loaded.forces()
    assert r['n_walkers'] == 12 and r['n_bad'] == 0 and r['cutoff'] == sysd.force_cutoff()
    for k in ('hf', 'zv'):
        want = per[k].cpu().numpy()
        assert np.abs(r[k] - want.mean(axis=0)).max() <= 1e-12 * max(1.0, np.abs(want).max())
        np.testing.assert_allclose(r[k + '_error'], want.std(axis=0) / np.sqrt(11), rtol=1e-6)
        np.testing.assert_array_equal(acc.forces()[k], r[k])
    run = estimator.IonForces(ld, dp, cutoff=0.8 * sysd.force_cutoff())
    inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(tmp_path), accumulators=(run,), iterations=2, key=17,
                            move_width=0.3, mcmc_steps=4, burn_in=2)
    assert run.reduced and run.n_walkers == 24
    rr = run.forces()
    assert rr['n_bad'] == 0 and np.isfinite(rr['zv']).all() and np.isfinite(rr['zv_error']).all() and (rr['zv_error'] > 0).all()
    with np.load(str(tmp_path / 'realspace.npz')) as f:
        for k in ('sums', 'n_bad', 'n_walkers', 'atoms', 'charges', 'latvec', 'cutoff', 'hf', 'hf_error', 'zv', 'zv_error'):
            assert k in f.files, k
        assert int(f['n_walkers']) == 24 and float(f['sums'][24]) == 24
