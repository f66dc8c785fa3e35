"""GPU tests of `ds_hf_orbitals_at`, `ds_obdm_accumulate` (csrc/ds_hf.h, csrc/ds_obdm.h) and `estimator.OneBodyDensityMatrix`.

The orbitals at arbitrary points are held to the host restatement at ATOL = 1e-10, the bound of test_gpu_hf.py, and to the bits of
`ds_hf_orbitals` at the electrons.  The fold is compared with the numpy model of tests/obdm_helpers.py ON THE DEVICE'S OWN basis
values (read back from `orbitals_at`), which isolates the accumulation kernel; the bound per entry is 16 P 2^-53 sum |term| over
the P samples of the call: the standard bound of a sum in any order, no measurement enters it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hf_helpers as hh
import obdm_helpers as ob
from deepsolid_amd import device, systems

pytestmark = pytest.mark.gpu
ATOL = 1e-10
G = device.OBDM_GROUP
NELEC = (2, 1)                 # the electrons of the fold tests: N = 3
N_EL = 3


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device='cuda')


def ri(t):
    return torch.view_as_real(t)


def cplx(t):
    a = t.detach().cpu().numpy()
    return a[..., 0] + 1j * a[..., 1]


@functools.lru_cache(maxsize=None)
def tables(kind):
    """-> (System, GaussianOrbitals, HfOrbitalTables) of 'lih' or a hex orbital count."""
    s = hh.lih_system() if kind == 'lih' else ob.hex_basis(kind)
    go = s.gaussian_orbitals()
    return s, go, go._device_tables(torch.device('cuda', torch.cuda.current_device()))


# ------------------------------------------------------------------------------------------------ 1. orbitals at points
@pytest.mark.parametrize('kind', ['lih', (5, 4), (3, 0)])
@pytest.mark.parametrize('P', [1, 67])
def test_orbitals_at_against_the_host(kind, P):
    s, go, tab = tables(kind)
    rng = np.random.default_rng(100 + P)
    pts = (rng.uniform(size=(P, 3)) + rng.integers(-2, 3, size=(P, 3))) @ s.a
    ao = go.eval_aos_host(pts)
    for sp in range(2):
        got = go.eval_orbitals_at(dev(pts), sp)
        assert got.is_cuda and got.dtype == torch.complex128 and tuple(got.shape) == (P, s.nelec[sp])
        if s.nelec[sp] == 0:
            continue
        want = np.concatenate([ao[k] @ c for k, c in enumerate(go.mo_coeff[sp])], axis=-1)
        worst = float(np.abs(got.cpu().numpy() - want).max())
        print(f'{kind} P = {P} spin {sp}: max deviation {worst:.3e}')
        assert (P == 1 or np.abs(want).max() > 0.1) and worst <= ATOL      # (one point may lie in the vacuum of the hex cell)
        p32 = dev(pts, torch.float32)
        assert torch.equal(ri(tab.orbitals_at(p32, sp)), ri(tab.orbitals_at(p32.to(torch.float64), sp)))


@pytest.mark.parametrize('kind', ['lih', (5, 4), (3, 0)])
def test_orbitals_at_the_electrons_have_the_bits_of_the_orbital_matrices(kind):
    s, go, tab = tables(kind)
    B, N = 5, sum(s.nelec)
    x = dev(hh.walkers(s, B, seed=12, spread=2))
    mats = tab.orbitals(x)
    i0 = 0
    for sp in range(2):
        ne = s.nelec[sp]
        rows = tab.orbitals_at(x.reshape(B, N, 3)[:, i0:i0 + ne].reshape(-1, 3).contiguous(), sp)
        assert tuple(rows.shape) == (B * ne, ne)
        if ne:
            assert torch.equal(ri(rows), ri(mats[sp].reshape(B * ne, ne)))
        i0 += ne


# ------------------------------------------------------------------------------------------------ 2. the fold
def fold_case(kind, B, M, first, seed, dtype=np.float64):
    """Random walkers, O(1) complex ratios, shifts and weights for N = 3 electrons, and the device's own basis values at r_e
    and r' per sample (zero beyond M_spin)."""
    s, go, tab = tables(kind)
    rng = np.random.default_rng(seed)
    x = ((rng.uniform(size=(B, N_EL, 3)) + rng.integers(-1, 2, size=(B, N_EL, 3))) @ s.a).astype(dtype)
    sh = ((rng.uniform(size=(B, M, 3)) * 2 - 1) @ s.a).astype(dtype)
    q = (rng.normal(size=(B, M)) + 1j * rng.normal(size=(B, M)))
    wt = rng.uniform(0.5, 1.5, size=(B, M))
    w_idx, e_idx = ob.sample_electrons(B, M, N_EL, first)
    spin = (e_idx >= NELEC[0]).astype(int)
    r_old = x[w_idx, e_idx].astype(np.float64)
    r_new = (x[w_idx, e_idx].astype(np.float64) + sh.reshape(-1, 3).astype(np.float64)).astype(dtype).astype(np.float64)
    mb = max(s.nelec)
    phi_old = np.zeros((B * M, mb), dtype=np.complex128)
    phi_new = np.zeros((B * M, mb), dtype=np.complex128)
    for sp in range(2):
        if s.nelec[sp] and (spin == sp).any():
            k = spin == sp
            phi_old[k, :s.nelec[sp]] = tab.orbitals_at(dev(r_old[k]), sp).cpu().numpy()
            phi_new[k, :s.nelec[sp]] = tab.orbitals_at(dev(r_new[k]), sp).cpu().numpy()
    return dict(s=s, tab=tab, x=x.reshape(B, 3 * N_EL), sh=sh, q=q, wt=wt, spin=spin, phi_old=phi_old, phi_new=phi_new, mb=mb)


def run_fold(c, M, first, q=None, wt=None, tdtype=torch.float64, **kw):
    q = c['q'] if q is None else q
    qt = dev(np.stack([q.real, q.imag], axis=-1), tdtype)
    return c['tab'].obdm_accumulate(dev(c['x'], tdtype), NELEC, M, first, qt, dev(c['sh'], tdtype),
                                    weights=None if wt is None else dev(wt), **kw)


def assert_fold(out, c, q, wt, spin, what=''):
    P = q.size
    w = None if wt is None else wt.reshape(-1)
    ref = ob.fold(q.reshape(-1), w, c['phi_new'], c['phi_old'], spin)
    mag = ob.fold(q.reshape(-1), w, c['phi_new'], c['phi_old'], spin, absolute=True)
    for name, r, m in zip(('dm_sums', 'ov_sums'), ref, mag):
        got = cplx(out[name])
        err = np.abs(got - r)
        lim = ob.bound(P, m)
        worst = float((err / np.maximum(lim, 1e-300)).max())
        print(f'{what} {name}: P = {P}, largest |error| / bound = {worst:.3e}, largest |sum| = {np.abs(r).max():.3e}')
        assert np.all(err <= lim), (name, worst)


SHAPES = [(1, 1, 2), (G - 1, 1, 2), (G, 1, 2), ((G + 1) // 3, 3, 0), ((2 * G + 3) // 7, 7, 2)]      # (B, n_samples, first_electron)


@pytest.mark.parametrize('kind', [(5, 4), (17, 4), (64, 1)])
@pytest.mark.parametrize('B,M,first', SHAPES)
def test_fold_against_the_numpy_model(kind, B, M, first):
    assert B * M in (1, G - 1, G, G + 1, 2 * G + 3)
    c = fold_case(kind, B, M, first, seed=B * M + kind[0])
    for wt in (None, c['wt']):
        out = run_fold(c, M, first, wt=wt)
        assert out['n_bad'].tolist() == [0, 0]
        assert_fold(out, c, c['q'], wt, c['spin'], what=f'{kind} B = {B} M = {M} weights = {wt is not None}:')
    # rows and columns beyond M_spin are not touched
    mb, norb = c['mb'], c['s'].nelec
    keep = torch.full((2, mb, mb, 2), 0.5, dtype=torch.float64, device='cuda')
    for sp in range(2):
        keep[sp, :norb[sp], :norb[sp]] = 0.0
    dm, ov = keep.clone(), keep.clone()
    run_fold(c, M, first, dm_sums=dm, ov_sums=ov)
    for t in (dm, ov):
        for sp in range(2):
            outside = torch.ones(mb, mb, dtype=torch.bool, device='cuda')
            outside[:norb[sp], :norb[sp]] = False
            assert torch.all(t[sp][outside] == 0.5)


# ------------------------------------------------------------------------------------------------ 3. bit identity, bad samples
def test_any_workspace_gives_the_same_bits_and_a_second_call_doubles():
    B, M, first = (2 * G + 3) // 7, 7, 2
    c = fold_case((17, 4), B, M, first, seed=77)
    tab = c['tab']
    size = lambda n: int(tab.lib.ds_obdm_workspace_bytes(tab.handle, n, 1))
    one, two, full = size(1), size(G + 1), int(tab.lib.ds_obdm_workspace_bytes(tab.handle, B, M))
    assert one < two < full
    big = run_fold(c, M, first, wt=c['wt'])
    for cap in (one, two, two + 8):
        small = run_fold(c, M, first, wt=c['wt'], max_bytes=cap)
        assert torch.equal(small['dm_sums'], big['dm_sums']) and torch.equal(small['ov_sums'], big['ov_sums'])
    again = run_fold(c, M, first, wt=c['wt'])
    assert torch.equal(again['dm_sums'], big['dm_sums']) and torch.equal(again['ov_sums'], big['ov_sums'])
    with pytest.raises(RuntimeError, match='workspace too small'):
        run_fold(c, M, first, max_bytes=one - 8)
    dm, ov = big['dm_sums'].clone(), big['ov_sums'].clone()
    run_fold(c, M, first, wt=c['wt'], dm_sums=dm, ov_sums=ov)
    assert torch.equal(dm, 2 * big['dm_sums']) and torch.equal(ov, 2 * big['ov_sums'])


def test_bad_samples_are_left_out_and_counted_per_spin():
    B, M, first = (2 * G + 3) // 7, 7, 2
    c = fold_case((5, 4), B, M, first, seed=78)
    q, wt, spin = c['q'].copy().reshape(-1), c['wt'].copy().reshape(-1), c['spin'].copy()
    up, dn = np.flatnonzero(spin == 0), np.flatnonzero(spin == 1)
    q[up[3]] = np.nan
    q[up[G // 2]] = complex(1.0, np.inf)
    wt[up[-1]] = np.nan
    q[dn[0]] = complex(-np.inf, 0.0)
    wt[dn[-2]] = np.nan
    bad = [up[3], up[G // 2], up[-1], dn[0], dn[-2]]
    out = run_fold(c, M, first, q=q.reshape(B, M), wt=wt.reshape(B, M))
    assert out['n_bad'].tolist() == [3, 2]
    assert torch.isfinite(out['dm_sums']).all() and torch.isfinite(out['ov_sums']).all()
    left = spin.copy()
    left[bad] = -1
    qz, wz = q.copy(), wt.copy()
    qz[bad], wz[bad] = 0.0, 0.0
    assert_fold(out, c, qz, wz, left, what='bad samples:')


# ------------------------------------------------------------------------------------------------ 4. determinant identity
def test_determinant_identity_on_the_device():
    """psi = det of the LiH-like orbitals, the same orbitals as the basis, a common r' per (walker, spin), M = N, first = 0:
    sum_e q_e phi_k(r_e) = phi_k(r'), so dm_sums[s] N_s == ov_sums[s]."""
    s, go, tab = tables('lih')
    cell = hh.lih_cell()
    B, N, nelec = 6, 8, (4, 4)
    x = hh.walkers(s, B, seed=21, spread=1, sim_a=cell.a).reshape(B, N, 3)
    rng = np.random.default_rng(22)
    pts = (rng.uniform(size=(B, 2, 3)) + rng.integers(-1, 2, size=(B, 2, 3))) @ np.asarray(cell.a)
    shifts = ob.common_point_shifts(x, nelec, pts)
    mats = [m.cpu().numpy() for m in tab.orbitals(dev(x.reshape(B, 3 * N)))]
    moved = x + shifts                                          # what the kernel evaluates the basis at
    q = np.empty((B, N), dtype=np.complex128)
    for sp in range(2):
        el = slice(4 * sp, 4 * sp + 4)
        at_new = tab.orbitals_at(dev(moved[:, 4 * sp]), sp).cpu().numpy()
        for w in range(B):
            q[w, el] = ob.det_ratios(mats[sp][w], at_new[w])
    out = tab.obdm_accumulate(dev(x.reshape(B, 3 * N)), nelec, N, 0, dev(np.stack([q.real, q.imag], -1)), dev(shifts))
    dm, ov = cplx(out['dm_sums']), cplx(out['ov_sums'])
    for sp in range(2):
        dev_rel = np.abs(dm[sp] * nelec[sp] - ov[sp]).max() / np.abs(ov[sp]).max()
        print(f'spin {sp}: |N dm - ov| / max |ov| = {dev_rel:.3e}')
        assert dev_rel <= 1e-10


# ------------------------------------------------------------------------------------------------ 5. the estimator end to end
@functools.lru_cache(maxsize=None)
def lih_network(dtype):
    from deepsolid_amd import network as dnet
    cell = hh.lih_cell()
    go = tables('lih')[1]
    make = lambda m: dnet.make_solid_fermi_net(klist=go.klist, simulation_cell=cell, method_name=m, dtype=dtype,
                                               **systems.DETNET_DEFAULTS)
    slog, logdet = make('eval_slogdet'), make('eval_logdet')
    params = {k: [{kk: vv.to(device='cuda', dtype=dtype) for kk, vv in d.items()} for d in v] for k, v in logdet.init(0).items()}
    return cell, go, slog, logdet, params


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_estimator_updates_equal_the_fold_of_the_exported_ratios(dtype):
    from deepsolid_amd import estimator
    cell, go, _, logdet, params = lih_network(dtype)
    s, _, tab = tables('lih')
    npd = np.float64 if dtype == torch.float64 else np.float32
    B, N, M, seed = 7, 8, 3, 11
    xs = [dev(hh.walkers(s, B, seed=31 + u, sim_a=cell.a), dtype) for u in range(2)]
    acc = estimator.OneBodyDensityMatrix(logdet, params, go, samples_per_walker=M, seed=seed)
    for x in xs:
        acc.update(x)
    assert acc.offset == 2 and acc.first_electron == 6 and acc.samples.tolist() == [B * 4, B * 2]
    assert acc.n_bad.tolist() == [0, 0]
    qs, spins, olds, news = [], [], [], []
    for u, x in enumerate(xs):
        first = (u * M) % N
        out = logdet.apply.system.one_body_ratios(params, x, M, first_electron=first, seed=acc.seed, offset=u, want_ratios=True,
                                                  want_shifts=True)
        q = out['ratios'].cpu().numpy().astype(np.complex128).reshape(-1)
        sh = out['shifts'].cpu().numpy()
        assert sh.dtype == npd
        w_idx, e_idx = ob.sample_electrons(B, M, N, first)
        spin = (e_idx >= 4).astype(int)
        xe = x.cpu().numpy().reshape(B, N, 3)[w_idx, e_idx]
        r_old = xe.astype(np.float64)
        r_new = (xe.astype(np.float64) + sh.reshape(-1, 3).astype(np.float64)).astype(npd).astype(np.float64)   # formed in the walkers' type
        po, pn = np.zeros((B * M, 4), np.complex128), np.zeros((B * M, 4), np.complex128)
        for sp in range(2):
            k = spin == sp
            if k.any():
                po[k] = tab.orbitals_at(dev(r_old[k]), sp).cpu().numpy()
                pn[k] = tab.orbitals_at(dev(r_new[k]), sp).cpu().numpy()
        qs.append(q); spins.append(spin); olds.append(po); news.append(pn)
    c = dict(phi_old=np.concatenate(olds), phi_new=np.concatenate(news))
    out = dict(dm_sums=acc.dm_sums, ov_sums=acc.ov_sums)
    assert_fold(out, c, np.concatenate(qs), None, np.concatenate(spins), what=f'estimator {dtype}:')
    n, ov = acc.density_matrix(), acc.overlap()
    assert all(np.isfinite(m).all() and m.shape == (4, 4) for m in n + ov)


# ------------------------------------------------------------------------------------------------ 6. inside run_inference
def test_run_inference_with_the_density_matrix(tmp_path):
    from deepsolid_amd import estimator, inference
    cell, go, slog, logdet, params = lih_network(torch.float64)
    s = tables('lih')[0]
    x0 = dev(hh.walkers(s, 32, seed=51, sim_a=cell.a))
    acc = estimator.OneBodyDensityMatrix(logdet, params, go, seed=2)
    inference.run_inference(slog, logdet, params, x0, cell, iterations=3, key=1, burn_in=2, mcmc_steps=2, save_path=str(tmp_path),
                            accumulators=(acc,))
    assert acc.reduced and acc.offset == 3 and acc.first_electron == 0 and acc.samples.tolist() == [3 * 32 * 4, 3 * 32 * 4]
    back = estimator.OneBodyDensityMatrix.load(str(tmp_path / 'realspace.npz'))
    n, ov = back.density_matrix(), back.overlap()
    for sp in range(2):
        assert np.isfinite(n[sp]).all() and np.isfinite(ov[sp]).all()
        d, m = 0.5 * (n[sp] + n[sp].conj().T), 0.5 * (ov[sp] + ov[sp].conj().T)
        tr = float(np.trace(np.linalg.solve(m, d)).real)
        print(f'spin {sp}: Tr S^-1 n = {tr:.4f} with {back.samples[sp]} samples')
        assert tr <= 4 + 1


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_launch_nothing():
    B, M, first = 5, 3, 0
    c = fold_case((5, 4), B, M, first, seed=91)
    tab, lib = c['tab'], c['tab'].lib
    mb = c['mb']
    x, sh = dev(c['x']), dev(c['sh'])
    q = dev(np.stack([c['q'].real, c['q'].imag], -1))
    dm = torch.full((2, mb, mb, 2), 0.25, dtype=torch.float64, device='cuda')
    ov = torch.full((2, mb, mb, 2), -0.75, dtype=torch.float64, device='cuda')
    n_bad = torch.zeros(2, dtype=torch.int64, device='cuda')
    ws = torch.empty(int(lib.ds_obdm_workspace_bytes(tab.handle, B, M)) // 8, dtype=torch.float64, device='cuda')
    dm0, ov0 = dm.clone(), ov.clone()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def call(**kw):
        a = dict(h=tab.handle, dtype=0, x=x, B=B, N=N_EL, n_up=2, M=M, first=first, q=q, sh=sh, dm=dm, ov=ov, ws_bytes=ws.numel() * 8)
        a.update(kw)
        return lib.ds_obdm_accumulate(a['h'], a['dtype'], ptr(a['x']), a['B'], a['N'], a['n_up'], a['M'], a['first'], ptr(a['q']),
                                      ptr(a['sh']), ptr(None), ptr(a['dm']), ptr(a['ov']), ptr(n_bad), ptr(ws), a['ws_bytes'], None)

    bad = [dict(h=None), dict(x=None), dict(q=None), dict(sh=None), dict(dm=None, ov=None), dict(B=0), dict(M=0), dict(N=0),
           dict(n_up=-1), dict(n_up=4), dict(first=-1), dict(first=3), dict(dtype=2), dict(B=2 ** 31 // 3 + 1), dict(ws_bytes=64)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert lib.ds_last_error().decode(), kw
    torch.cuda.synchronize()
    assert torch.equal(dm, dm0) and torch.equal(ov, ov0) and n_bad.tolist() == [0, 0]
    assert call() == 0                                          # and the same arguments without a fault run
    assert call(dm=None) == 0 and call(ov=None) == 0            # either sum alone may be left out
    torch.cuda.synchronize()
    assert not torch.equal(dm, dm0) and not torch.equal(ov, ov0)
    # ds_hf_orbitals_at: refusals, and the calls that launch nothing
    out = torch.full((4, 5, 2), 3.0, dtype=torch.float64, device='cuda')
    pts = dev(np.zeros((4, 3)))
    at = lambda h, spin, dtype, p, n, o: lib.ds_hf_orbitals_at(h, spin, dtype, ptr(p), n, ptr(o), None)
    assert at(None, 0, 0, pts, 4, out) != 0 and at(tab.handle, 2, 0, pts, 4, out) != 0 and at(tab.handle, 0, 3, pts, 4, out) != 0
    assert at(tab.handle, 0, 0, None, 4, out) != 0 and at(tab.handle, 0, 0, pts, 4, None) != 0
    assert at(tab.handle, 0, 0, pts, 0, out) == 0
    empty = tables((3, 0))[2]
    assert at(empty.handle, 1, 0, pts, 4, out) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)
