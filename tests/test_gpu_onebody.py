"""GPU tests of `ds_one_body_ratios` (csrc/ds_onebody.h) and `estimator.MomentumDistribution`: the ratios q = psi(R') / psi(R)
against the float64 CPU oracle with the shifts replayed in numpy, the momentum sums against the numpy fold of the oracle's
ratios, chunked workspaces, explicit shifts (the twisted-boundary property and a plane-wave determinant whose ratios and n(k)
are known in closed form), float32, the accumulator inside `run_inference`, and the refusals of the C ABI.

Float64 tolerance on q: 2 (1e-9 + 1e-8) max(1, |q_ref|) -- two log|psi| and two phases enter q, 1e-9 and 1e-8 are the bounds of
test_gpu_parity.test_logpsi_and_orbitals_vs_reference_vectors."""
import ctypes as C

import numpy as np
import pytest
import torch

import onebody_helpers as oh
import sampler_helpers as sh

pytestmark = pytest.mark.gpu

TOL_Q = 2 * (1e-9 + 1e-8)
# float32: the same construction from the bounds of test_gpu_parity.test_float32_chain_vs_float64_oracle on 'lih' (log|psi| 2e-3,
# phase 5e-3): 2 (2e-3 + 5e-3) = 1.4e-2, times max(1, |q_ref|)
TOL_Q_F32 = 2 * (2e-3 + 5e-3)
CASES = ['lih', 'lih_twist', 'bcc_li', 'lih_fulldet', 'lih_bias', 'li_polarized']
SEED, OFFSET = 20240607, 5


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(vv, dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v] for k, v in params.items()}


def system(name, dtype=torch.float64, klist=None, net_kw=None, params=None):
    """-> (DeviceSystem of the case, device parameters, cell)."""
    from deepsolid_amd import network
    _, cell, kl, kw, p = sh.case(name)
    net = network.make_solid_fermi_net(klist=klist if klist is not None else kl, simulation_cell=cell, method_name='eval_logdet',
                                       dtype=dtype, **(net_kw or kw))
    return net.apply.system, dev_params(params if params is not None else p, dtype), cell


def cu(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device='cuda')


def complex_np(t):
    return t.cpu().numpy().astype(np.complex128)


def kpoints(cell, klist, n_k):
    from deepsolid_amd import estimator
    return estimator.momentum_kpoints(cell, klist, {1: 0, 27: 1, 125: 2}[n_k])[0]


def philox_setup(name, f32=False):
    cell = sh.case(name)[1]
    N = sum(int(v) for v in cell.nelec)
    return oh.reference(name, SEED, OFFSET, N + 1, N - 1, f32), N + 1, N - 1


# ------------------------------------------------------------------------------------------------ 1. ratios, Philox mode
@pytest.mark.parametrize('name', CASES)
def test_ratios_and_shifts_vs_oracle(name):
    """Fixture walkers, M = N + 1 samples from first_electron = N - 1 (the electron index wraps): the shifts equal the numpy
    replay to 1 ulp, the ratios the oracle's within TOL_Q, nothing is counted as bad."""
    ref, M, first = philox_setup(name)
    assert np.all(np.isfinite(ref['q']))                                  # oracle side: every ratio of these inputs is finite
    sysd, dp, cell = system(name)
    out = sysd.one_body_ratios(dp, cu(ref['x']), M, first_electron=first, seed=SEED, offset=OFFSET, want_ratios=True, want_shifts=True)
    s = out['shifts'].cpu().numpy()
    assert s.shape == ref['s'].shape and np.all(np.abs(s - ref['s']) <= np.spacing(np.abs(ref['s'])))
    q = complex_np(out['ratios'])
    err = np.abs(q - ref['q']) / np.maximum(1.0, np.abs(ref['q']))
    print(f'{name}: max scaled |q - q_ref| = {err.max():.3e} (tolerance {TOL_Q:.1e}), |q| in [{np.abs(ref["q"]).min():.3g}, {np.abs(ref["q"]).max():.3g}]')
    assert err.max() <= TOL_Q
    assert out['n_bad'].tolist() == [0, 0] and out['nk_sums'] is None


# ------------------------------------------------------------------------------------------------ 2. sums
@pytest.mark.parametrize('n_k', [1, 27, 125])
@pytest.mark.parametrize('name', CASES)
def test_momentum_sums_vs_numpy_fold(name, n_k):
    """nk_sums equals the numpy fold of the oracle's q with the replayed s (TOL_Q max(1, |q|) per sample, so the bound of a sum is
    that of its samples added up); a second call adds -- the buffer doubles exactly --, two fresh runs are bit-identical, and
    the empty spin channel of li_polarized stays exactly zero."""
    ref, M, first = philox_setup(name)
    sysd, dp, cell = system(name)
    kv = kpoints(cell, sh.case(name)[2], n_k)
    assert kv.shape == (n_k, 3)
    x = cu(ref['x'])
    kw = dict(kvec=kv, first_electron=first, seed=SEED, offset=OFFSET)
    out = sysd.one_body_ratios(dp, x, M, **kw)
    sums = out['nk_sums']
    got = sums.cpu().numpy()
    want = oh.fold(ref['q'], ref['s'], kv, first, ref['nelec'])
    spin = (oh.electrons(M, sum(ref['nelec']), first) >= ref['nelec'][0]).astype(int)
    for sp in range(2):
        tol = TOL_Q * np.maximum(1.0, np.abs(ref['q'][:, spin == sp])).sum()
        err = np.abs(got[sp] - want[sp]).max()
        print(f'{name} n_k={n_k} spin {sp}: max |sum - fold| = {err:.3e} (tolerance {tol:.3e})')
        assert err <= tol, (sp, err, tol)
    if ref['nelec'][1] == 0:
        assert not got[1].any()
    assert out['n_bad'].tolist() == [0, 0]
    first_call = sums.clone()
    sysd.one_body_ratios(dp, x, M, nk_sums=sums, **kw)
    assert torch.equal(sums, 2 * first_call)
    again = sysd.one_body_ratios(dp, x, M, **kw)['nk_sums']
    assert torch.equal(again, first_call)


# ------------------------------------------------------------------------------------------------ 3. chunking
def test_small_workspace_runs_more_chunks_with_identical_results():
    """lih tiled to B = 37, M = 9: 333 configurations = 5 groups of 80 samples.  A workspace cut to two groups runs the chunks
    160 + 160 + 13.  The partial sums are formed over fixed groups of 80 consecutive samples and added in group order whatever
    the chunks are, so ratios AND sums are bit-identical to the one-chunk run."""
    fx, cell, klist, _, _ = sh.case('lih')
    sysd, dp, _ = system('lih')
    B, M = 37, 9
    x = cu(sh.tiled_walkers(cell, fx['x'], B))
    size = lambda m: int(sysd.lib.ds_one_body_workspace_bytes(sysd.handle, B, m))
    one, two, full = size(1), size(4), size(M)                           # 37, 148, 333 configurations: 1, 2, 5 groups
    per = two - one
    assert 3.5 * per < full - one < 4.5 * per, (one, two, full)
    kv = kpoints(cell, klist, 27)
    kw = dict(kvec=kv, first_electron=2, seed=SEED, offset=1, want_ratios=True)
    big = sysd.one_body_ratios(dp, x, M, **kw)
    small = sysd.one_body_ratios(dp, x, M, max_bytes=two, **kw)
    assert torch.equal(small['ratios'], big['ratios'])
    assert torch.equal(small['nk_sums'], big['nk_sums'])
    assert bool(big['nk_sums'].abs().sum() > 0)
    with pytest.raises(RuntimeError, match='workspace too small'):
        sysd.one_body_ratios(dp, x, M, max_bytes=one // 2, **kw)


def test_more_configurations_than_one_chunk_may_hold():
    """B = 700, M = 96: 67 200 configurations, over the 65535 of one chunk.  Zero shifts give q = 1 for every sample."""
    fx, cell, klist, _, _ = sh.case('lih')
    sysd, dp, _ = system('lih')
    B, M = 700, 96
    x = cu(sh.tiled_walkers(cell, fx['x'], B))
    out = sysd.one_body_ratios(dp, x, M, shifts=torch.zeros(B, M, 3, dtype=torch.float64, device='cuda'), want_ratios=True,
                               kvec=kpoints(cell, klist, 1))
    q = out['ratios']
    assert q.shape == (B, M) and float((q - 1).abs().max()) <= 1e-12
    # exp(-i k.0) = 1: each spin's sum is its number of samples
    np.testing.assert_allclose(out['nk_sums'].cpu().numpy()[:, 0, 0], oh.samples_per_spin(B, M, 0, (2, 2)), rtol=1e-12)
    assert out['n_bad'].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 4. explicit shifts
def test_lattice_vector_shift_gives_the_twist_phase():
    """Moving an electron by a supercell lattice vector L multiplies psi by exp(i k_t . L): the twisted boundary condition."""
    fx, cell, klist, _, _ = sh.case('lih_twist')
    sysd, dp, _ = system('lih_twist')
    a = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    x = np.asarray(fx['x'], dtype=np.float64)
    B, M = len(x), 6
    n = np.asarray([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 2, 0], [1, -1, 1], [-2, 0, 3]])
    s = np.broadcast_to((n @ a)[None], (B, M, 3)).copy()
    kt = np.asarray(klist[0], dtype=np.float64).reshape(-1, 3)[0]
    want = np.broadcast_to(np.exp(1j * (n @ a) @ kt)[None], (B, M))
    assert np.abs(want - 1).min() > 1e-2                                   # every sample has a phase to get right
    q = complex_np(sysd.one_body_ratios(dp, cu(x), M, first_electron=1, shifts=cu(s), want_ratios=True)['ratios'])
    assert np.abs(q - want).max() <= TOL_Q


# ------------------------------------------------------------------------------------------------ 5. known answer
def test_plane_wave_determinant_ratios_and_occupations():
    """The plane-wave network of onebody_helpers on LiH with a twist, B = 2, independent of the oracle: q from positions alone,
    and with one full 3 x 3 x 3 grid of shifts per electron the per-walker estimate is 1 on the occupied k and 0 on the other k
    of the 27 (TOL_Q per sample, times 27 samples per grid sum)."""
    fx, cell, klist, _, _ = sh.case('lih_twist')
    pw_klist, net_kw, params, kpts, occ = oh.plane_wave_case(cell, klist)
    sysd, dp, _ = system('lih_twist', klist=pw_klist, net_kw=net_kw, params=params)
    nelec = (2, 2)
    B, N = 2, 4
    x = np.asarray(fx['x'][:B], dtype=np.float64)
    s = oh.grid_shifts(cell.a, B, N)
    M = s.shape[1]
    want = oh.plane_wave_ratios(x, s, 0, pw_klist, nelec)
    out = sysd.one_body_ratios(dp, cu(x), M, kvec=kpts, shifts=cu(s), want_ratios=True)
    q = complex_np(out['ratios'])
    err = np.abs(q - want) / np.maximum(1.0, np.abs(want))
    print(f'plane waves: max scaled |q - q_closed| = {err.max():.3e}, |q| up to {np.abs(want).max():.3g}')
    assert err.max() <= TOL_Q
    sums = out['nk_sums'].cpu().numpy()
    est = (sums[..., 0] + 1j * sums[..., 1]) / (27 * B)                    # mean over walkers of the per-walker estimate
    exact = np.zeros((2, 27))
    exact[0, occ[0]] = 1
    exact[1, occ[1]] = 1
    # a grid sum holds 27 N_s samples per walker and is divided by 27: N_s = 2 sample bounds at most, inside 27 of them
    bound = 27 * TOL_Q * max(1.0, np.abs(want).max())
    print(f'plane waves: max |n(k) - occupation| = {np.abs(est - exact).max():.3e} (tolerance {bound:.3e})')
    assert np.abs(est - exact).max() <= bound


# ------------------------------------------------------------------------------------------------ 6. float32
def test_ratios_float32_vs_float32_oracle():
    ref, M, first = philox_setup('lih', f32=True)
    assert np.all(np.isfinite(ref['q']))
    sysd, dp, _ = system('lih', torch.float32)
    out = sysd.one_body_ratios(dp, cu(ref['x'], torch.float32), M, first_electron=first, seed=SEED, offset=OFFSET, want_ratios=True,
                               want_shifts=True)
    s32 = ref['s'].astype(np.float32)
    s = out['shifts'].cpu().numpy()
    assert s.dtype == np.float32 and np.all(np.abs(s - s32) <= np.spacing(np.abs(s32)))
    assert out['ratios'].dtype == torch.complex64
    q = complex_np(out['ratios'])
    err = np.abs(q - ref['q']) / np.maximum(1.0, np.abs(ref['q']))
    print(f'lih float32: max scaled |q - q_ref| = {err.max():.3e} (tolerance {TOL_Q_F32:.1e})')
    assert err.max() <= TOL_Q_F32
    assert out['n_bad'].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 7. accumulator end to end
def test_run_inference_with_momentum_distribution(tmp_path):
    """B = 64, 3 iterations after a burn-in of 2: realspace.npz holds the fields, the samples are 3 x 64 x M split by spin, and
    the same seed twice gives bit-identical sums."""
    import realspace_helpers as rh
    from deepsolid_amd import estimator, inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(64)
    kw = dict(iterations=3, key=17, move_width=0.3, mcmc_steps=4, burn_in=2)
    files = []
    for run in ('a', 'b'):
        acc = estimator.MomentumDistribution(ld, dp, seed=11)
        assert acc.samples_per_walker == 4 and len(acc.kpoints) == 27
        inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(tmp_path / run), accumulators=(acc,), **kw)
        assert acc.reduced and acc.offset == 3 and acc.first_electron == 0
        with np.load(str(tmp_path / run / 'realspace.npz')) as f:
            files.append({k: f[k] for k in f.files})
    a, b = files
    for k in ('sums', 'samples', 'n_bad', 'kpoints', 'k_int', 'nelec', 'n_k'):
        assert k in a, k
    assert a['samples'].tolist() == [3 * 64 * 2, 3 * 64 * 2] and a['n_bad'].tolist() == [0, 0] and a['nelec'].tolist() == [2, 2]
    assert a['sums'].shape == (2, 27, 2) and a['n_k'].shape == (2, 27) and np.all(np.isfinite(a['sums'])) and a['sums'].any()
    np.testing.assert_array_equal(a['n_k'], 2 * (a['sums'][..., 0] + 1j * a['sums'][..., 1]) / 384)
    np.testing.assert_array_equal(a['sums'], b['sums'])
    other = estimator.MomentumDistribution(ld, dp, seed=12)
    other.update(x0)
    mine = estimator.MomentumDistribution(ld, dp, seed=11)
    mine.update(x0)
    assert not torch.equal(mine.sums, other.sums)                          # the seed reaches the kernel


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing():
    fx, cell, klist, _, _ = sh.case('lih')
    sysd, dp, _ = system('lih')
    lib, N = sysd.lib, 4
    x = cu(fx['x'])
    B, M, n_k = x.shape[0], 3, 27
    p = sysd.pack_params(dp)
    kv = cu(kpoints(cell, klist, n_k))
    sums = torch.zeros(2, n_k, 2, dtype=torch.float64, device='cuda')
    ratio = torch.full((B, M, 2), 7.0, dtype=torch.float64, device='cuda')
    n_bad = torch.zeros(2, dtype=torch.int64, device='cuda')
    ws = sysd._workspace('ds_one_body_workspace_bytes', B, M)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(B=B, M=M, first=0, kvec=kv, n_k=n_k, sums=sums, ratio=ratio)

    def call(**kw):
        a = {**good, **kw}
        return lib.ds_one_body_ratios(sysd.handle, ptr(p), ptr(x), a['B'], a['M'], a['first'], 1, 0, ptr(None), ptr(a['kvec']), a['n_k'],
                                      ptr(a['sums']), ptr(a['ratio']), ptr(None), ptr(n_bad), ptr(ws), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [('B', dict(B=0)), ('n_samples', dict(M=0)), ('first_electron', dict(first=N)), ('first_electron', dict(first=-1)),
           ('n_k', dict(n_k=513)), ('n_k', dict(n_k=-1)), ('kvec', dict(kvec=None)), ('nk_sums', dict(sums=None)),
           ('nothing to write', dict(n_k=0, kvec=None, sums=None, ratio=None))]
    for word, kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert not sums.any() and bool((ratio == 7.0).all()) and n_bad.tolist() == [0, 0]
    assert call() == 0                                                     # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert sums.any() and not bool((ratio == 7.0).any())
