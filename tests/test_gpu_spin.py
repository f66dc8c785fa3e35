"""GPU tests of `ds_spin_exchange_ratios` (csrc/ds_spin.h) and `estimator.SpinSquared`: the exchange ratios q = psi(P_p R) / psi(R)
against the float64 CPU oracle, the walker sums and the packed sums against numpy on the call's own ratios, chunked workspaces
(bit-identical), the involution q_p(R) q_p(P_p R) = 1, determinants of plane waves whose <S^2> is known exactly, float32, a walker
on a node, the normalisation of the accumulator on a real network, the accumulator inside `run_inference`, and the refusals of
the C ABI.

Float64 tolerance on q: TOL_Q max(1, |q_ref|) with TOL_Q = 2 (1e-9 + 1e-8), the bound test_gpu_onebody.py uses for the same
quantity (two log|psi| and two phases enter q)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import onebody_helpers as oh
import sampler_helpers as sh
import spin_helpers as sp

pytestmark = pytest.mark.gpu

TOL_Q = 2 * (1e-9 + 1e-8)
TOL_Q_F32 = 2 * (2e-3 + 5e-3)          # test_gpu_onebody.TOL_Q_F32: the float32 bounds of test_gpu_parity on 'lih'
EPS = 2.0 ** -52
FIXTURE_CASES = ['h2', 'lih', 'lih_twist', 'bcc_li', 'lih_fulldet', 'lih_bias']
CASES = FIXTURE_CASES + ['mirror_1_2']


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(vv, dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v] for k, v in params.items()}


def make_net(cell, klist, net_kw, dtype=torch.float64):
    from deepsolid_amd import network
    return network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', dtype=dtype, **net_kw)


def system(name, dtype=torch.float64):
    """-> (DeviceSystem of the case, device parameters, net)."""
    _, cell, kl, kw, p = sh.case(name)
    net = make_net(cell, kl, kw, dtype)
    return net.apply.system, dev_params(p, dtype), net


def cu(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device='cuda')


def complex_np(t):
    return t.cpu().numpy().astype(np.complex128)


def walker_bound(q):
    """Rounding bound of a sum of M numbers in any order: M 2^-52 sum |q_m| per walker."""
    return q.shape[1] * EPS * np.abs(q).sum(axis=1)


def check_sums(out, B):
    """`walker` against the numpy sum of the call's own float64 ratios and `sums` against `walker`, each within the rounding
    bound of its sum; the walkers with a non-finite ratio are left out, NaN, and counted.  -> mask of the good walkers."""
    q = complex_np(out['ratios'])
    t = complex_np(out['walker'])
    good = np.isfinite(q).all(axis=1)
    assert np.all(np.isnan(t[~good].real)) and np.all(np.isnan(t[~good].imag))
    assert np.all(np.abs(t[good] - q[good].sum(axis=1)) <= walker_bound(q[good]))
    sums = out['sums'].cpu().numpy()
    n = int(good.sum())
    tg = t[good]
    assert sums[3] == n and int(out['n_bad']) == B - n
    assert abs(sums[0] - tg.real.sum()) <= n * EPS * np.abs(tg.real).sum()
    assert abs(sums[1] - tg.imag.sum()) <= n * EPS * np.abs(tg.imag).sum()
    assert abs(sums[2] - (tg.real ** 2).sum()) <= (n + 1) * EPS * (tg.real ** 2).sum()      # (+1: each square is rounded too)
    return good


# ------------------------------------------------------------------------------------------------ 1. ratios vs oracle
@pytest.mark.parametrize('name', CASES)
def test_ratios_vs_oracle(name):
    """The case's walkers, M = P + 1 samples from first_pair = P - 1 (the pair index wraps): the ratios equal the oracle's within
    TOL_Q max(1, |q_ref|), nothing is counted as bad."""
    ref = sp.reference(name)
    nelec = ref['nelec']
    P = nelec[0] * nelec[1]
    M, first = P + 1, P - 1
    q_ref = ref['q_all'][:, sp.pair_indices(M, nelec, first)]
    mag = np.abs(q_ref)
    assert np.all(np.isfinite(q_ref))                                     # oracle side: every ratio of these inputs is finite
    if name in FIXTURE_CASES:                                             # ... with |q| in [0.016, 16.6], to the digits given
        assert 0.016 <= round(mag.min(), 3) and round(mag.max(), 1) <= 16.6, (mag.min(), mag.max())
    sysd, dp, _ = system(name)
    assert sysd.nelec == nelec
    out = sysd.spin_exchange_ratios(dp, cu(ref['x']), M, first_pair=first, want_ratios=True)
    q = complex_np(out['ratios'])
    assert q.shape == q_ref.shape
    err = np.abs(q - q_ref) / np.maximum(1.0, mag)
    print(f'{name}: max scaled |q - q_ref| = {err.max():.3e} (tolerance {TOL_Q:.1e}), |q| in [{mag.min():.3g}, {mag.max():.3g}]')
    assert err.max() <= TOL_Q
    assert out['n_bad'].tolist() == [0] and out['walker'] is None
    # the default is every pair once
    dflt = complex_np(sysd.spin_exchange_ratios(dp, cu(ref['x']), want_ratios=True)['ratios'])
    assert dflt.shape == (len(ref['x']), P) and np.all(np.abs(dflt - q_ref[:, 1:]) <= TOL_Q * np.maximum(1.0, mag[:, 1:]))


# ------------------------------------------------------------------------------------------------ 2. sums
@pytest.mark.parametrize('name,M', [('lih', 5), ('bcc_li', 145), ('bcc_li', 12), ('mirror_1_2', 3), ('h2', 130)])
def test_walker_sums_and_packed_sums(name, M):
    """t_w is the sum of the call's own ratios and `sums` follows from t_w, within the rounding of the sums (M = 145 and 130: more
    than one term per lane; 130 on one pair: all terms equal).  Entry 3 is B."""
    ref = sp.reference(name)
    sysd, dp, _ = system(name)
    B = len(ref['x'])
    P = ref['nelec'][0] * ref['nelec'][1]
    out = sysd.spin_exchange_ratios(dp, cu(ref['x']), M, first_pair=P - 1, want_ratios=True, want_walker=True)
    assert out['walker'].dtype == torch.complex128 and out['walker'].shape == (B,) and out['ratios'].shape == (B, M)
    good = check_sums(out, B)
    assert good.all() and float(out['sums'][3]) == B
    # sums alone (no ratios, no walker sums asked for) are the same bits
    alone = sysd.spin_exchange_ratios(dp, cu(ref['x']), M, first_pair=P - 1)
    assert torch.equal(alone['sums'], out['sums']) and alone['ratios'] is None and alone['walker'] is None


# ------------------------------------------------------------------------------------------------ 3. chunks
def one_group_bytes(sysd, dp, x, M):
    """Bytes of the smallest workspace the call accepts (one group of 80 configurations), read from its refusal of 1 byte."""
    with pytest.raises(RuntimeError, match='workspace too small') as e:
        sysd.spin_exchange_ratios(dp, x, M, max_bytes=1)
    return int(re.search(r'< (\d+) for one group', str(e.value)).group(1))


def test_one_group_workspace_gives_identical_bits():
    """bcc_li, M = 145 > 80: with a workspace of one group every chunk is 80 configurations, so one walker's samples straddle
    chunks.  sums, walker and ratios are bit-equal to the uncapped call and from run to run; a second call into the same sums
    doubles them exactly."""
    ref = sp.reference('bcc_li')
    sysd, dp, _ = system('bcc_li')
    x = cu(ref['x'])
    B, M = x.shape[0], 145
    kw = dict(first_pair=7, want_ratios=True, want_walker=True)
    full = int(sysd.lib.ds_spin_exchange_workspace_bytes(sysd.handle, B, M))
    one = one_group_bytes(sysd, dp, x, M)
    assert B * M > 2 * 80 and one < full
    big = sysd.spin_exchange_ratios(dp, x, M, **kw)
    small = sysd.spin_exchange_ratios(dp, x, M, max_bytes=one, **kw)
    again = sysd.spin_exchange_ratios(dp, x, M, max_bytes=one, **kw)
    for k in ('ratios', 'walker', 'sums', 'n_bad'):
        assert torch.equal(torch.view_as_real(small[k]) if small[k].is_complex() else small[k],
                           torch.view_as_real(big[k]) if big[k].is_complex() else big[k]), k
        assert torch.equal(torch.view_as_real(again[k]) if again[k].is_complex() else again[k],
                           torch.view_as_real(small[k]) if small[k].is_complex() else small[k]), k
    assert bool(big['sums'].abs().min() > 0)
    sums = big['sums'].clone()
    sysd.spin_exchange_ratios(dp, x, M, first_pair=7, sums=sums, max_bytes=one)
    assert torch.equal(sums, 2 * big['sums'])
    with pytest.raises(RuntimeError, match='workspace too small'):
        sysd.spin_exchange_ratios(dp, x, M, max_bytes=one - 1, **kw)


# ------------------------------------------------------------------------------------------------ 4. involution
@pytest.mark.parametrize('name,B', [('lih_twist', None), ('bcc_li', 2)])
def test_exchange_is_an_involution(name, B):
    """P_p P_p = 1, so q_p(R) q_p(P_p R) = 1: the exchanged configurations are given as walkers of a second call (independent
    of the oracle)."""
    ref = sp.reference(name)
    nelec = ref['nelec']
    P = nelec[0] * nelec[1]
    x = ref['x'][:B]
    B = len(x)
    sysd, dp, _ = system(name)
    q = complex_np(sysd.spin_exchange_ratios(dp, cu(x), want_ratios=True)['ratios'])
    xs = sp.swapped(x, nelec).reshape(B * P, -1)
    back = complex_np(sysd.spin_exchange_ratios(dp, cu(xs), want_ratios=True)['ratios']).reshape(B, P, P)
    qb = back[:, np.arange(P), np.arange(P)]                               # walker (w, p), pair p
    mag = np.abs(q)
    err = np.abs(q * qb - 1) / np.maximum(1.0, np.maximum(mag, 1 / mag))
    print(f'{name}: max scaled |q q_back - 1| = {err.max():.3e} (tolerance {2 * TOL_Q:.1e})')
    assert err.max() <= 2 * TOL_Q


# ------------------------------------------------------------------------------------------------ 5. plane waves
@pytest.mark.parametrize('which', ['lih', 'bcc_li', '2,1', '1,2'])
def test_shared_k_plane_waves_give_s_s_plus_1(which):
    """The determinant of plane waves with the same k points in both channels is an eigenstate of S^2 with s = |S_z|, walker by
    walker: t_w = min(n_up, n_dn) and `SpinSquared` returns s (s + 1), within the tolerance of the ratios added up."""
    from deepsolid_amd import estimator
    ref = sp.shared_reference(which)
    nu, nd = ref['nelec']
    P = nu * nd
    net = make_net(ref['cell'], ref['klist'], ref['net_kw'])
    dp = dev_params(ref['params'])
    x = cu(ref['x'])
    out = net.apply.system.spin_exchange_ratios(dp, x, want_ratios=True, want_walker=True)
    q, t = complex_np(out['ratios']), complex_np(out['walker'])
    assert np.all(np.isfinite(q))
    bound = TOL_Q * np.maximum(1.0, np.abs(q)).sum(axis=1)
    dev = np.abs(t - min(nu, nd))
    print(f'{which}: max |t_w - min(n_up, n_dn)| = {dev.max():.3e} (tolerance {bound.min():.3e})')
    assert np.all(dev <= bound)
    acc = estimator.SpinSquared(net, dp)
    acc.update(x)
    r = acc.spin_squared()
    s = 0.5 * abs(nu - nd)
    assert r['n_walkers'] == len(x) and r['n_bad'] == 0 and r['sz'] == 0.5 * (nu - nd)
    assert abs(r['value'] - s * (s + 1)) <= bound.sum() / len(x)           # n_good M / P = B
    # ... and with M = 1 pair per walker, scaled by P: the estimate of ONE pair is not s (s + 1), but P updates visit every pair
    one = estimator.SpinSquared(net, dp, pairs_per_walker=1)
    for _ in range(P):
        one.update(x)
    assert one.first_pair == 0
    r1 = one.spin_squared()
    assert r1['n_walkers'] == P * len(x)
    assert abs(r1['value'] - s * (s + 1)) <= bound.sum() / len(x)          # n_good M / P = (P B) / P


@pytest.mark.parametrize('name', ['lih_twist', 'bcc_li'])
def test_distinct_k_plane_wave_ratios_equal_the_closed_form(name):
    fx, cell, klist, _, _ = sh.case(name)
    pw_klist, net_kw, params, _, _ = oh.plane_wave_case(cell, klist)
    nelec = tuple(int(v) for v in cell.nelec)
    x = np.asarray(fx['x'], dtype=np.float64)
    want = sp.plane_wave_pair_ratios(x, pw_klist, nelec)
    net = make_net(cell, pw_klist, net_kw)
    q = complex_np(net.apply.system.spin_exchange_ratios(dev_params(params), cu(x), want_ratios=True)['ratios'])
    err = np.abs(q - want) / np.maximum(1.0, np.abs(want))
    print(f'{name}: max scaled |q - q_closed| = {err.max():.3e}, |q| up to {np.abs(want).max():.3g}')
    assert err.max() <= TOL_Q


# ------------------------------------------------------------------------------------------------ 6. float32
def test_ratios_float32_vs_float32_oracle():
    ref = sp.reference('lih', True)
    nelec = ref['nelec']
    P = nelec[0] * nelec[1]
    M, first = P + 1, P - 1
    q_ref = ref['q_all'][:, sp.pair_indices(M, nelec, first)]
    assert np.all(np.isfinite(q_ref))
    sysd, dp, _ = system('lih', torch.float32)
    out = sysd.spin_exchange_ratios(dp, cu(ref['x'], torch.float32), M, first_pair=first, want_ratios=True, want_walker=True)
    assert out['ratios'].dtype == torch.complex64 and out['walker'].dtype == torch.complex128 and out['sums'].dtype == torch.float64
    q = complex_np(out['ratios'])
    err = np.abs(q - q_ref) / np.maximum(1.0, np.abs(q_ref))
    print(f'lih float32: max scaled |q - q_ref| = {err.max():.3e} (tolerance {TOL_Q_F32:.1e})')
    assert err.max() <= TOL_Q_F32
    assert out['n_bad'].tolist() == [0]
    # the walker sums are formed from the float64 ratios: they equal the sum of the float32-rounded ones to float32 rounding
    t = complex_np(out['walker'])
    assert np.all(np.abs(t - q.sum(axis=1)) <= M * 2.0 ** -23 * np.abs(q).sum(axis=1))


# ------------------------------------------------------------------------------------------------ 7. a walker on a node
@pytest.mark.parametrize('kind', ['node', 'nan'])
def test_walker_without_finite_ratios_is_left_out_and_counted(kind):
    """lih, walker 0 spoilt.  'node': electron 1 placed exactly on electron 0 (same spin), psi(R) = 0.  The float64 oracle does not
    reach an exact zero there -- its two orbital rows differ in the last bits and |q| comes out near 1e15 -- so what is asserted on
    the oracle is that psi(R) vanishes to rounding (no finite ratio below 1e12); the library has to find NO finite ratio.
    'nan': one coordinate is NaN, which no evaluation can turn into a finite ratio."""
    ref = sp.reference('lih')
    nelec = ref['nelec']
    x = np.array(ref['x'])
    if kind == 'node':
        x[0, 3:6] = x[0, 0:3]
    else:
        x[0, 4] = np.nan
    q_ref = sp.oracle_ratios(sh.oracle('lih'), x, nelec, 4, 0)
    print(f'{kind}: oracle |q| of the spoilt walker = {np.abs(q_ref[0])}')
    assert np.all(~np.isfinite(q_ref[0]) | (np.abs(q_ref[0]) > 1e12)) and np.isfinite(q_ref[1:]).all()
    if kind == 'nan':
        assert not np.isfinite(q_ref[0]).any()
    sysd, dp, _ = system('lih')
    B = len(x)
    out = sysd.spin_exchange_ratios(dp, cu(x), 5, first_pair=2, want_ratios=True, want_walker=True)
    q = complex_np(out['ratios'])
    print(f'{kind}: library q of the spoilt walker = {q[0]}')
    bad = ~np.isfinite(q).all(axis=1)
    assert int(out['n_bad']) >= 1 and int(out['n_bad']) == int(bad.sum()) and bad[0]
    good = check_sums(out, B)
    assert np.array_equal(good, ~bad) and np.isnan(complex_np(out['walker'])[0])
    assert np.all(np.isfinite(out['sums'].cpu().numpy()))


# ------------------------------------------------------------------------------------------------ 8. normalisation
def test_spin_squared_on_a_real_network_vs_oracle():
    """bcc_li fixture network and walkers, M = 12 of the 144 pairs per update, two updates (pairs 0..11, then 12..23): the
    accumulator equals the formula of DESIGN.md section 17 evaluated from the oracle's ratios of the same pairs."""
    from deepsolid_amd import estimator
    ref = sp.reference('bcc_li')
    nelec = ref['nelec']
    B, M, P = len(ref['x']), 12, 144
    sysd, dp, net = system('bcc_li')
    acc = estimator.SpinSquared(net, dp, pairs_per_walker=M)
    x = cu(ref['x'])
    acc.update(x)
    assert acc.first_pair == 12
    acc.update(x)
    assert acc.first_pair == 24 and acc.n_walkers == 2 * B
    q = ref['q_all'][:, :24].reshape(B, 2, M)                              # [walker, update, sample]
    want = sp.spin_value(nelec, M, q.sum(axis=2).real.sum(), 2 * B)
    tol = (P / M) * TOL_Q * np.maximum(1.0, np.abs(q)).sum(axis=2).mean()
    r = acc.spin_squared()
    print(f'bcc_li: <S^2> = {r["value"]:.10f} +- {r["error"]:.3f}, oracle {want:.10f}, |diff| = {abs(r["value"] - want):.3e} (tolerance {tol:.3e})')
    assert abs(r['value'] - want) <= tol
    assert r['n_bad'] == 0 and r['n_walkers'] == 2 * B and r['sz'] == 0.0
    t = q.sum(axis=2).real.reshape(-1)
    assert r['error'] == pytest.approx((P / M) * np.sqrt(t.var() / (2 * B - 1)), rel=1e-6)
    assert abs(r['imag'] + (P / M) * q.sum(axis=2).imag.mean()) <= tol


# ------------------------------------------------------------------------------------------------ 9. run_inference
def test_run_inference_with_spin_squared(tmp_path):
    """B = 16, 3 iterations after a burn-in of 2: realspace.npz holds the fields, load round-trips, n_walkers = 3 x 16."""
    import realspace_helpers as rh
    from deepsolid_amd import estimator, inference
    cell, slog, ld, dp, x0 = rh.lih_drivers(16)
    acc = estimator.SpinSquared(ld, dp, pairs_per_walker=3)
    inference.run_inference(slog, ld, dp, x0.clone(), cell, save_path=str(tmp_path), accumulators=(acc,), iterations=3, key=17,
                            move_width=0.3, mcmc_steps=4, burn_in=2)
    assert acc.reduced and acc.n_walkers == 48 and acc.first_pair == (3 * 3) % 4
    r = acc.spin_squared()
    assert r['n_walkers'] == 48 and r['n_bad'] == 0 and np.isfinite(r['value']) and np.isfinite(r['error']) and r['error'] > 0
    path = str(tmp_path / 'realspace.npz')
    with np.load(path) as f:
        for k in ('sums', 'n_bad', 'n_walkers', 'nelec', 'pairs_per_walker', 'first_pair', 'value', 'error', 'imag'):
            assert k in f.files, k
        assert int(f['n_walkers']) == 48 and f['nelec'].tolist() == [2, 2] and float(f['sums'][3]) == 48
        assert float(f['value']) == r['value']
    loaded = estimator.SpinSquared.load(path)
    assert loaded.spin_squared() == r and loaded.first_pair == acc.first_pair and not loaded.reduced


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_launch_nothing():
    ref = sp.reference('lih')
    sysd, dp, _ = system('lih')
    lib, P = sysd.lib, 4
    x = cu(ref['x'])
    B, M = x.shape[0], 3
    p = sysd.pack_params(dp)
    sums = torch.zeros(4, dtype=torch.float64, device='cuda')
    ratio = torch.full((B, M, 2), 7.0, dtype=torch.float64, device='cuda')
    walker = torch.full((B, 2), 7.0, dtype=torch.float64, device='cuda')
    n_bad = torch.zeros(1, dtype=torch.int64, device='cuda')
    ws = sysd._workspace('ds_spin_exchange_workspace_bytes', B, M)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(sysd=sysd, p=p, x=x, B=B, M=M, first=0, sums=sums, ratio=ratio, walker=walker, ws_bytes=ws.numel())

    def call(**kw):
        a = {**good, **kw}
        return lib.ds_spin_exchange_ratios(a['sysd'].handle, ptr(a['p']), ptr(a['x']), a['B'], a['M'], a['first'], ptr(a['sums']),
                                           ptr(a['ratio']), ptr(a['walker']), ptr(n_bad), ptr(ws), a['ws_bytes'],
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    # li_polarized, nelec (3, 0): no pair of opposite spins
    pol, pol_dp, _ = system('li_polarized')
    pol_x = cu(sh.case('li_polarized')[0]['x'])
    assert pol.lib.ds_spin_exchange_workspace_bytes(pol.handle, 4, 1) > 0
    bad = [('B', dict(B=0)), ('n_pairs', dict(M=0)), ('first_pair', dict(first=P)), ('first_pair', dict(first=-1)),
           ('nothing to write', dict(sums=None, ratio=None, walker=None)), ('workspace too small', dict(ws_bytes=4096)),
           ('no pair of opposite spins', dict(sysd=pol, p=pol.pack_params(pol_dp), x=pol_x, B=pol_x.shape[0], M=1))]
    for word, kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
    with pytest.raises(RuntimeError, match='no pair of opposite spins'):
        pol.spin_exchange_ratios(pol_dp, pol_x)
    with pytest.raises(ValueError):
        sysd.spin_exchange_ratios(dp, x, M, sums=torch.zeros(3, dtype=torch.float64, device='cuda'))
    torch.cuda.synchronize()
    assert not sums.any() and bool((ratio == 7.0).all()) and bool((walker == 7.0).all()) and n_bad.tolist() == [0]
    assert call() == 0                                                     # the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert sums.any() and float(sums[3]) == B and not bool((ratio == 7.0).any()) and not bool((walker == 7.0).any())
