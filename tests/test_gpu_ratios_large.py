"""GPU tests of the three ratio passes -- `ds_one_body_ratios` (csrc/ds_onebody.h), `ds_spin_exchange_ratios` (csrc/ds_spin.h) and
`ds_ecp_energy` (csrc/ds_ecp.h) -- where test_gpu_onebody.py, test_gpu_spin.py and test_gpu_ecp.py do not go:

A. the large cells (48 to 108 electrons: the value chain's wide-slot, blocked-trace and one-lane-per-row instances; bcc_li_333 with
   41 + 40 electrons, where confusing n_up with n_dn changes a pair), two fixture walkers each, against the float64 CPU oracle, and
   diamond in float32 against the float32 oracle;
B. full batches of DISTINCT lih walkers (sampler_helpers.distinct_walkers: a result read from the wrong walker differs): more than
   65 520 configurations in one call, walkers beyond 1024 in k_ecp_offsets (three per thread) and beyond 256 in k_spin_final, the
   forward of the undisplaced walkers in several passes of a capped workspace, and n_k at its cap of 512.

Tolerances are those of the small-cell tests: TOL_Q = 2 (1e-9 + 1e-8) max(1, |q_ref|) per float64 ratio (two log|psi| and two phases
enter q; 1e-9 and 1e-8 are the bounds of test_gpu_parity.test_logpsi_and_orbitals_vs_reference_vectors, which includes diamond,
bcc_li_333 and graphene_331), TOL_Q_F32 = 2 (2e-3 + 5e-3) in float32 (test_float32_chain_vs_float64_oracle, which includes
diamond); a sum gets the sum of its samples' bounds.  test_ratios_large_cpu.py shows on the oracle alone that moving the inputs by
a few ulp moves q by at most 4.9e-4 TOL_Q.  A sum of the call's own exported terms is held to the bound of tests/obdm_helpers.py,
16 P 2^-53 sum |term| for P terms in any order."""
import re

import numpy as np
import pytest
import torch

import ecp_helpers as eh
import obdm_helpers as ob
import onebody_helpers as oh
import ratios_large_helpers as rl
import sampler_helpers as sh
import spin_helpers as sp
from ratios_large_helpers import TOL_Q, TOL_Q_F32
from test_gpu_ecp import check_against_reference, e_loc_bound, ptr, raw_call, stream
from test_gpu_onebody import complex_np, cu, kpoints, system
from test_gpu_spin import check_sums

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)


def one_group_bytes(call):
    """Bytes of the smallest workspace `call(max_bytes=...)` accepts (one group of 80 configurations), read from its refusal."""
    with pytest.raises(RuntimeError, match='workspace too small') as e:
        call(max_bytes=1)
    return int(re.search(r'< (\d+) for one group', str(e.value)).group(1))


def capped_bytes(one, full, full_groups, groups):
    """A workspace with room for `groups` groups of 80 configurations and not for one more, from the bytes of one group and of the
    `full_groups` the uncapped call gets (the layout is linear in the groups up to two alignment pads of under 1 KiB)."""
    per = (full - one) / (full_groups - 1)
    assert full_groups > groups and per > 4096, (one, full, full_groups)
    cap = one + int((groups - 1) * per) + int(per / 2)
    assert one + (groups - 1) * per + 1024 < cap < one + groups * per - 1024
    return cap


def room_for(one, full, full_groups, groups):
    """A workspace with room for at least `groups` groups (same inputs as `capped_bytes`)."""
    per = (full - one) / (full_groups - 1)
    return one + int(groups * per) + 4096


def fold_check(got, q, s, kv, first, nelec, what):
    """nk_sums against the numpy fold of the call's own exported q and s (samples with a non-finite q left out): per spin within
    16 P 2^-53 sum |q| (obdm_helpers.bound; |exp(-i k.s)| = 1).  -> largest error / bound."""
    good = np.isfinite(q)
    qz, sz = np.where(good, q, 0.0), np.where(good[..., None], s, 0.0)
    want = oh.fold(qz, sz, kv, first, nelec)
    spin = (oh.electrons(q.shape[1], sum(nelec), first) >= nelec[0]).astype(int)
    worst = 0.0
    for sn in range(2):
        k = good[:, spin == sn]
        lim = ob.bound(int(k.sum()), np.abs(qz[:, spin == sn]).sum())
        err = np.abs(got[sn] - want[sn]).max()
        worst = max(worst, err / lim)
        assert err <= lim, (what, sn, err, lim)
    print(f'{what}: largest |nk_sums - fold| / bound = {worst:.3e}')
    return worst


# =================================================================================================== A. large cells
# ------------------------------------------------------------------------------------------------ 1. one-body
@pytest.mark.parametrize('name', rl.ONEBODY_CELLS)
def test_onebody_large_cells_vs_oracle(name):
    """Two fixture walkers, M = N + 1 samples from first_electron = N - 1 in Philox mode (every electron once, the index wraps,
    2 (N + 1) <= 218 configurations: neither a multiple of 80 nor of 64): shifts equal the replay to 1 ulp, q the oracle's within
    TOL_Q, nothing is bad, the sums of 27 k points equal the fold of the oracle's q within the summed bound.
    Measured (ratio error / TOL_Q, |q| range, sum error / bound): graphene 1.1e-4, [1.4e-3, 1.4e3], 3.6e-5; diamond 7.0e-5,
    [0.028, 16.7], 3.4e-6; bcc_li_333 4.3e-5, [0.010, 29.4], 4.9e-6; graphene_331 4.9e-4, [3.1e-4, 1.0e3], 4.8e-5."""
    ref, M, first = rl.onebody_reference(name)
    nelec = ref['nelec']
    sysd, dp, cell = system(name)
    kv = kpoints(cell, sh.case(name)[2], 27)
    out = sysd.one_body_ratios(dp, cu(ref['x']), M, kvec=kv, first_electron=first, seed=rl.SEED, offset=rl.OFFSET, want_ratios=True,
                               want_shifts=True)
    s = out['shifts'].cpu().numpy()
    assert s.shape == ref['s'].shape and np.all(np.abs(s - ref['s']) <= np.spacing(np.abs(ref['s'])))
    q = complex_np(out['ratios'])
    err = rl.scaled(q, ref['q'])
    print(f'{name}: max scaled |q - q_ref| / TOL_Q = {err.max() / TOL_Q:.3e}, {rl.q_range(ref["q"])}')
    assert np.all(np.isfinite(ref['q'])) and err.max() <= TOL_Q
    assert out['n_bad'].tolist() == [0, 0]
    got = out['nk_sums'].cpu().numpy()
    want = oh.fold(ref['q'], ref['s'], kv, first, nelec)
    spin = (oh.electrons(M, sum(nelec), first) >= nelec[0]).astype(int)
    for sn in range(2):
        tol = TOL_Q * np.maximum(1.0, np.abs(ref['q'][:, spin == sn])).sum()
        e = np.abs(got[sn] - want[sn]).max()
        print(f'{name} spin {sn}: max |sum - fold| / bound = {e / tol:.3e}')
        assert e <= tol, (sn, e, tol)
    if name == 'bcc_li_333':
        # per walker electron 80 (down) twice, 0..40 (up) and 41..79 (down) once: 41 up against 40 + 1 down
        assert nelec == (41, 40) and oh.samples_per_spin(len(ref['x']), M, first, nelec).tolist() == [2 * 41, 2 * 41]
        assert int((spin == 0).sum()) == 41 and int((spin == 1).sum()) == 41


# ------------------------------------------------------------------------------------------------ 2. spin
@pytest.mark.parametrize('name', rl.SPIN_CELLS)
def test_spin_large_cells_vs_oracle(name):
    """diamond (48, 48) and bcc_li_333 (41, 40), M = 130 pairs from first_pair = P - 7 (the index wraps; more than two laps of the 64
    lanes of k_spin_walker; 260 configurations): q equals the oracle's on the pairs taken within TOL_Q, `walker` and `sums` follow
    from the call's own ratios within the rounding of their sums.
    Measured (ratio error / TOL_Q, |q| range): diamond 7.3e-5, [0.024, 7.0]; bcc_li_333 4.6e-5, [0.038, 24.3]."""
    ref, M, first = rl.spin_reference(name)
    nu, nd = ref['nelec']
    if name == 'bcc_li_333':
        p = sp.pair_indices(M, (nu, nd), first)
        assert np.any(np.stack([p // nu, nu + p % nu], axis=1) != sp.pairs((nu, nd))[p])      # i = p / n_up takes another pair
    sysd, dp, _ = system(name)
    assert sysd.nelec == (nu, nd)
    B = len(ref['x'])
    out = sysd.spin_exchange_ratios(dp, cu(ref['x']), M, first_pair=first, want_ratios=True, want_walker=True)
    q = complex_np(out['ratios'])
    assert q.shape == ref['q'].shape == (B, 130) and np.all(np.isfinite(ref['q']))
    err = rl.scaled(q, ref['q'])
    print(f'{name}: max scaled |q - q_ref| / TOL_Q = {err.max() / TOL_Q:.3e}, {rl.q_range(ref["q"])}')
    assert err.max() <= TOL_Q
    good = check_sums(out, B)
    assert good.all() and out['n_bad'].tolist() == [0] and float(out['sums'][3]) == B
    t = complex_np(out['walker'])
    assert np.all(np.abs(t - ref['q'].sum(axis=1)) <= TOL_Q * np.maximum(1.0, np.abs(ref['q'])).sum(axis=1))


# ------------------------------------------------------------------------------------------------ 3. pseudopotential
def run_ecp(name, n_quad=12, f32=False, mode='philox'):
    ref = rl.ecp_reference(name, n_quad, f32)
    dtype = torch.float32 if f32 else torch.float64
    sysd, dp, _ = system(name, dtype)
    rot = dict(rotations=cu(ref['rot'])) if mode == 'explicit' else dict(seed=eh.SEED, offset=eh.OFFSET)
    out = sysd.ecp_energy(dp, cu(ref['x'], dtype), ref['ecp'], want_pairs=True, want_ratios=True, want_rotations=True, **rot)
    return ref, out


@pytest.mark.parametrize('mode', ['philox', 'explicit'])
@pytest.mark.parametrize('name,n_quad', rl.ECP_RULES)
def test_ecp_large_cells_vs_oracle(name, n_quad, mode):
    """diamond ([17, 18] pairs, 420 configurations) and bcc_li_333 ([5, 9]; also with the 6-point rule), r_cut = 1.2 Bohr, Philox and
    explicit rotations: the pairs equal the table and the model, E_loc the model within its float64 bound, the ratios the oracle's
    within TOL_Q and E_nl within TOL_Q times the walker's scale.
    Measured (ratio error / TOL_Q, |q| range, E_nl error / bound, E_loc error / bound): diamond 1.5e-3, [0.023, 11.9], 2.5e-4,
    5.6e-3; bcc_li_333 4.0e-5, [0.025, 5.1], 3.6e-6, 5.2e-3; 6 points 2.7e-5, [0.15, 5.9], 4.4e-6, 5.2e-3."""
    ref, out = run_ecp(name, n_quad, mode=mode)
    counts = eh.LARGE_CASES[name][1]
    assert out['pairs'].tolist() == counts and np.array_equal(out['pairs'].cpu().numpy(), ref['pairs']['counts'])
    assert out['ratios'].shape == (sum(counts) * n_quad,) and out['ratios'].dtype == torch.complex128
    assert np.abs(out['rotations'].cpu().numpy() - ref['rot']).max() <= 1e-15
    err, bound = np.abs(out['e_loc'].cpu().numpy() - ref['e_loc']), e_loc_bound(ref)
    print(f'{name} N_q = {n_quad} {mode}: max |E_loc - model| / bound = {(err / bound).max():.3e}; '
          f'max scaled |q - q_ref| / TOL_Q = {rl.scaled(complex_np(out["ratios"]), ref["q"]).max() / TOL_Q:.3e}, {rl.q_range(ref["q"])}; '
          f'max |E_nl - model| / bound = {(np.abs(complex_np(out["e_nl"]) - ref["e_nl"]) / (TOL_Q * ref["e_nl_scale"])).max():.3e}')
    assert ref['e_loc_terms'].sum() > 0 and np.all(err <= bound)
    check_against_reference(ref, out, TOL_Q, n_quad)


# ------------------------------------------------------------------------------------------------ 4. float32
def test_onebody_float32_diamond_vs_float32_oracle():
    """M = 24 from first_electron = N - 12: twelve up and twelve down electrons.  Against the float32 oracle within TOL_Q_F32; the
    float32 oracle's own loss against the float64 oracle at the same rounded configurations is printed beside it.
    Measured: error 4.1e-4 of max(1, |q|) = 2.9e-2 TOL_Q_F32, float32 oracle loss 3.8e-4, |q| in [0.072, 12.6]."""
    ref, M, first = rl.onebody_reference('diamond', True)
    assert set(oh.electrons(M, 96, first) >= 48) == {False, True}
    sysd, dp, _ = system('diamond', torch.float32)
    out = sysd.one_body_ratios(dp, cu(ref['x'], torch.float32), M, first_electron=first, seed=rl.SEED, offset=rl.OFFSET, want_ratios=True,
                               want_shifts=True)
    s32 = ref['s'].astype(np.float32)
    s = out['shifts'].cpu().numpy()
    assert s.dtype == np.float32 and np.all(np.abs(s - s32) <= np.spacing(np.abs(s32)))
    assert out['ratios'].dtype == torch.complex64
    err = rl.scaled(complex_np(out['ratios']), ref['q'])
    print(f'diamond float32 one-body: max scaled |q - q_ref| = {err.max():.3e} = {err.max() / TOL_Q_F32:.3e} TOL_Q_F32, float32 oracle '
          f'loss {rl.onebody_f32_oracle_loss("diamond"):.3e}, {rl.q_range(ref["q"])}')
    assert np.all(np.isfinite(ref['q'])) and err.max() <= TOL_Q_F32
    assert out['n_bad'].tolist() == [0, 0]


def test_spin_float32_diamond_vs_float32_oracle():
    """M = 24 pairs from first_pair = P - 7.  Measured: error 5.0e-4 = 3.6e-2 TOL_Q_F32 (float32 oracle loss on the one-body
    samples 3.8e-4), |q| in [0.043, 4.4]."""
    ref, M, first = rl.spin_reference('diamond', True)
    sysd, dp, _ = system('diamond', torch.float32)
    out = sysd.spin_exchange_ratios(dp, cu(ref['x'], torch.float32), M, first_pair=first, want_ratios=True, want_walker=True)
    assert out['ratios'].dtype == torch.complex64 and out['walker'].dtype == torch.complex128
    q = complex_np(out['ratios'])
    err = rl.scaled(q, ref['q'])
    print(f'diamond float32 spin: max scaled |q - q_ref| = {err.max():.3e} = {err.max() / TOL_Q_F32:.3e} TOL_Q_F32, float32 oracle loss '
          f'(one-body samples) {rl.onebody_f32_oracle_loss("diamond"):.3e}, {rl.q_range(ref["q"])}')
    assert np.all(np.isfinite(ref['q'])) and err.max() <= TOL_Q_F32
    assert out['n_bad'].tolist() == [0]
    t = complex_np(out['walker'])
    assert np.all(np.abs(t - q.sum(axis=1)) <= M * 2.0 ** -23 * np.abs(q).sum(axis=1))


def test_ecp_float32_diamond_vs_float32_oracle():
    """The float32 system on the float32-rounded walkers: the pairs are the float64 count there ([17, 18]; `fixture` asserts the
    margin to every cutoff at the rounded walkers), E_loc meets the model's float64 bound, ratios and E_nl the float32 oracle
    within TOL_Q_F32.  Measured: ratio error 6.1e-4 = 4.4e-2 TOL_Q_F32 (float32 oracle loss on the one-body samples 3.8e-4),
    |q| in [0.023, 11.9]."""
    ref, out = run_ecp('diamond', f32=True)
    assert out['ratios'].dtype == torch.complex64 and out['e_nl'].dtype == torch.complex128 and out['e_loc'].dtype == torch.float64
    assert out['pairs'].tolist() == eh.LARGE_CASES['diamond'][1] == ref['pairs']['counts'].tolist()
    assert np.all(np.abs(out['e_loc'].cpu().numpy() - ref['e_loc']) <= e_loc_bound(ref))
    err = rl.scaled(complex_np(out['ratios']), ref['q'])
    print(f'diamond float32 pseudopotential: max scaled |q - q_ref| = {err.max():.3e} = {err.max() / TOL_Q_F32:.3e} TOL_Q_F32, float32 '
          f'oracle loss (one-body samples) {rl.onebody_f32_oracle_loss("diamond"):.3e}, {rl.q_range(ref["q"])}')
    check_against_reference(ref, out, TOL_Q_F32, 12)


# =================================================================================================== B. full batches
# ------------------------------------------------------------------------------------------------ 5. one-body, 67 100 configurations
def test_onebody_more_configurations_than_65520_on_distinct_walkers():
    """lih, B = 1100 distinct walkers, M = 61 from first_electron = 3, Philox mode, default workspace: 67 100 configurations.
    - shifts equal the replay to 1 ulp; q equals the oracle's within TOL_Q on walkers 0, 1074 (its samples are configurations
      65 514 .. 65 574) and 1099;
    - every walker equals the same call made in four slices of 275 walkers with the exported shifts as explicit ones, within TOL_Q
      (nothing in DESIGN.md promises that the value chain of a walker has the same bits in another batch);
    - nk_sums (27 k points) equals the numpy fold of the exported q and s within 16 P 2^-53 sum |q|, and is bit-identical with
      the workspace capped to two groups;
    - the default workspace holds 64 groups, so its chunks are 5120 configurations.  A workspace with room for every group of the
      call, given through the C ABI, is cut at OB_MAX_GROUPS = 819 groups: the second chunk then begins at configuration 65 520,
      inside walker 1074.  Ratios and sums are bit-identical again.
    Measured: oracle error 1.3e-4 TOL_Q, |q| in [0.087, 4.7]; slices differ by 0 (bit-identical); fold error 7.0e-5 of its bound;
    the workspace for all 839 groups is 2.7 GiB (default 209 MiB)."""
    ref = rl.onebody_big_reference()
    B, M = rl.OB_BIG
    first, nelec = rl.LIH_FIRST, ref['nelec']
    assert B * M > 65520
    sysd, dp, cell = system('lih')
    kv = kpoints(cell, sh.case('lih')[2], 27)
    x = cu(ref['x'])
    kw = dict(kvec=kv, first_electron=first, seed=rl.SEED, offset=rl.OFFSET, want_ratios=True)
    out = sysd.one_body_ratios(dp, x, M, want_shifts=True, **kw)
    s = out['shifts'].cpu().numpy()
    assert s.shape == (B, M, 3) and np.all(np.abs(s - ref['s']) <= np.spacing(np.abs(ref['s'])))
    q = complex_np(out['ratios'])
    assert out['n_bad'].tolist() == [0, 0] and np.all(np.isfinite(q))
    err = rl.scaled(q[list(rl.OB_CHECK)], ref['q'])
    print(f'walkers {rl.OB_CHECK}: max scaled |q - q_ref| / TOL_Q = {err.max() / TOL_Q:.3e}, {rl.q_range(ref["q"])}')
    assert err.max() <= TOL_Q
    worst = 0.0
    for k in range(4):
        sl = slice(275 * k, 275 * (k + 1))
        part = sysd.one_body_ratios(dp, x[sl].contiguous(), M, first_electron=first, shifts=out['shifts'][sl].contiguous(), want_ratios=True)
        worst = max(worst, rl.scaled(complex_np(part['ratios']), q[sl]).max())
    print(f'four slices of 275 walkers: max scaled |q_slice - q| / TOL_Q = {worst / TOL_Q:.3e}')
    assert worst <= TOL_Q
    fold_check(out['nk_sums'].cpu().numpy(), q, s, kv, first, nelec, 'B = 1100, M = 61')
    call = lambda max_bytes: sysd.one_body_ratios(dp, x, M, max_bytes=max_bytes, **kw)
    full = int(sysd.lib.ds_one_body_workspace_bytes(sysd.handle, B, M))
    two = capped_bytes(one_group_bytes(call), full, 64, 2)
    small = call(two)
    assert same_bits(small['nk_sums'], out['nk_sums']) and same_bits(small['ratios'], out['ratios'])
    assert small['n_bad'].tolist() == [0, 0]
    groups = (B * M + 79) // 80
    assert groups > 819
    ws = torch.empty(room_for(one_group_bytes(call), full, 64, groups), dtype=torch.uint8, device='cuda')
    print(f'workspace for {groups} groups: {ws.numel() / 2 ** 20:.0f} MiB (default {full / 2 ** 20:.0f} MiB)')
    sums = torch.zeros(2, 27, 2, dtype=torch.float64, device='cuda')
    ratio = torch.empty(B, M, 2, dtype=torch.float64, device='cuda')
    n_bad = torch.zeros(2, dtype=torch.int64, device='cuda')
    kvd = cu(kv)
    rc = sysd.lib.ds_one_body_ratios(sysd.handle, ptr(sysd.pack_params(dp)), ptr(x), B, M, first, rl.SEED, rl.OFFSET, ptr(None), ptr(kvd), 27,
                                     ptr(sums), ptr(ratio), ptr(None), ptr(n_bad), ptr(ws), ws.numel(), stream())
    assert rc == 0, sysd.lib.ds_last_error().decode()
    assert same_bits(sums, out['nk_sums']) and same_bits(torch.view_as_complex(ratio), out['ratios']) and n_bad.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 6. the base forward in passes
def test_undisplaced_forward_in_several_passes_gives_identical_bits():
    """lih, B = 400 distinct walkers.  A workspace capped to two groups (one for the spin pass) holds 160 (80) configurations, so the
    forward of the 400 undisplaced walkers, which runs in the same buffers, takes three (five) passes: ratios and sums of the
    three entry points are bit-identical to the uncapped call, whose workspace holds all 400 in one pass."""
    B, M = 400, 2
    cell, klist = sh.case('lih')[1], sh.case('lih')[2]
    sysd, dp, _ = system('lih')
    x = cu(rl.lih_walkers(B))
    # one-body: 800 configurations = 10 groups uncapped
    kw = dict(kvec=kpoints(cell, klist, 27), first_electron=1, seed=rl.SEED, offset=2, want_ratios=True)
    call = lambda max_bytes=None: sysd.one_body_ratios(dp, x, M, max_bytes=max_bytes, **kw)
    two = capped_bytes(one_group_bytes(call), int(sysd.lib.ds_one_body_workspace_bytes(sysd.handle, B, M)), 10, 2)
    assert B > 2 * 80
    big, small = call(), call(two)
    assert same_bits(small['ratios'], big['ratios']) and same_bits(small['nk_sums'], big['nk_sums'])
    assert bool(big['nk_sums'].abs().sum() > 0) and big['n_bad'].tolist() == small['n_bad'].tolist() == [0, 0]
    # spin: the smallest workspace the call accepts is one group
    kw = dict(first_pair=3, want_ratios=True, want_walker=True)
    call = lambda max_bytes=None: sysd.spin_exchange_ratios(dp, x, M, max_bytes=max_bytes, **kw)
    one = one_group_bytes(call)
    assert one < int(sysd.lib.ds_spin_exchange_workspace_bytes(sysd.handle, B, M)) and B > 80
    big, small = call(), call(one)
    for k in ('ratios', 'walker', 'sums', 'n_bad'):
        assert same_bits(small[k], big[k]), k
    assert float(big['sums'][3]) == B
    with pytest.raises(RuntimeError, match='workspace too small'):
        call(one - 1)
    # pseudopotential: the default capacity B N = 1600 pairs, 19 200 configurations = 240 groups, of which a workspace gets 64
    ecp = eh.make_ecp(cell, eh.CASES['lih'][0])
    kw = dict(seed=eh.SEED, offset=eh.OFFSET, want_pairs=True, want_ratios=True)
    call = lambda max_bytes=None: sysd.ecp_energy(dp, x, ecp, max_bytes=max_bytes, **kw)
    big = call()                                                                  # (builds the device tables and keeps them on ecp)
    full =int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, ecp.__dict__['_ds_tables'].handle, B, B * 4))
    two = capped_bytes(one_group_bytes(call), full, 64, 2)
    small = call(two)
    assert int(big['pairs'].sum()) * 12 > 2 * 80
    for k in ('ratios', 'e_loc', 'e_nl', 'pairs'):
        assert same_bits(small[k], big[k]), k
    assert bool(torch.isfinite(torch.view_as_real(big['e_nl'])).all()) and bool(big['e_nl'].abs().sum() > 0)


def test_capped_workspace_gives_identical_bits_across_the_int8_threshold():
    """bcc_li (24 electrons): a launch of the value chain with 22 or more groups of 80 configurations (512 (group, electron) tiles)
    runs its residual hidden layers as the int8 split, a smaller one on the float64 kernels; the two agree to 1e-12, not to the
    bit.  The ratio passes decide once per call, from all its configurations, so a workspace capped to two groups -- whose launches
    are far below the threshold -- still gives the bits of the uncapped call, whose launches are above it, as their documentation
    promises.  (While every launch decided for itself the capped and the uncapped call took different kernels: on lih with
    B = 1100, M = 61 and room for 128 groups or more the ratios moved by up to 7.8e-12 max(1, |q|), the sums by 4e-10.)"""
    fx, cell, klist, _, _ = sh.case('bcc_li')
    sysd, dp, _ = system('bcc_li')
    x = cu(np.asarray(fx['x'], dtype=np.float64))
    B, M = len(fx['x']), 450
    assert 24 * ((B * M + 79) // 80) >= 512 > 24 * 2
    kw = dict(kvec=kpoints(cell, klist, 27), first_electron=5, seed=rl.SEED, offset=9, want_ratios=True)
    call = lambda max_bytes=None: sysd.one_body_ratios(dp, x, M, max_bytes=max_bytes, **kw)
    full_groups = (B * M + 79) // 80
    two = capped_bytes(one_group_bytes(call), int(sysd.lib.ds_one_body_workspace_bytes(sysd.handle, B, M)), full_groups, 2)
    big, small = call(), call(two)
    assert same_bits(small['ratios'], big['ratios']) and same_bits(small['nk_sums'], big['nk_sums'])
    kw = dict(first_pair=140, want_ratios=True, want_walker=True)
    call = lambda max_bytes=None: sysd.spin_exchange_ratios(dp, x, M, max_bytes=max_bytes, **kw)
    big, small = call(), call(one_group_bytes(call))
    for k in ('ratios', 'walker', 'sums'):
        assert same_bits(small[k], big[k]), k
    xe = cu(sh.distinct_walkers(cell, fx['x'], 12))
    ecp = eh.make_ecp(cell, eh.CASES['bcc_li'][0])
    kw = dict(seed=eh.SEED, offset=eh.OFFSET, want_pairs=True, want_ratios=True)
    call = lambda max_bytes=None: sysd.ecp_energy(dp, xe, ecp, max_bytes=max_bytes, **kw)
    big = call()
    assert 24 * ((int(big['pairs'].sum()) * 12 + 79) // 80) >= 512
    full = int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, ecp.__dict__['_ds_tables'].handle, 12, 12 * 24))
    small = call(capped_bytes(one_group_bytes(call), full, (12 * 24 * 12 + 79) // 80, 2))
    for k in ('ratios', 'e_loc', 'e_nl', 'pairs'):
        assert same_bits(small[k], big[k]), k


# ------------------------------------------------------------------------------------------------ 7. spin, B = 700
def test_spin_more_walkers_than_threads_of_the_final_sum():
    """lih, B = 700 = 2 * 256 + 188 distinct walkers, M = 4 = P: thread t of k_spin_final adds walkers t, t + 256 and t + 512.
    Walkers 300 and 699 carry a NaN coordinate: `walker` is NaN exactly there, n_bad = 2, `sums` follows from the 698 others
    within the rounding bound of test_gpu_spin.check_sums; q equals the oracle's on walkers 0, 255, 256 and 698 within TOL_Q.
    Measured: oracle error 8.2e-7 TOL_Q, |q| in [1.7e-3, 2.0]; sums[0] equals the model of the order to the bit."""
    ref = rl.spin_big_reference()
    B, M = rl.SPIN_BIG
    sysd, dp, _ = system('lih')
    out = sysd.spin_exchange_ratios(dp, cu(ref['x']), M, want_ratios=True, want_walker=True)
    good = check_sums(out, B)
    bad = np.flatnonzero(~good)
    assert bad.tolist() == list(rl.SPIN_BAD) and out['n_bad'].tolist() == [2] and float(out['sums'][3]) == B - 2
    t = complex_np(out['walker'])
    assert np.isnan(t.real).nonzero()[0].tolist() == list(rl.SPIN_BAD) and np.all(np.isfinite(t[good]))
    # the packed sums in the order of k_spin_final: thread t adds w = t, t + 256, ..., thread 0 adds the 256 results in order
    tr = np.where(good, t.real, 0.0)
    model = np.zeros(256)
    for w0 in range(0, B, 256):
        seg = tr[w0:w0 + 256]
        model[:len(seg)] = model[:len(seg)] + seg
    total = 0.0
    for v in model:
        total = total + v
    print(f'sums[0] = {float(out["sums"][0])!r}, model of the order {total!r}')
    assert abs(float(out['sums'][0]) - total) <= B * 2.0 ** -52 * np.abs(tr).sum()
    q = complex_np(out['ratios'])
    err = rl.scaled(q[list(rl.SPIN_CHECK)], ref['q'])
    print(f'walkers {rl.SPIN_CHECK}: max scaled |q - q_ref| / TOL_Q = {err.max() / TOL_Q:.3e}, {rl.q_range(ref["q"])}')
    assert err.max() <= TOL_Q


# ------------------------------------------------------------------------------------------------ 8. pseudopotential, B = 2100
def test_ecp_more_walkers_than_threads_of_the_offset_scan():
    """lih, B = 2100 distinct walkers, N_q = 12, default workspace: k_ecp_offsets gives each of its 1024 threads three walkers and
    threads 700.. none; 7703 pairs, 92 436 configurations > 65 520.
    - pairs equal the numpy pair list on all walkers, E_loc the model within its float64 bound on all walkers;
    - ratios (at the offsets of the model's pair list) and E_nl equal the oracle's within TOL_Q (TOL_Q times the walker's scale) on
      walkers 0, 1023, 1024, 2099 and on the walker that holds configuration 65 520;
    - E_nl is bit-identical with the workspace capped to two groups, and with a workspace for every group of the call given
      through the C ABI (the default one holds 64 groups: chunks of 5120; that one is cut at OB_MAX_GROUPS = 819 groups, so the
      second chunk begins at configuration 65 520, inside a walker);
    - a NaN coordinate in walker 1500 gives NaN there and the same bits in every other walker: the offsets behind it stay right.
    Measured: ratio error 1.2e-4 TOL_Q, E_nl error 3.0e-5 of its bound, E_loc error 0.085 of its bound; walker 1488 holds
    configuration 65 520; the workspace for all 1260 groups is 4.0 GiB (default 212 MiB)."""
    ref = rl.ecp_big_reference()
    B, nq = rl.ECP_BIG, 12
    pl, off = ref['pairs'], ref['off']
    assert off[-1] > 65520
    sysd, dp, _ = system('lih')
    x = cu(ref['x'])
    kw = dict(seed=eh.SEED, offset=eh.OFFSET, want_pairs=True, want_ratios=True)
    call = lambda max_bytes=None: sysd.ecp_energy(dp, x, ref['ecp'], max_bytes=max_bytes, **kw)
    out = call()
    assert np.array_equal(out['pairs'].cpu().numpy(), pl['counts']) and out['ratios'].shape == (off[-1],)
    err, bound = np.abs(out['e_loc'].cpu().numpy() - ref['e_loc']), (8 + ref['e_loc_terms']) * eh.EPS * ref['e_loc_mag']
    k = ref['e_loc_terms'] > 0
    print(f'max |E_loc - model| / bound = {(err[k] / bound[k]).max():.3e} over {int(k.sum())} walkers with a term')
    assert np.all(err <= bound)
    q, e = complex_np(out['ratios']), complex_np(out['e_nl'])
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(e))
    worst_q = worst_e = 0.0
    for w in ref['check']:
        assert len(ref['q'][w]) == off[w + 1] - off[w] > 0, w
        worst_q = max(worst_q, rl.scaled(q[off[w]:off[w + 1]], ref['q'][w]).max())
        worst_e = max(worst_e, abs(e[w] - ref['e_nl'][w]) / (TOL_Q * ref['e_nl_scale'][w]))
    print(f'walkers {ref["check"]}: max scaled |q - q_ref| / TOL_Q = {worst_q / TOL_Q:.3e}, max |E_nl - model| / bound = {worst_e:.3e}')
    assert worst_q <= TOL_Q and worst_e <= 1.0
    # every walker's energy is the sum of its own terms, at the model's offsets
    mine, scale = eh.energy(q, ref['Wn'], pl, B, nq)
    assert np.all(np.abs(e - mine) <= 64 * eh.EPS * scale)
    full = int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, ref['ecp'].__dict__['_ds_tables'].handle, B, B * 4))
    one = one_group_bytes(call)
    small = call(capped_bytes(one, full, 64, 2))
    assert same_bits(small['e_nl'], out['e_nl']) and same_bits(small['ratios'], out['ratios']) and same_bits(small['e_loc'], out['e_loc'])
    groups = (B * 4 * nq + 79) // 80                                              # of the capacity B N: what the library sizes chunks by
    assert groups > 819
    ws = torch.empty(room_for(one, full, 64, groups), dtype=torch.uint8, device='cuda')
    print(f'workspace for {groups} groups: {ws.numel() / 2 ** 20:.0f} MiB (default {full / 2 ** 20:.0f} MiB)')
    energy = torch.empty(B, 3, dtype=torch.float64, device='cuda')
    rc = raw_call(sysd, ref['ecp'].__dict__['_ds_tables'], sysd.pack_params(dp), x, B, B * 4, energy, ws)
    assert rc == 0, sysd.lib.ds_last_error().decode()
    torch.cuda.synchronize()
    assert same_bits(energy[:, 0], out['e_loc']) and same_bits(torch.complex(energy[:, 1], energy[:, 2]), out['e_nl'])
    xb = np.array(ref['x'])
    xb[rl.ECP_BAD, 7] = np.nan
    bad = sysd.ecp_energy(dp, cu(xb), ref['ecp'], **kw)
    counts = pl['counts'].copy()
    counts[rl.ECP_BAD] = 0
    assert np.array_equal(bad['pairs'].cpu().numpy(), counts)
    eb = complex_np(bad['e_nl'])
    assert np.flatnonzero(np.isnan(eb.real)).tolist() == [rl.ECP_BAD] and np.isnan(float(bad['e_loc'][rl.ECP_BAD]))
    keep = torch.as_tensor(np.flatnonzero(np.arange(B) != rl.ECP_BAD), device='cuda')
    assert same_bits(bad['e_nl'][keep], out['e_nl'][keep]) and same_bits(bad['e_loc'][keep], out['e_loc'][keep])
    assert bad['ratios'].shape == (off[-1] - pl['counts'][rl.ECP_BAD] * nq,) and pl['counts'][rl.ECP_BAD] > 0
    qb = complex_np(bad['ratios'])
    cut = off[rl.ECP_BAD]
    assert np.array_equal(qb[:cut], q[:cut]) and np.array_equal(qb[cut:], q[off[rl.ECP_BAD + 1]:])


# ------------------------------------------------------------------------------------------------ 9. n_k at its cap
def test_momentum_sums_with_512_and_511_k_points():
    """lih, six walkers, M = 5 explicit shifts, 512 seeded random k points (the fold needs no lattice points): the last k row of a
    partial row lies beside the two bad counts (OB_ROW = 4 * 512 + 2).  One sample of each spin has a NaN shift: nk_sums equals the
    numpy fold of the exported q without them, n_bad = [1, 1]; a second call doubles the buffer exactly; the call with the first
    511 points gives the first 511 rows to the bit.  Measured: fold error 6.0e-2 of its bound."""
    fx, cell, _, _, _ = sh.case('lih')
    sysd, dp, _ = system('lih')
    nelec = (2, 2)
    x = np.asarray(fx['x'], dtype=np.float64)
    B, M, first = len(x), 5, 0
    assert B == 6
    rng = np.random.default_rng(512)
    kv = rng.normal(0.0, 1.0, (512, 3))
    s = rng.uniform(0.0, 1.0, (B, M, 3)) @ np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    s[1, 1] = np.nan                                                       # electron 1: spin up
    s[4, 2] = np.nan                                                       # electron 2: spin down
    kw = dict(first_electron=first, shifts=cu(s), want_ratios=True)
    out = sysd.one_body_ratios(dp, cu(x), M, kvec=kv, **kw)
    q = complex_np(out['ratios'])
    bad = ~np.isfinite(q)
    assert np.argwhere(bad).tolist() == [[1, 1], [4, 2]] and out['n_bad'].tolist() == [1, 1]
    sums = out['nk_sums']
    assert sums.shape == (2, 512, 2) and bool(torch.isfinite(sums).all()) and bool((sums.abs().sum(dim=(1, 2)) > 0).all())
    fold_check(sums.cpu().numpy(), q, s, kv, first, nelec, 'n_k = 512')
    first_call = sums.clone()
    again = sysd.one_body_ratios(dp, cu(x), M, kvec=kv, nk_sums=sums, **kw)
    assert torch.equal(sums, 2 * first_call) and again['n_bad'].tolist() == [1, 1]
    less = sysd.one_body_ratios(dp, cu(x), M, kvec=kv[:511], **kw)
    assert less['nk_sums'].shape == (2, 511, 2) and torch.equal(less['nk_sums'], first_call[:, :511]) and less['n_bad'].tolist() == [1, 1]
