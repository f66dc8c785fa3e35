"""GPU tests of the four fused Metropolis samplers (csrc/ds_mcmc.h) and of the walker gradient `ds_logpsi_grad` against the
float64 CPU oracle (oracle/qmc.py per move, torch autograd over oracle/network.py), beyond small float64 cells:

* the in-kernel Philox stream, replayed by the numpy model of sampler_helpers.py: a chain in seed mode equals the same chain fed
  the model's noise, and both equal the oracle's chain (B = 70: two accept workgroups, the second partial);
* the complex walker gradient, both halves, on twisted cells, every network option, unequal and mirrored spin channels, the
  large cells' trace kernels, float32, ragged / empty / chunked batches;
* single moves of all four samplers on 48- and 96-electron cells and in float32, from the oracle's own state.

A Metropolis decision is discontinuous, so every comparison of decisions is made where the oracle's margin ratio - log u exceeds
the tolerance on lp; the seeds (tools/find_sampler_seeds.py) make that every decision, and each test asserts it at run time."""
import numpy as np
import pytest
import torch

import sampler_helpers as sh
from common import float32_tolerance

pytestmark = pytest.mark.gpu

TOL_X = {'mh': 1e-10, 'one': 1e-10, 'asym': 1e-10, 'imp': 1e-9}        # the tolerances of test_gpu_vmc.py for these moves
TOL_LP = {'mh': 1e-8, 'one': 1e-8, 'asym': 1e-8, 'imp': 1e-7}


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(vv, dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v] for k, v in params.items()}


def slog_net(name, dtype=torch.float64):
    """-> (eval_slogdet network of the case on the device, its parameters, cell)."""
    from deepsolid_amd import network
    _, cell, klist, net_kw, params = sh.case(name)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', dtype=dtype, **net_kw)
    return net, dev_params(params, dtype), cell


def cu(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device='cuda')


def fused(sysd, dp, kind, cell, x0, steps, width, seed=None, offset=0, nz=None, un=None, lp=None, first=0):
    """One fused C-ABI call of sampler `kind` from x0 (and lp, when given: lp_valid) -> (x, lp, accept count)."""
    x = x0.clone()
    lp_valid = lp is not None
    lp = lp.clone() if lp_valid else torch.empty(x.shape[0], dtype=x.dtype, device=x.device)
    kw = {'mh': {}, 'one': dict(first_electron=first), 'imp': dict(importance=True), 'asym': dict(atoms=sh.nuclei(cell))}[kind]
    if nz is not None:
        kw.update(normals=cu(nz, x.dtype), uniforms=cu(un, x.dtype))
    else:
        kw.update(seed=seed, offset=offset)
    nacc = sysd.mcmc_step(dp, x, lp, steps, width, lp_valid=lp_valid, **kw)
    return x, lp, float(nacc.item())


def per_move(kind, net, dp, cell, x1, lp1, width, nz, un, i=0):
    """The per-move entry point of deepsolid_amd.qmc for `kind` -> (x_new, lp_new, accept count)."""
    from deepsolid_amd import qmc
    nacc = torch.zeros(1, dtype=x1.dtype, device='cuda')
    kw = dict(stddev=width, normal=cu(nz, x1.dtype), uniform=cu(un, x1.dtype))
    if kind == 'mh':
        x, _, lp, nacc = qmc.mh_update(dp, net.apply, x1, None, lp1, nacc, cell.a, **kw)
    elif kind == 'asym':
        x, _, lp, nacc = qmc.mh_update(dp, net.apply, x1, None, lp1, nacc, cell.a, atoms=sh.nuclei(cell), **kw)
    elif kind == 'one':
        x, _, lp, nacc = qmc.mh_one_electron_update(dp, net.apply, x1, None, lp1, nacc, cell.a, i=i, **kw)
    else:
        x, _, lp, nacc = qmc.importance_update(dp, net.apply.value_and_grad, x1, None, lp1, nacc, cell.a, **kw)
    return x, lp, float(nacc.item())


def make_step(kind, net, cell, B, steps):
    from deepsolid_amd import qmc
    kw = {'mh': {}, 'one': dict(one_electron_moves=True), 'imp': dict(importance_sampling=net.apply), 'asym': dict(atoms=sh.nuclei(cell))}[kind]
    return qmc.make_mcmc_step(net.apply, B, cell.a, steps=steps, **kw)


def moved_rows(x_new, x_old):
    return (x_new != x_old).any(dim=1).cpu()


# ------------------------------------------------------------------------------------------------ 2. Philox mode = replay = oracle
@pytest.mark.parametrize('name,kind', sorted(sh.CHAINS))
def test_philox_chain_equals_replayed_chain_and_oracle(name, kind, record_property):
    """A chain in seed mode, the same chain with sampler_helpers.noise(...) as explicit noise, and the oracle's chain on the
    same arrays, move by move (single-move calls with offset = i and the previous lp), then the whole chain as ONE call
    (make_mcmc_step), which must equal the move-by-move result bit for bit in both modes.
    Seed against replay: the same walkers move at every step and pmove is equal, exactly; x and lp to 1e-12 (the device's log /
    sincos against numpy's in the Box-Muller map is the only licensed difference).  Against the oracle: x 1e-10, lp 1e-8
    (importance move 1e-9 / 1e-7), equal decisions and accept counts."""
    seed, width, steps = sh.CHAINS[(name, kind)]
    B = sh.CHAIN_BATCH
    ref = sh.chain_reference(name, kind, seed, width, B, steps)
    sh.assert_conditions(ref['cond3'])
    record_property('min_margin', ref['cond3']['min_margin'])
    net, dp, cell = slog_net(name)
    sysd = net.apply.system
    N = sysd.n
    assert steps == (N if kind == 'one' else steps)
    x0 = cu(ref['x0'])
    xs, lps, xr, lpr, total = x0, None, x0, None, 0.0
    for i, m in enumerate(ref['moves']):
        xs2, lps, na_s = fused(sysd, dp, kind, cell, xs, 1, width, seed=seed, offset=i, lp=lps, first=i % N)
        xr2, lpr, na_r = fused(sysd, dp, kind, cell, xr, 1, width, nz=ref['nz'][i:i + 1], un=ref['un'][i:i + 1], lp=lpr, first=i % N)
        mv_s, mv_r = moved_rows(xs2, xs), moved_rows(xr2, xr)
        assert torch.equal(mv_s, mv_r) and na_s == na_r, (i, mv_s.nonzero().reshape(-1).tolist(), mv_r.nonzero().reshape(-1).tolist())
        assert torch.equal(mv_r, m['cond']) and na_r == m['nacc'] == int(mv_r.sum()), (i, (mv_r != m['cond']).nonzero().reshape(-1).tolist())
        assert float((xs2 - xr2).abs().max()) <= 1e-12 and float((lps - lpr).abs().max()) <= 1e-12, i
        assert float((xr2.cpu() - m['x']).abs().max()) <= TOL_X[kind], i
        assert float((lpr.cpu() - m['lp']).abs().max()) <= TOL_LP[kind], i
        xs, xr, total = xs2, xr2, total + na_r
    step = make_step(kind, net, cell, B, 1 if kind == 'one' else steps)
    xf_s, pm_s = step(dp, x0, seed, width)
    xf_r, pm_r = step(dp, x0, (cu(ref['nz']), cu(ref['un'])), width)
    assert torch.equal(xf_s, xs) and torch.equal(xf_r, xr)
    assert float(pm_s) == float(pm_r) and abs(float(pm_r) - total / (steps * B)) < 1e-15


@pytest.mark.parametrize('kind', sh.KINDS)
@pytest.mark.parametrize('name', ['lih', 'bcc_li'])
def test_four_moves_equal_two_calls_of_two(name, kind):
    """steps = 4 in one call equals two calls of steps = 2, the second with offset = 2 and lp_valid=True (and, for the
    one-electron sampler, first_electron advanced by 2), bit for bit: the counter is offset + step and lp is carried."""
    net, dp, cell = slog_net(name)
    sysd = net.apply.system
    fx = sh.case(name)[0]
    x0 = cu(sh.tiled_walkers(cell, fx['mcmc_x0'], sh.CHAIN_BATCH))
    width = sh.CHAINS[(name, kind)][1]
    first = 1
    x4, lp4, n4 = fused(sysd, dp, kind, cell, x0, 4, width, seed=77, offset=5, first=first)
    xa, lpa, na = fused(sysd, dp, kind, cell, x0, 2, width, seed=77, offset=5, first=first)
    xb, lpb, nb = fused(sysd, dp, kind, cell, xa, 2, width, seed=77, offset=7, lp=lpa, first=(first + 2) % sysd.n)
    assert torch.equal(x4, xb) and torch.equal(lp4, lpb) and n4 == na + nb
    assert 0 < n4 < 4 * sh.CHAIN_BATCH
    # the lp a call leaves behind is 2 log|psi| of the walkers it leaves behind (the contract lp_valid relies on)
    if kind != 'imp':          # (the importance move's lp carries its proposal densities as well)
        assert float((lp4 - 2.0 * net.apply(dp, x4)).abs().max()) <= 1e-9 * max(1.0, float(lp4.abs().max()))


@pytest.mark.parametrize('name', ['lih', 'bcc_li'])
def test_one_electron_sampler_moves_electron_first_plus_i(name):
    """`first_electron` = k != 0: move i displaces electron (k + i) % N, by the deviates of THAT electron (index walker * N +
    electron of the Philox stream).  Every other electron of an accepted walker is bit-identical to the wrap of its old position
    (the reference wraps the whole configuration, qmc.py:271; `ds_mh_propose` with zero noise is that wrap), a rejected walker is
    bit-identical altogether; and seed mode agrees with the replay of noise(..., first_electron=k)."""
    net, dp, cell = slog_net(name)
    sysd = net.apply.system
    N, B, width, seed = sysd.n, sh.CHAIN_BATCH, 0.5, 4
    k = N - 2
    fx = sh.case(name)[0]
    x = cu(sh.tiled_walkers(cell, fx['mcmc_x0'], B))
    nz, un = sh.noise(seed, 0, 3, B, N, one_electron=True, first_electron=k)
    xr, lpr, nr = fused(sysd, dp, 'one', cell, x, 3, width, nz=nz, un=un, first=k)
    prev, lp = x, None
    for i in range(3):
        e = (k + i) % N
        # moves 0..i in one call (first_electron = k throughout); the earlier moves are replayed identically: pure function of the key
        cur, lp_i, _ = fused(sysd, dp, 'one', cell, x, i + 1, width, seed=seed, first=k)
        wrapped = sysd.mh_propose(prev, torch.zeros_like(prev), width)
        acc = moved_rows(cur, prev).cuda()
        others = torch.ones(3 * N, dtype=torch.bool, device='cuda')
        others[3 * e:3 * e + 3] = False
        assert 0 < int(acc.sum()) < B
        assert torch.equal(cur[~acc], prev[~acc])
        assert torch.equal(cur[acc][:, others], wrapped[acc][:, others])
        assert bool((cur[acc][:, ~others] != prev[acc][:, ~others]).any(dim=1).all())
        # the displacement of electron e is width * (its own three deviates), minimum image
        a = cu(np.asarray(cell.a, dtype=np.float64).reshape(3, 3))
        d = (cur[acc][:, ~others] - prev[acc][:, ~others]) @ torch.linalg.inv(a)
        d = (d - torch.round(d)) @ a
        assert float((d - width * cu(nz[i])[acc]).abs().max()) <= 1e-10
        prev = cur
    assert float((prev - xr).abs().max()) <= 1e-12 and torch.equal(moved_rows(prev, x), moved_rows(xr, x))


# ------------------------------------------------------------------------------------------------ 3. walker gradient
def grad_tolerance_f64(g_ref):
    return 1e-8 * max(1.0, float(g_ref.abs().max()))


GRAD_CASES = [('lih_twist', 3), ('bcc_li_twist', 2), ('lih_fulldet', 3), ('lih_tri', 3), ('lih_lastlayer', 3), ('lih_fullenv', 3),
              ('lih_diagenv', 3), ('li_polarized', 3), ('mirror_0_3', 3), ('mirror_1_2', 3), ('graphene', 2), ('diamond', 2),
              ('bcc_li_333', 1)]


@pytest.mark.parametrize('name,B', GRAD_CASES)
def test_walker_gradient_both_halves_vs_oracle_autograd(name, B):
    """`SystemDevice.logpsi_grad` against autograd over the oracle's eval_logdet: Re = grad log|psi|, Im = grad arg psi, each to
    1e-8 * max(1, max|g_ref|) of its own half.  Twisted cells (non-trivial phase gradient), the network options, unequal and
    mirrored spin channels (the gradient comes back in the caller's electron order), and the determinant-trace variants of the
    48-, 81- and 96-electron cells."""
    from deepsolid_amd import systems
    fx, cell, _, _, _ = sh.case(name)
    net, dp, _ = slog_net(name)
    x = fx['x'][:B] if fx is not None else systems.synthetic_walkers(cell, B, seed=8)
    la_ref, g_ref = sh.oracle(name).value_and_grad(x)
    la, g = net.apply.system.logpsi_grad(dp, cu(x))
    g = g.cpu()
    assert g.shape == (B, x.shape[1]) and g.dtype == torch.complex128
    assert float((la.cpu() - la_ref).abs().max()) <= 1e-9 * max(1.0, float(la_ref.abs().max()))
    for half, got, ref in (('re', g.real, g_ref.real), ('im', g.imag, g_ref.imag)):
        err = (got - ref).abs()
        b, c = divmod(int(err.argmax()), err.shape[1])
        assert float(err.max()) <= grad_tolerance_f64(ref), (half, 'walker', b, 'electron', c // 3, float(err.max()), float(ref.abs().max()))
    if 'twist' in name:
        assert float(g_ref.imag.abs().max()) > 0.1                     # the phase gradient is really there


def test_walker_gradient_ragged_empty_and_chunked_batches():
    """lih: B = 1; B = 0 (empty tensors of the right shape); B = 67 of tiled walkers, where every row equals the single-walker
    call of its walker bit for bit; and a workspace of five walkers minus a little on B = 17 (chunks 4+4+4+4+1: the library offsets
    the gradient by the chunk start), bit-identical to the full workspace."""
    fx, cell, _, _, _ = sh.case('lih')
    net, dp, _ = slog_net('lih')
    sysd = net.apply.system
    nw = len(fx['x'])
    la_ref, g_ref = sh.oracle('lih').value_and_grad(fx['x'])
    singles = [sysd.logpsi_grad(dp, cu(fx['x'][b:b + 1])) for b in range(nw)]
    for b, (la1, g1) in enumerate(singles):
        assert la1.shape == (1,) and g1.shape == (1, fx['x'].shape[1])
        assert float((g1[0].cpu().real - g_ref[b].real).abs().max()) <= grad_tolerance_f64(g_ref.real)
        assert float((g1[0].cpu().imag - g_ref[b].imag).abs().max()) <= grad_tolerance_f64(g_ref.imag)
    la0, g0 = sysd.logpsi_grad(dp, cu(fx['x'][:0]))
    assert la0.shape == (0,) and g0.shape == (0, fx['x'].shape[1]) and g0.dtype == torch.complex128
    x = cu(np.tile(fx['x'], (12, 1))[:67])
    la, g = sysd.logpsi_grad(dp, x)
    for b in range(67):
        assert torch.equal(la[b], singles[b % nw][0][0]), b
        assert torch.equal(torch.view_as_real(g[b]), torch.view_as_real(singles[b % nw][1][0])), b
    # bytes per walker of the chain's workspace: the slope of ds_workspace_bytes where the walker term decides (the value for
    # one walker is the larger per-group buffer of the value chain, so five times THAT would hold all 17 walkers in one chunk)
    per = (int(sysd.lib.ds_workspace_bytes(sysd.handle, 3000)) - int(sysd.lib.ds_workspace_bytes(sysd.handle, 2000))) // 1000
    assert per > 1024 and 17 * per > 5 * per - 1024
    la_c, g_c = sysd.logpsi_grad(dp, x[:17], ws_bytes=5 * per - 1024)
    assert torch.equal(la_c, la[:17]) and torch.equal(torch.view_as_real(g_c), torch.view_as_real(g[:17]))


def _grad_err(g, g64):
    """max over both halves of |g - g64| / max(1, max|g64|), per walker."""
    d = torch.view_as_real(g.to(torch.complex128) - g64).abs().flatten(1).max(dim=1).values
    return (d / torch.view_as_real(g64).abs().flatten(1).max(dim=1).values.clamp(min=1.0)).tolist()


@pytest.mark.parametrize('name,B', [('bcc_li', 4), ('diamond', 2)])
def test_walker_gradient_float32(name, B, record_property):
    """float32 at float32-rounded walkers against the float64 oracle.  The tolerance comes from the reference, not the kernel:
    the oracle's own gradient run in float32 at the same walkers loses max|g32 - g64| / max(1, max|g64|); the kernel gets 3 x
    that (the summation order differs), with the floor rule of common.float32_tolerance."""
    fx, cell, _, _, _ = sh.case(name)
    net, dp, _ = slog_net(name, torch.float32)
    x32 = fx['x'][:B].astype(np.float32)
    _, g64 = sh.oracle(name).value_and_grad(x32.astype(np.float64))
    _, g32 = sh.oracle(name, True).value_and_grad(x32)
    loss = _grad_err(g32, g64)
    la, g = net.apply.system.logpsi_grad(dp, cu(x32, torch.float32))
    assert g.dtype == torch.complex64
    err = _grad_err(g.cpu(), g64)
    record_property('oracle_f32_loss', loss)
    record_property('kernel_error', err)
    print(f'{name}: oracle float32 loss {loss}, kernel error {err}')
    for b in range(B):
        assert err[b] <= float32_tolerance(loss, b), (b, err[b], loss[b])


# ------------------------------------------------------------------------------------------------ 4. single moves
@pytest.mark.parametrize('name,f32,kind', sorted(sh.SINGLE_MOVES))
def test_single_move_from_oracle_state(name, f32, kind, record_property):
    """One move of each sampler from the oracle's own state (x1, lp1 = 2 log|psi| of the oracle) with explicit noise, on the
    48-electron cell (B = 4), the 96-electron cell (second trip of the accept kernel's electron loop; one-electron move of an
    electron >= 64) and in float32.  Every decision is decidable in the oracle (asserted), so the accept mask and count must be the
    oracle's.  float64: x 1e-10, lp 1e-8 (importance 1e-9 / 1e-7).  float32: x to 1e-5 * max(1, |cell|) per coordinate, lp within
    the float32 budget of the move (sampler_helpers.single_move_reference)."""
    seed, width, B, i = sh.SINGLE_MOVES[(name, f32, kind)]
    ref = sh.single_move_reference(name, kind, seed, width, B, i, f32)
    sh.assert_conditions(ref['cond3'])
    record_property('min_margin', ref['cond3']['min_margin'])
    if name == 'diamond' and kind == 'one':
        assert i % 96 >= 64
    dtype = torch.float32 if f32 else torch.float64
    net, dp, cell = slog_net(name, dtype)
    x1, lp1 = cu(ref['x1'], dtype), cu(ref['lp1'], dtype)
    x, lp, nacc = per_move(kind, net, dp, cell, x1, lp1, width, ref['nz'], ref['un'], i)
    acc = moved_rows(x, x1)
    assert torch.equal(acc, ref['cond']) and nacc == ref['nacc'], (acc.tolist(), ref['cond'].tolist(), ref['margin'].tolist())
    dx = (x.cpu().double() - ref['x']).abs().max(dim=1).values
    dlp = (lp.cpu().double() - ref['lp']).abs()
    if f32:
        record_property('oracle_f32_loss', ref['loss'])
        record_property('kernel_error', (dlp / ref['lp'].abs().clamp(min=1.0)).tolist())
        print(f'{name} {kind}: oracle float32 loss {ref["loss"]}, kernel lp error {(dlp / ref["lp"].abs().clamp(min=1.0)).tolist()}, '
              f'min margin {ref["cond3"]["min_margin"]}')
        assert float(dx.max()) <= 1e-5 * max(1.0, float(np.abs(np.asarray(cell.a)).max())), dx.tolist()
        assert bool((dlp <= ref['tol']).all()), (dlp.tolist(), ref['tol'].tolist())
    else:
        assert float(dx.max()) <= TOL_X[kind], dx.tolist()
        assert float(dlp.max()) <= TOL_LP[kind], dlp.tolist()


@pytest.mark.parametrize('kind', sh.KINDS)
def test_fused_loop_equals_per_move_loop_on_graphene(kind):
    """graphene (48 electrons) at B = 70, two moves, explicit noise: the fused C-ABI call of each sampler equals the per-move
    Python loop over the same kernels bit for bit (test_gpu_vmc.py checks this at 24 electrons)."""
    net, dp, cell = slog_net('graphene')
    sysd = net.apply.system
    fx = sh.case('graphene')[0]
    B, N = sh.CHAIN_BATCH, sysd.n
    x0 = cu(sh.tiled_walkers(cell, fx['x'], B))
    width = {'mh': 0.05, 'one': 0.5, 'imp': 0.05, 'asym': 0.02}[kind]
    nz, un = sh.noise(12, 0, 2, B, N, one_electron=kind == 'one')
    xf, lpf, nf = fused(sysd, dp, kind, cell, x0, 2, width, nz=nz, un=un)
    x, lp, n = x0, 2.0 * net.apply(dp, x0), 0.0
    for i in range(2):
        x, lp, na = per_move(kind, net, dp, cell, x, lp, width, nz[i], un[i], i)
        n += na
    assert torch.equal(xf, x) and torch.equal(lpf, lp) and nf == n
    assert 0 < n < 2 * B
