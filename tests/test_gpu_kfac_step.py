"""GPU tests of the KFAC step: `ds_kfac_inverses` / `ds_kfac_precondition` (csrc/ds_kfac.h) through the C ABI, the index map
between the packed gradient and the block matrices, `deepsolid_amd.kfac` and `run_training(optimizer='kfac')`, against the torch
restatement of tests/kfac_step_helpers.py (itself held to reference-executed inverses by tests/test_kfac_step_cpu.py).

Bounds (float64): every inverse within 1e-9 of its largest entry -- the bound tests/test_gpu_kfac.py holds the factors to -- after
asserting on the CPU that two independent float64 inversions of the same damped matrix (torch.linalg.inv and Cholesky) agree to
1e-10, so the bound does not hide conditioning; symmetry exact.  Preconditioner: 1e-9 of each block's largest entry and 1e-9
relative on each <P, V> (plain float64 products of at most 864 terms).  The deviations measured are recorded as test properties.
Measured on an MI355X, worst of a matrix's largest entry (the elimination WITHOUT its Newton step had missed 1e-9 on `lih_mixed` at
damping 1e-3, EXPERIMENTS.md "KFAC step"; with the one step):
  inverses at damping 1e-3: 1.3e-12 over the five earlier cases; bcc_li_333 8.8e-13, diamond 3.5e-12, graphene_331 4.6e-12 (orders up to
  865, condition up to 5.2e5: one Newton step is enough, as a numpy emulation of the block steps predicts: 4.9e-12);
  inverses at damping 1e-1: 2.8e-13 over the earlier cases; 9.1e-14, 4.3e-13, 9.5e-13 on the three large cells;
  synthetic SPD sizes 1 ... 97: 3.5e-15 (float64), 4.6e-8 (float32); float32 system on lih: 5.4e-8;
  preconditioner, float64 (lih, bcc_li, lih_mixed, bcc_li_333, graphene_331): out 3.6e-16, <P, V> 7.8e-16;
  preconditioner, float32 (lih, diamond; the products accumulate in float64): out 5.0e-8 and 5.2e-8, <P, V> 7.4e-16 and 8.4e-16;
  with float32 accumulators <P, V> had missed its budget on diamond (see test_precondition_vs_restatement);
  whole step on lih: 4.9e-11 of a leaf's largest entry."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import kfac_helpers as kh
import kfac_step_helpers as ks
from common import load_case
from deepsolid_amd import systems
from test_gpu_grad import dev_params, fresh_system, system_for

pytestmark = pytest.mark.gpu

DAMPINGS = [1e-3, 1e-1]
# the last three: orbital-head G of order 656 / 640 (20 block steps and an edge block of 16), 768 and 864 (27 block steps); their
# worst damped matrix at damping 1e-3 has condition 9.7e4, 3.6e5 and 5.2e5, where `assert_well_conditioned` still passes
INVERSE_CASES = [('lih', 5), ('lih_narrow', 3), ('lih_mixed', 3), ('bcc_li', 3), ('bcc_li_fulldet', 3),
                 ('bcc_li_333', 3), ('diamond', 3), ('graphene_331', 3)]


def rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def assert_well_conditioned(A, G, lam):
    """Two independent float64 inversions of each damped matrix agree to 1e-10 of the largest entry."""
    mats = ks.damped(A, G, lam)
    for m in mats or ():
        a = torch.linalg.inv(m)
        b = torch.cholesky_inverse(torch.linalg.cholesky(m))
        assert rel(a, b) <= 1e-10, 'the damped matrix is too ill-conditioned for a 1e-9 comparison'


@pytest.mark.parametrize('damping', DAMPINGS)
@pytest.mark.parametrize('name,batch', INVERSE_CASES)
def test_inverses_vs_restatement(name, batch, damping, record_property):
    """The library's own factors at a few synthetic walkers, through the moving average once (weight 1), inverted on the device
    and by the restatement.  bcc_li carries factors beyond 64 rows: several block steps and an edge block."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    x = torch.as_tensor(systems.synthetic_walkers(cell, batch, seed=91), device='cuda')
    flat, _ = sysd.kfac_factors(dev_params(params), x, flat=True)
    layout = sysd.kfac_layout()
    inv = sysd.kfac_inverses(flat, 1.0, damping)
    devs = []
    for b, (A, G), (Ai, Gi) in zip(layout, sysd.kfac_views(flat, layout), sysd.kfac_views(inv, layout)):
        lam = damping / b['repeats']
        A, G = A.double().cpu(), G.double().cpu()
        assert_well_conditioned(A, G, lam)
        ra, rg = ks.pi_adjusted_inverse(A, G, lam)
        assert torch.equal(Ai, Ai.T) and torch.equal(Gi, Gi.T)
        devs += [rel(Ai, ra), rel(Gi, rg)]
    record_property('inverse_dev', max(devs))
    print(f'{name} damping {damping:g}: worst inverse deviation {max(devs):.3e}')
    assert max(devs) <= 1e-9, devs
    again = sysd.kfac_inverses(flat, 1.0, damping)
    assert torch.equal(inv, again)                       # no atomics: two calls give the same bits


def spd(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    d = np.exp(rng.uniform(math.log(1e-3), 0.0, size=n))
    a = (q.T * d) @ q
    return (a + a.T) / 2


def sized_inverses(dtype, d_in, d_out, reps, flat, w, damping):
    from deepsolid_amd import _lib
    lib = _lib.load()
    nb = len(d_in)
    arr = C.c_int32 * nb
    di, do, rp = arr(*d_in), arr(*d_out), arr(*reps)
    need = int(lib.ds_kfac_inverses_sized_workspace_bytes(nb, di, do))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.empty_like(flat)
    _lib.check(lib.ds_kfac_inverses_sized(0 if dtype == torch.float64 else 1, nb, di, do, rp, C.c_void_p(flat.data_ptr()), float(w),
                                          float(damping), C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), need,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ds_kfac_inverses_sized')
    return out


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_inverses_on_synthetic_spd_matrices(dtype, record_property):
    """The same kernels on explicit sizes 1, 2, 31, 32, 33, 64, 65, 97 in ONE batched call (matrices finish at different block
    steps; one, two, three and four block steps; full and ragged edge blocks), Q^T D Q with eigenvalues in [1e-3, 1], a moving
    average weight other than 1, plus a zero factor for the I / sqrt(lambda) branch.  The sized entry applies the general formula
    at any size, which is what the restatement's `pi_adjusted_inverse` computes.  float32: the inputs are float32-exact and the
    elimination is float64, so only the final rounding separates the result from the float64 inverse of the same input:
    1e-6 of the largest entry (8 float32 ulp against half an ulp of rounding)."""
    rng = np.random.default_rng(7)
    d_in, d_out, reps = [1, 2, 31, 32, 5], [97, 65, 64, 33, 33], [1, 4, 16, 2, 3]
    w, damping = 1.0 + 0.95, 1e-3
    mats = []
    for b, (a, g) in enumerate(zip(d_in, d_out)):
        mats += [np.zeros((a, a)) if b == 4 else spd(rng, a) * w, spd(rng, g) * w]
    flat = torch.cat([torch.as_tensor(m).reshape(-1) for m in mats]).to(dtype).cuda()
    out = sized_inverses(dtype, d_in, d_out, reps, flat, w, damping)
    devs, off = [], 0
    host = flat.double().cpu()
    for b, (a, g) in enumerate(zip(d_in, d_out)):
        A = host[off:off + a * a].view(a, a) / w
        Ai = out[off:off + a * a].view(a, a); off += a * a
        G = host[off:off + g * g].view(g, g) / w
        Gi = out[off:off + g * g].view(g, g); off += g * g
        lam = damping / reps[b]
        assert_well_conditioned(A, G, lam)
        ra, rg = ks.pi_adjusted_inverse(A, G, lam)
        assert torch.equal(Ai, Ai.T) and torch.equal(Gi, Gi.T)
        devs += [rel(Ai, ra), rel(Gi, rg)]
        if b == 4:                                                        # the zero branch: diagonal matrices
            assert float((Ai - torch.diag(Ai.diagonal())).abs().max()) == 0.0 and float((Gi - torch.diag(Gi.diagonal())).abs().max()) == 0.0
    record_property('inverse_dev', max(devs))
    print(f'synthetic {dtype}: deviations {devs}')
    assert max(devs) <= (1e-9 if dtype == torch.float64 else 1e-6), devs
    assert torch.equal(out, sized_inverses(dtype, d_in, d_out, reps, flat, w, damping))


def test_inverses_float32_system(record_property):
    """A float32 system on `lih`: its own float32 factors, inverted in float64 on the device, against the float64 CPU inverse of
    the same float32 input: 1e-6 of the largest entry."""
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = fresh_system(cell, klist, net_kw, torch.float32)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 5, seed=91).astype(np.float32), device='cuda')
    flat, _ = sysd.kfac_factors(dev_params(params, torch.float32), x, flat=True)
    layout = sysd.kfac_layout()
    inv = sysd.kfac_inverses(flat, 1.0, 1e-3)
    assert inv.dtype == torch.float32
    devs = []
    for b, (A, G), (Ai, Gi) in zip(layout, sysd.kfac_views(flat, layout), sysd.kfac_views(inv, layout)):
        ra, rg = ks.pi_adjusted_inverse(A.double().cpu(), G.double().cpu(), 1e-3 / b['repeats'])
        assert torch.equal(Ai, Ai.T) and torch.equal(Gi, Gi.T)
        devs += [rel(Ai, ra), rel(Gi, rg)]
    record_property('inverse_dev_f32', max(devs))
    print('float32 inverse deviations', devs)
    assert max(devs) <= 1e-6, devs


@pytest.mark.parametrize('name,dtype', [('lih', torch.float64), ('bcc_li', torch.float64), ('lih_mixed', torch.float64),
                                        ('lih', torch.float32),
                                        # 21 to 27 column tiles of 32, and the ragged 16-column tile of 656
                                        ('bcc_li_333', torch.float64), ('graphene_331', torch.float64), ('diamond', torch.float32)])
def test_precondition_vs_restatement(name, dtype, record_property):
    """out_b = A^- v G^- / R and <out_b, v> with random v and the DEVICE's own inverses as input (inverse error does not compound).
    float32: the bound is what the restatement's own float32 run of the two products loses against its float64 run, times 4
    (the summation order differs), measured per block and recorded.
    bcc_li_333, graphene_331 and diamond bring 21 to 27 column tiles and the ragged 16-column tile of 656.
    Measured on an MI355X.  float64: out at most 3.6e-16, <P, V> at most 7.8e-16.  float32 (the kernel accumulates both products
    in float64 and sums <P, V> from the unrounded entries): out 5.0e-8 (lih) and 5.2e-8 (diamond) of budgets from 4.0e-7 up,
    <P, V> 7.4e-16 and 8.4e-16 of budgets from 1.8e-10 up.
    The (`diamond`, float32) case is why: with float32 accumulators `out` was inside its budget (1.9e-6 at worst) but <P, V> missed
    it on three of seven blocks --
        kernel  5.4e-9, 2.3e-10, 3.2e-9, 2.4e-8, 2.7e-8, 8.3e-10, 3.3e-9
        budget  1.4e-9, 1.9e-9,  1.7e-9, 3.8e-8, 1.1e-7, 9.9e-9,  1.8e-10      (4 x the restatement's float32 loss)
    -- because the float32 loss of that one number per block is the sum of the rounding errors, of either sign, of up to 213 000
    entries and moves by one to two decades with the summation order (tools/kfac_sq_spread.py: 4.1e-11 ... 3.3e-9 on one block
    over 12 orders on the CPU), so no float32 accumulation meets 4 x one draw reliably."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw) if dtype == torch.float64 else fresh_system(cell, klist, net_kw, dtype)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 3, seed=91).astype(np.float64 if dtype == torch.float64 else np.float32),
                        device='cuda')
    flat, _ = sysd.kfac_factors(dev_params(params, dtype), x, flat=True)
    layout = sysd.kfac_layout()
    inv = sysd.kfac_inverses(flat, 1.0, 1e-3)
    nv = sum(b['d_in'] * b['d_out'] for b in layout)
    v = torch.as_tensor(np.random.default_rng(3).normal(size=nv)).to(dtype).cuda()
    out, sq = sysd.kfac_precondition(inv, v)
    out2, sq2 = sysd.kfac_precondition(inv, v)
    assert torch.equal(out, out2) and torch.equal(sq, sq2) and sq.dtype == torch.float64
    off, devs, sdevs, budget = 0, [], [], []
    for i, (b, (Ai, Gi)) in enumerate(zip(layout, sysd.kfac_views(inv, layout))):
        n = b['d_in'] * b['d_out']
        vb = v[off:off + n].view(b['d_in'], b['d_out']).cpu()
        ob = out[off:off + n].view(b['d_in'], b['d_out']); off += n
        ref, dot = ks.precondition(Ai.cpu(), Gi.cpu(), vb, b['repeats'])
        devs.append(rel(ob, ref))
        sdevs.append(abs(float(sq[i]) - dot) / abs(dot))
        if dtype == torch.float32:
            r32, d32 = ks.precondition(Ai.cpu(), Gi.cpu(), vb, b['repeats'], dtype=torch.float32)
            budget.append((4 * rel(r32, ref), 4 * abs(d32 - dot) / abs(dot)))
    record_property('precondition_dev', max(devs))
    record_property('sq_norm_dev', max(sdevs))
    print(f'{name} {dtype}: out deviations {devs}\n  sq_norm deviations {sdevs}\n  float32 budget {budget}')
    if dtype == torch.float64:
        assert max(devs) <= 1e-9 and max(sdevs) <= 1e-9, (devs, sdevs)
    else:
        record_property('f32_budget', budget)
        for d, s, (bd, bs) in zip(devs, sdevs, budget):
            assert d <= bd and s <= bs, (d, bd, s, bs)


def numbered_tree(params):
    n = [1]

    def walk(o):
        if isinstance(o, dict):
            return {k: walk(o[k]) for k in sorted(o)}
        if isinstance(o, (list, tuple)):
            return [walk(v) for v in o]
        a = np.asarray(o)
        out = torch.arange(n[0], n[0] + a.size, dtype=torch.float64).reshape(a.shape)
        n[0] += a.size
        return out
    return walk(params)


@pytest.mark.parametrize('name', ['lih', 'lih_bias', 'lih_lastlayer', 'li_polarized', 'bcc_li_fulldet'])
def test_index_map(name):
    """Scatter v from a tree whose entries carry their own number: every tagged leaf lands in its block, row for row
    ([w.reshape(-1, d_out) ; b]) against `kfac_layout`; the diagonal set is exactly the untagged leaves (the envelope)."""
    fx, cell, klist, net_kw, params = load_case(name)
    sysd = system_for(cell, klist, net_kw)
    tree = numbered_tree(params)
    dp = {k: [{kk: vv.cuda() for kk, vv in d.items()} for d in v] for k, v in tree.items()}
    packed = sysd.pack_params(dp)
    idx = sysd.kfac_index(dp)
    v = packed.index_select(0, idx['v_src']).cpu()
    off = 0
    for b in sysd.kfac_layout():
        n = b['d_in'] * b['d_out']
        got = v[off:off + n].view(b['d_in'], b['d_out']); off += n
        assert torch.equal(got, ks.block_matrix(tree, b['kind'], b['index'])), (b['kind'], b['index'])
        assert ('b' in tree[b['kind']][b['index']]) == b['has_bias']
    assert off == v.numel()
    diag = packed.index_select(0, idx['diag_src']).cpu()
    want = torch.cat([e[k].reshape(-1) for e in tree['envelope'] for k in sorted(e)])
    assert torch.equal(diag, want)
    assert all(p[0] == 'envelope' for p in idx['diag_paths'])
    total = sum(t.numel() for t in ks.leaves(tree))
    assert idx['v_tree'].numel() + idx['diag_tree'].numel() == total == sum(idx['leaf_sizes'])
    both = torch.cat([idx['v_tree'], idx['diag_tree']]).cpu()
    assert torch.equal(both.sort().values, torch.arange(total))
    # the tree-flat positions are the numbers themselves (entry k carries k + 1)
    assert torch.equal(v, (idx['v_tree'].cpu() + 1).double())


def tree_of(flat, params):
    off = [0]

    def walk(o):
        if isinstance(o, dict):
            return {k: walk(o[k]) for k in sorted(o)}
        if isinstance(o, (list, tuple)):
            return [walk(v) for v in o]
        out = flat[off[0]:off[0] + o.numel()].view(o.shape)
        off[0] += o.numel()
        return out
    return walk(params)


def _lih_step_inputs(sysd, dp, cell, seed):
    x = torch.as_tensor(systems.synthetic_walkers(cell, 5, seed=seed), device='cuda')
    cot = torch.as_tensor(np.random.default_rng(seed).normal(size=(5, 2)) / 5, device='cuda')
    grad = sysd.logpsi_vjp(dp, x, cot)[0]
    flat, seed_grad = sysd.kfac_factors(dp, x, flat=True)
    return grad, flat, seed_grad


def test_whole_step_vs_restatement(record_property):
    """`lih`, B = 5, two steps of `kfac.step` against `kfac_step` of the restatement fed the device's factors and gradients: every
    leaf of delta within 1e-8 of its largest entry (three factors, each within 1e-9).  The second step runs on the parameters the
    first one moved, with a moving-average weight of 1.95.  With invert_every = 2 the odd step leaves the inverses untouched."""
    from deepsolid_amd import kfac
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    shapes = kh.block_shapes(params, cell.nelec)
    init, step = kfac.kfac(lambda t: 0.05 / (1 + t))
    init2, step2 = kfac.kfac(lambda t: 0.05 / (1 + t), invert_every=2)
    state, ref_state = init(dp), ks.init_state(shapes, params)
    worst = []
    for k in range(2):
        grad, flat, seed_grad = _lih_step_inputs(sysd, dp, cell, 31 + k)
        gtree, stree = sysd.unpack_grad(grad, dp), sysd.unpack_grad(seed_grad, dp)
        factors = [(A.clone(), G.clone()) for A, G in sysd.kfac_views(flat)]
        before = [t.clone() for t in ks.leaves(dp)]
        state, dp, delta = step(sysd, dp, state, grad, flat, seed_grad, 5)
        ref_state, rdelta = ks.kfac_step(ref_state, shapes, params, gtree, factors, stree, 5, 0.05 / (1 + k))
        dtree = tree_of(delta, dp)
        for s in shapes:
            worst.append(rel(ks.block_matrix(dtree, s[0], s[1]), rdelta[s[0]][s[1]]))
        for c, e in enumerate(rdelta['envelope']):
            worst += [rel(dtree['envelope'][c][kk], e[kk]) for kk in e]
        for old, new, d in zip(before, ks.leaves(dp), ks.leaves(dtree)):
            assert torch.equal(new, old + d)                             # the parameters moved by delta, in place
        assert state['count'] == k + 1 and abs(state['ema_weight'] - ref_state['ema_weight']) == 0.0
        assert torch.equal(state['velocities'], delta)
    record_property('delta_dev', max(worst))
    print('delta deviations', worst, 'c', ref_state['c'])
    assert max(worst) <= 1e-8, worst
    dp = dev_params(params)
    state = init2(dp)
    grad, flat, seed_grad = _lih_step_inputs(sysd, dp, cell, 31)
    state, dp, _ = step2(sysd, dp, state, grad, flat, seed_grad, 5)
    kept = state['inverses'].clone()
    grad, flat, seed_grad = _lih_step_inputs(sysd, dp, cell, 32)
    state, dp, _ = step2(sysd, dp, state, grad, flat, seed_grad, 5)
    assert torch.equal(state['inverses'], kept)
    grad, flat, seed_grad = _lih_step_inputs(sysd, dp, cell, 33)
    state, dp, _ = step2(sysd, dp, state, grad, flat, seed_grad, 5)
    assert not torch.equal(state['inverses'], kept)


def test_discarded_step_leaves_everything_untouched():
    """A step whose gradient carries a NaN, under check_nan: walkers, parameters and every state tensor bit-identical."""
    from deepsolid_amd import kfac, train
    fx, cell, klist, net_kw, params = load_case('lih')
    sysd = system_for(cell, klist, net_kw)
    dp = dev_params(params)
    opt = kfac.kfac(0.05)
    grad, flat, seed_grad = _lih_step_inputs(sysd, dp, cell, 31)
    state, dp, _ = opt[1](sysd, dp, opt[0](dp), grad, flat, seed_grad, 5)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 5, seed=40), device='cuda')
    poison = [True]

    def packed(p, data):
        g = sysd.logpsi_vjp(p, data, torch.full((5, 2), 0.1, dtype=torch.float64, device='cuda'))[0]
        if poison[0]:
            g = g.clone()
            g[7] = float('nan')
        aux = train.AuxiliaryLossData(variance=None, local_energy=None, imaginary=None, kinetic=None, ewald=None,
                                      n_nonfinite=torch.zeros((), device='cuda'))
        return (torch.ones((), dtype=torch.float64, device='cuda'), aux), g
    energy = types.SimpleNamespace(system=sysd, value_and_grad_packed=packed)
    mcmc = lambda p, data, key, width: (data + 0.01, torch.tensor(0.5))
    step = kfac.make_kfac_training_step(mcmc, energy, opt, check_nan=True)
    snap = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in state.items()}
    psnap = [t.clone() for t in ks.leaves(dp)]
    data, dp2, state2, loss, aux, pmove, direction = step(0, x, dp, state, None, 0.1)
    assert loss is None and aux is None and direction is None and data is x and state2 is state
    for k, v in snap.items():
        assert torch.equal(state[k], v) if isinstance(v, torch.Tensor) else state[k] == v, k
    assert all(torch.equal(a, b) for a, b in zip(psnap, ks.leaves(dp)))
    poison[0] = False                                                    # the same step without the NaN is kept
    data, dp2, state2, loss, aux, pmove, direction = step(1, x, dp, state, None, 0.1)
    assert loss is not None and state2['count'] == 2 and not torch.equal(data, x)
    assert not all(torch.equal(a, b) for a, b in zip(psnap, ks.leaves(dp)))


def _drivers():
    from deepsolid_amd import network as dnet
    fx, cell, klist, net_kw, params = load_case('lih')
    logdet = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 16, seed=4), device='cuda')
    return cell, slog, logdet, params, x


def test_run_training_kfac_rows_and_bitwise_resume(tmp_path):
    """run_training(optimizer='kfac') on `lih`, B = 16: finite energies in the usual row schema; two iterations, save, restore and
    two more give the parameters of four uninterrupted iterations to the bit (kernels and Philox are deterministic; the noise
    key is a generator that both runs draw from in the same order)."""
    from deepsolid_amd import checkpoint, inference
    cell, slog, logdet, params, x = _drivers()
    kw = dict(burn_in=0, mcmc_steps=4, move_width=0.1, optimizer='kfac', kfac={'damping': 1e-3, 'invert_every': 1})
    dp = dev_params(params)
    w0 = dp['single'][0]['w'].clone()
    _, p4, st4, _, rows = inference.run_training(slog, logdet, dp, x, cell, iterations=4, key=torch.Generator().manual_seed(5),
                                                 save_path=str(tmp_path / 'a'), **kw)
    assert len(rows) == 4 and all(set(r) == set(inference.TRAIN_SCHEMA) and np.isfinite(r['energy']) for r in rows)
    assert st4['count'] == 4 and not torch.equal(w0, p4['single'][0]['w'])
    lines = open(tmp_path / 'a' / 'train_stats.csv').read().strip().splitlines()
    assert lines[0] == 'step,energy,variance,pmove,imaginary,kinetic,ewald' and len(lines) == 5
    gen = torch.Generator().manual_seed(5)
    inference.run_training(slog, logdet, dev_params(params), x, cell, iterations=2, key=gen, save_path=str(tmp_path / 'b'), **kw)
    t, d, p, opt, w = checkpoint.restore(checkpoint.find_last_checkpoint(str(tmp_path / 'b')), batch_size=16)
    d, p, w = checkpoint.to_single_device(d, p, w)
    opt = checkpoint.opt_state_to_single_device(opt)
    assert t == 2 and opt['count'] == 2 and abs(opt['ema_weight'] - 1.95) < 1e-15
    _, p22, st22, _, rows2 = inference.run_training(slog, logdet, dev_params(p), torch.as_tensor(d, device='cuda'), cell, iterations=2,
                                                    key=gen, t_init=t, opt_state=opt, **{**kw, 'move_width': w})
    assert [r['step'] for r in rows2] == [2, 3] and st22['count'] == 4
    for a, b in zip(ks.leaves(p4), ks.leaves(p22)):
        assert torch.equal(a, b)
    for k in ('factors', 'diag', 'inverses', 'velocities'):
        assert torch.equal(st4[k], st22[k]), k
    assert [r['energy'] for r in rows[2:]] == [r['energy'] for r in rows2]


def test_adam_is_still_the_default_and_unchanged():
    from deepsolid_amd import inference
    cell, slog, logdet, params, x = _drivers()
    kw = dict(iterations=2, key=3, burn_in=2, mcmc_steps=4, learning_rate=1e-3)
    _, pa, sa, _, rows_a = inference.run_training(slog, logdet, dev_params(params), x, cell, **kw)
    _, pb, sb, _, rows_b = inference.run_training(slog, logdet, dev_params(params), x, cell, optimizer='adam', **kw)
    assert rows_a == rows_b and set(sa) == {'count', 'm', 'v'} == set(sb) and sa['count'] == 2
    assert all(torch.equal(a, b) for a, b in zip(ks.leaves(pa), ks.leaves(pb)))
    assert all(set(r) == set(inference.TRAIN_SCHEMA) and np.isfinite(r['energy']) for r in rows_a)
    with pytest.raises(ValueError, match='optimizer'):
        inference.run_training(slog, logdet, dev_params(params), x, cell, optimizer='sgd', **kw)
    with pytest.raises(NotImplementedError, match='momentum'):
        inference.run_training(slog, logdet, dev_params(params), x, cell, optimizer='kfac', kfac={'momentum': 0.5}, **kw)
