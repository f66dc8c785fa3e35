"""GPU tests of the Hartree-Fock orbital kernel (`ds_hf_orbitals`, csrc/ds_hf.h, deepsolid_amd/hf.py) and of the HF-density
pretraining (`pretrain_hartree_fock_usingHF`).  Everything is compared with the direct image sum of tests/hf_helpers.py, which
tests/test_hf_cpu.py holds to an independent reciprocal-space sum, at atol 1e-10 on matrices with entries of O(1): the bound the
project holds orbital matrices to (test_gpu_parity.py).  The objects under test sum over the helper's own translations
(truncated below 1e-16), so what is measured is the kernel's arithmetic, not the truncation.
Measured on the MI355X: largest deviation 7.2e-15 on the LiH-like cell (1055 images), 8.7e-14 on the hexagonal cell (405 images,
where 238 of 486 (electron, full chunk) pairs meet the skip rule, and the same with the 1607-image list, 1777 of 2025); first pretraining loss equal to the host formula in all 12
printed digits; 20 iterations of method 'hf' take the loss from 1.079 to 0.431 (pmove 0.94)."""
import functools

import numpy as np
import pytest
import torch

import hf_helpers as hh
from deepsolid_amd import systems
from pretrain_helpers import reference_loss

pytestmark = pytest.mark.gpu
ATOL = 1e-10


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device='cuda')


@functools.lru_cache(maxsize=None)
def lih_reference():
    """One walker set and one reference for all LiH-like tests: 67 walkers spread over +-2 cells."""
    s = hh.lih_system()
    x = hh.walkers(s, 67, seed=31, spread=2)
    return s, x, hh.orb_mats(s, x)


def check(mats, ref, rows=slice(None)):
    worst = 0.0
    for got, want in zip(mats, ref):
        want = want[rows]
        assert got.dtype == torch.complex128 and tuple(got.shape) == want.shape
        if want.size:
            worst = max(worst, float(np.abs(got.cpu().numpy() - want).max()))
    assert worst <= ATOL, worst
    return worst


@pytest.mark.parametrize('B', [16, 1, 67])
def test_lih_orbital_matrices(B):
    """LiH-like fcc primitive cell, 2 x 1 x 1 supercell: n_k = 2, nelec = (4, 4), 6 AOs (one column tile)."""
    s, x, ref = lih_reference()
    go = s.gaussian_orbitals()
    mats = go.eval_orb_mat(dev(x[:B]).reshape(B, -1, 3))
    assert float(np.abs(ref[0]).max()) > 0.5                      # entries of O(1)
    print(f'B = {B}: {go.images.shape[0]} images, max deviation {check(mats, ref, slice(0, B)):.3e}')


@pytest.mark.parametrize('nelec,wide', [((5, 4), False), ((3, 0), False), ((5, 4), True)])
def test_hexagonal_vacuum_cell(nelec, wide):
    """Two atoms, 20 Bohr of vacuum, s + p + d on either atom (18 AOs: two column tiles, the second ragged), n_k = 3 with a twist,
    a count of translations that 4 and 64 do not divide, walkers over +-3 cells; an empty spin channel is kept as (B, 0, 0).
    wide: translations out to 1.6 x the radius, sorted by length -- the kernel skips the far chunks (alpha_min |d|^2 > 90)."""
    s = hh.hex_system(nelec, wide)
    assert s.images.shape[0] % 4 and s.images.shape[0] % 64 and s.nao == 18
    x = hh.walkers(s, 9, seed=41, spread=3)
    go = s.gaussian_orbitals()
    # the kernel's rule, on the host: chunks of 64 images of the list as handed over, in its order, whose every image has
    # alpha_min |r - R - L|^2 > 90 for every atom, per wrapped electron position
    r = hh.wrap(s.a, x.reshape(-1, 3))[0]
    d2 = ((r[:, None, None, :] - s.atoms[None, None, :, :] - go.images[None, :, None, :]) ** 2).sum(-1).min(-1)      # (P, n_L)
    far = s.alpha_min * d2 > 90.0
    full = far.shape[1] // 64 * 64                               # the ragged last chunk is padded with L = 0 and never qualifies
    skipped = sum(int(far[:, c:c + 64].all(axis=1).sum()) for c in range(0, full, 64))
    assert skipped > 0 or not wide, skipped                      # the wide list IS cut for these walkers
    mats = go.eval_orb_mat(dev(x).reshape(9, -1, 3))
    assert [tuple(m.shape) for m in mats] == [(9, nelec[0], nelec[0]), (9, nelec[1], nelec[1])]
    print(f'nelec = {nelec}, {s.images.shape[0]} images, {skipped} (electron, chunk) pairs meet the skip rule: max deviation {check(mats, hh.orb_mats(s, x)):.3e}')


@pytest.mark.parametrize('n_d', [5, 13])
def test_wide_basis_tiles(n_d):
    """The other instantiations of the kernel: 5 (13) more d shells on the triclinic cell give 43 (83) AOs, i.e. four column tiles
    (eight, with 32-image chunks), and 9 k points take two k groups of the grid."""
    base = hh.pin_system('triclinic')
    shells = base.shells + [(i % 2, 2, np.array([0.3 + 0.1 * i]), hh._norm(2, [0.3 + 0.1 * i], [1.0])) for i in range(n_d)]
    recip = 2 * np.pi * np.linalg.inv(base.a).T
    kpts = np.array([[i / 3.0, j / 3.0, 0.2] for i in range(3) for j in range(3)]) @ recip
    s = hh.System(base.a, base.atoms, shells, kpts, [[1] * 9, [1, 0, 1, 0, 0, 1, 0, 0, 1]], seed=5)
    x = hh.walkers(s, 3, seed=6, spread=1)
    check(s.gaussian_orbitals().eval_orb_mat(dev(x).reshape(3, -1, 3)), hh.orb_mats(s, x))


def test_float32_walkers_are_widened_on_load():
    s, x, _ = lih_reference()
    go = s.gaussian_orbitals()
    x32 = dev(x[:16], torch.float32)
    got = go.eval_orb_mat(x32.reshape(16, -1, 3))
    same = go.eval_orb_mat(x32.to(torch.float64).reshape(16, -1, 3))
    for a, b in zip(got, same):
        assert float((a - b).abs().max()) <= ATOL
    check(got, hh.orb_mats(s, x32.cpu().numpy().astype(np.float64)))


def test_bit_identity_and_batch_independence():
    s, x, _ = lih_reference()
    go = s.gaussian_orbitals()
    xs = dev(x).reshape(67, -1, 3)
    a, b = go.eval_orb_mat(xs), go.eval_orb_mat(xs)
    assert all(torch.equal(torch.view_as_real(p), torch.view_as_real(q)) for p, q in zip(a, b))
    perm = torch.randperm(67, generator=torch.Generator().manual_seed(1)).cuda()
    c = go.eval_orb_mat(xs[perm].contiguous())
    d = go.eval_orb_mat(xs[40:45].contiguous())
    for sp in range(2):
        assert torch.equal(torch.view_as_real(c[sp]), torch.view_as_real(a[sp][perm]))
        assert torch.equal(torch.view_as_real(d[sp]), torch.view_as_real(a[sp][40:45]))


def test_eval_slogdet_and_value():
    for s in (hh.lih_system(), hh.hex_system((3, 0))):
        x = hh.walkers(s, 12, seed=17, spread=1)
        go = s.gaussian_orbitals()
        phase, logabs = go.eval_slogdet(dev(x).reshape(12, -1, 3))
        rp, rl = hh.slogdet(s, x)
        assert phase.is_cuda and logabs.dtype == torch.float64
        assert float(np.abs(logabs.cpu().numpy() - rl).max()) <= 1e-9
        assert float(np.abs(phase.cpu().numpy() - rp).max()) <= 1e-9
        psi = go(dev(x).reshape(12, -1, 3)).cpu().numpy()
        assert np.abs(psi - rp * np.exp(rl)).max() <= 1e-9 * np.abs(np.exp(rl)).max()


@functools.lru_cache(maxsize=None)
def lih_networks():
    from deepsolid_amd import network as dnet
    cell = hh.lih_cell()
    go = hh.lih_system().gaussian_orbitals()
    kw = dict(systems.DETNET_DEFAULTS)
    make = lambda m: dnet.make_solid_fermi_net(klist=go.klist, simulation_cell=cell, method_name=m, **kw)
    return cell, go, make('eval_mats'), make('eval_slogdet'), make('eval_logdet')


def host_loss(mats, params, x, targets):
    """pretrain.py:87-88 with the library's eval_mats and the helper's targets."""
    predict = [m.cpu() for m in mats.apply(params, dev(x))]
    return float(reference_loss(predict, [torch.as_tensor(t) for t in targets], False))


def test_hf_density_sampler_follows_the_replay():
    """`pretrain_hartree_fock_usingHF` with replayed noise, nsteps = 3, 2 iterations, B = 32: the final walkers and the accept
    count of every move equal the helper's replay; run move by move (the walk does not depend on the parameters), the walkers
    after each single move do, which is every walker's every decision (a differing decision moves a walker by ~ 0.02).  The seed
    leaves every decision decidable (test_hf_cpu.py); the loss of the first iteration equals the host formula at the replay's
    walkers."""
    from deepsolid_amd import pretrain
    cell, go, mats, _, _ = lih_networks()
    s = hh.lih_system()
    N = sum(s.nelec)
    normals, uniforms = hh.sampler_noise(hh.SAMPLER_SEED, N)
    x0 = hh.sampler_start(s, cell.a)
    trace = []
    x_ref, dec, margin = hh.replay_sampler(s, cell.a, x0, normals, uniforms, trace=trace)
    assert np.abs(margin).min() > hh.SAMPLER_MARGIN and dec.any() and (~dec).any()
    noise = (dev(normals), dev(uniforms))
    params = mats.init(0)
    x_it0 = trace[hh.SAMPLER_NSTEPS - 1]
    want_loss = host_loss(mats, params, x_it0, [t for t in hh.orb_mats(s, x_it0) if t.shape[-1]])
    hist = []
    p2, x = pretrain.pretrain_hartree_fock_usingHF(params, dev(x0), mats.apply, 0, cell, go, iterations=hh.SAMPLER_ITERATIONS,
                                                   nsteps=hh.SAMPLER_NSTEPS, history=hist, noise=noise)
    assert p2 is params and float(np.abs(x.cpu().numpy() - x_ref).max()) <= 1e-10
    assert [h['accepts'] for h in hist] == [[int(d.sum()) for d in it] for it in dec]
    assert all(abs(h['pmove'] - it[-1].sum() / hh.SAMPLER_BATCH) < 1e-15 for h, it in zip(hist, dec))
    assert abs(hist[0]['loss'] - want_loss) <= 1e-10 * want_loss
    assert abs(hist[-1]['logprob_target'] - float(np.mean(2 * hh.slogdet(s, x_ref)[1]))) <= 1e-8
    # move by move: every decision of every walker
    xd, prev, k = dev(x0), x0, 0
    for t in range(hh.SAMPLER_ITERATIONS):
        for i in range(hh.SAMPLER_NSTEPS):
            _, xd = pretrain.pretrain_hartree_fock_usingHF(params, xd, mats.apply, 0, cell, go, iterations=1, nsteps=1,
                                                           noise=(noise[0][t:t + 1, i:i + 1], noise[1][t:t + 1, i:i + 1]))
            got = xd.cpu().numpy()
            assert float(np.abs(got - trace[k]).max()) <= 1e-10, (t, i)
            moved = np.abs(got - prev).max(axis=1) > 0
            assert np.array_equal(moved, dec[t, i]), (t, i)
            prev, k = got, k + 1


def test_first_loss_and_hf_pretraining_lowers_the_loss():
    """`pretrain_hartree_fock` with GaussianOrbitals targets (the `on_device` hook): the loss of the first iteration equals the host
    formula with the helper's targets to 1e-10 relative.  Twenty iterations of method 'hf' lower the loss."""
    from deepsolid_amd import pretrain
    cell, go, mats, slog, _ = lih_networks()
    s = hh.lih_system()
    x0 = hh.sampler_start(s, cell.a)
    params = mats.init(0)
    want = host_loss(mats, params, x0, hh.orb_mats(s, x0))
    hist = []
    pretrain.pretrain_hartree_fock(params, dev(x0), slog.apply, mats.apply, 3, cell, go, iterations=1, history=hist)
    print(f'first loss {hist[0]["loss"]:.12g}, host formula {want:.12g}')
    assert abs(hist[0]['loss'] - want) <= 1e-10 * want
    params = mats.init(0)
    hist = []
    pretrain.pretrain_hartree_fock_usingHF(params, dev(x0), mats.apply, 3, cell, go, iterations=20, history=hist)
    losses = [h['loss'] for h in hist]
    print(f'method hf: loss {losses[0]:.6g} -> {losses[-1]:.6g}, pmove {hist[-1]["pmove"]:.2f}')
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert all(0.0 < h['pmove'] <= 1.0 and np.isfinite(h['logprob']) and np.isfinite(h['logprob_target']) for h in hist)


def test_run_training_pretrain_method_switch(tmp_path):
    from deepsolid_amd import inference
    cell, go, _, slog, logdet = lih_networks()
    params = logdet.init(0)
    w0 = params['orbital'][0]['w'].clone()
    data = dev(hh.sampler_start(hh.lih_system(), cell.a))
    kw = dict(iterations=1, key=3, burn_in=2, mcmc_steps=2, learning_rate=1e-3, save_path=str(tmp_path), pretrain_iterations=3)
    with pytest.raises(ValueError, match="needs scf_approx"):
        inference.run_training(slog, logdet, params, data, cell, pretrain_method='hf', **kw)
    with pytest.raises(ValueError, match="'net' or 'hf'"):
        inference.run_training(slog, logdet, params, data, cell, pretrain_method='scf', scf_approx=go, **kw)
    assert torch.equal(w0, params['orbital'][0]['w'])
    data, params, state, width, rows = inference.run_training(slog, logdet, params, data, cell, pretrain_method='hf',
                                                              pretrain_steps=2, scf_approx=go, **kw)
    assert len(rows) == 1 and np.isfinite(rows[0]['energy']) and not torch.equal(w0, params['orbital'][0]['w'])
