"""CPU checks of the one-body ratios / momentum distribution: the exported symbols, the numpy replay of the shift stream against
`ds_philox_host`, the k-point lists and the host algebra of `estimator.MomentumDistribution` on synthetic sums."""
import ctypes as C

import numpy as np
import pytest
import torch

import onebody_helpers as oh
import sampler_helpers as sh


def test_library_exports_the_one_body_symbols():
    from deepsolid_amd import _lib
    lib = _lib.load()
    for n in ('ds_one_body_workspace_bytes', 'ds_one_body_ratios'):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert lib.ds_one_body_workspace_bytes(None, 4, 4) == -1


def test_replayed_shift_blocks_equal_the_library_stream_3():
    from deepsolid_amd import _lib
    lib = _lib.load()
    seed, offset, B, M = 0x1234567890ABCDEF, (1 << 40) + 17, 5, 7
    A, Bk = oh.shift_blocks(seed, offset, B * M)
    out = (C.c_uint32 * 4)()
    for g in range(B * M):
        for blk, idx in ((A, 2 * g), (Bk, 2 * g + 1)):
            lib.ds_philox_host(seed, offset, 0, idx, 3, out)
            assert [int(v) for v in blk[:, g]] == [int(v) for v in out], (g, idx)
    # other streams and the neighbouring offset give other words
    lib.ds_philox_host(seed, offset, 0, 0, 2, out)
    assert [int(v) for v in A[:, 0]] != [int(v) for v in out]
    assert not np.array_equal(oh.shift_blocks(seed, offset + 1, 1)[0], A[:, :1])
    a = np.asarray(sh.case('bcc_li')[1].a, dtype=np.float64).reshape(3, 3)
    s, f = oh.replay_shifts(seed, offset, B, M, a)
    assert s.shape == (B, M, 3) and f.min() >= 0.0 and f.max() < 1.0
    np.testing.assert_allclose(s @ np.linalg.inv(a), f, atol=1e-14)           # the shifts lie in [0, 1) . a
    assert len(np.unique(f.reshape(-1))) == f.size


@pytest.mark.parametrize('name', ['lih_twist', 'bcc_li'])
def test_momentum_kpoints(name):
    from deepsolid_amd import estimator
    _, cell, klist, _, _ = sh.case(name)
    g = 2 * np.pi * np.linalg.inv(np.asarray(cell.a, dtype=np.float64).reshape(3, 3)).T
    kl = np.concatenate([np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in klist])
    for shells, count in ((0, 1), (1, 27), (2, 125)):
        k, n = estimator.momentum_kpoints(cell, klist, shells)
        assert k.shape == (count, 3) and n.shape == (count, 3) and n.dtype == np.int64
        assert not n[0].any() and np.array_equal(k[0], kl[0])
        assert len({tuple(v) for v in n}) == count and np.abs(n).max() == shells
        np.testing.assert_allclose(k - kl[0], n @ g, atol=1e-13)
        # ... and an integer combination of G_S from EVERY entry of the k list (they differ by supercell reciprocal vectors)
        for kt in kl:
            c = (k - kt) @ np.linalg.inv(g)
            np.testing.assert_allclose(c, np.round(c), atol=1e-9)
    with pytest.raises(ValueError):
        estimator.momentum_kpoints(cell, klist, 4)


def _accumulator(name='lih', **kw):
    from deepsolid_amd import estimator, network
    _, cell, klist, net_kw, _ = sh.case(name)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    return estimator.MomentumDistribution(net, None, **kw), cell


def _fill(acc, rng, samples, n_bad):
    acc.sums = torch.as_tensor(rng.standard_normal((2, len(acc.kpoints), 2)))
    acc.samples = np.asarray(samples, dtype=np.int64)
    acc.n_bad = torch.as_tensor(np.asarray(n_bad, dtype=np.int64))


def test_momentum_distribution_host_algebra(tmp_path):
    from deepsolid_amd import estimator
    rng = np.random.default_rng(3)
    acc, cell = _accumulator()
    assert acc.samples_per_walker == 4 and acc.kpoints.shape == (27, 3) and acc.nelec == (2, 2)
    _fill(acc, rng, (1000, 1200), (10, 0))
    s = acc.sums.numpy()
    nk = acc.momentum_distribution()
    assert nk.shape == (2, 27) and nk.dtype == np.complex128
    np.testing.assert_allclose(nk[0], 2 * (s[0, :, 0] + 1j * s[0, :, 1]) / 990, rtol=1e-15)      # bad samples removed
    np.testing.assert_allclose(nk[1], 2 * (s[1, :, 0] + 1j * s[1, :, 1]) / 1200, rtol=1e-15)
    # merge adds sums and counts
    other, _ = _accumulator()
    _fill(other, rng, (500, 300), (1, 2))
    want = s + other.sums.numpy()
    acc.merge(other)
    np.testing.assert_array_equal(acc.sums.numpy(), want)
    assert acc.samples.tolist() == [1500, 1500] and acc.n_bad.tolist() == [11, 2]
    # state_dict round trip into a fresh accumulator, and save / load
    acc.offset, acc.first_electron = 9, 3
    sd = acc.state_dict()
    for k in ('sums', 'samples', 'n_bad', 'kpoints', 'k_int', 'nelec'):
        assert k in sd, k
    fresh, _ = _accumulator()
    fresh.load_state_dict(sd)
    np.testing.assert_array_equal(fresh.sums.numpy(), acc.sums.numpy())
    assert fresh.samples.tolist() == [1500, 1500] and fresh.n_bad.tolist() == [11, 2] and (fresh.offset, fresh.first_electron) == (9, 3)
    np.testing.assert_array_equal(fresh.momentum_distribution(), acc.momentum_distribution())
    path = tmp_path / 'nk.npz'
    acc.save(path, results=True)
    with np.load(path) as f:
        np.testing.assert_array_equal(f['n_k'], acc.momentum_distribution())
        np.testing.assert_array_equal(f['k_int'], acc.k_int)
    loaded = estimator.MomentumDistribution.load(path)
    np.testing.assert_array_equal(loaded.momentum_distribution(), acc.momentum_distribution())
    np.testing.assert_array_equal(loaded.kpoints, acc.kpoints)
    with pytest.raises(RuntimeError):
        loaded.update(torch.zeros(1, 12))                       # no network behind a loaded accumulator
    # another k list: merge and load_state_dict refuse
    wide, _ = _accumulator(shells=2)
    with pytest.raises(ValueError):
        acc.merge(wide)
    with pytest.raises(ValueError):
        wide.load_state_dict(sd)
    # reduce: the identity on one rank, refused twice
    before = acc.sums.numpy().copy()
    acc.reduce()
    np.testing.assert_array_equal(acc.sums.numpy(), before)
    with pytest.raises(RuntimeError):
        acc.reduce()


def test_momentum_distribution_empty_spin_channel_and_no_samples():
    acc, _ = _accumulator('li_polarized')
    assert acc.nelec == (3, 0) and acc.samples_per_walker == 3
    _fill(acc, np.random.default_rng(4), (90, 0), (0, 0))
    nk = acc.momentum_distribution()
    assert np.all(nk[1] == 0) and np.all(np.isfinite(nk[0]))
    acc.samples[:] = 0
    assert np.all(np.isnan(acc.momentum_distribution()[0]))
