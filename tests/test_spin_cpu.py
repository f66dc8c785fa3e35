"""CPU checks of the total-spin estimator (csrc/ds_spin.h, `estimator.SpinSquared`): the exported symbols, the convention of
DESIGN.md section 17 on determinants of plane waves in the float64 oracle (a shared-k determinant is an eigenstate of S^2 with
s = |S_z|; the closed form of the exchange ratios for distinct k), and the host algebra of the accumulator on hand-made sums."""
import numpy as np
import pytest
import torch

import onebody_helpers as oh
import sampler_helpers as sh
import spin_helpers as sp


def test_library_exports_the_spin_exchange_symbols():
    from deepsolid_amd import _lib
    lib = _lib.load()
    for n in ('ds_spin_exchange_workspace_bytes', 'ds_spin_exchange_ratios'):
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert lib.ds_spin_exchange_workspace_bytes(None, 4, 4) == -1


def test_pair_order_and_swap():
    """Pair p = i n_dn + (j - n_up); the swap exchanges exactly the two positions and is an involution."""
    nelec = (3, 2)
    pr = sp.pairs(nelec)
    assert pr.tolist() == [[0, 3], [0, 4], [1, 3], [1, 4], [2, 3], [2, 4]]
    assert sp.pair_indices(8, nelec, 5).tolist() == [5, 0, 1, 2, 3, 4, 5, 0]
    x = np.random.default_rng(0).standard_normal((2, 15))
    xs = sp.swapped(x, nelec)
    assert xs.shape == (2, 6, 15)
    for p, (i, j) in enumerate(pr):
        want = x.reshape(2, 5, 3).copy()
        want[:, [i, j]] = want[:, [j, i]]
        np.testing.assert_array_equal(xs[:, p], want.reshape(2, 15))
        np.testing.assert_array_equal(sp.swapped(xs[:, p], nelec)[:, p], x)


# ------------------------------------------------------------------------------------------------ the convention, in the oracle
@pytest.mark.parametrize('which', ['lih', 'bcc_li', '2,1', '3,1', '1,2'])
def test_shared_k_plane_wave_determinant_is_a_spin_eigenstate(which):
    """Both channels occupy the same k points (the smaller a subset of the larger): summed over the electrons of the LARGER
    channel the exchange ratios give 1 for every electron of the smaller one, so t_w = min(n_up, n_dn) for every walker and
    <S^2> = s (s + 1) with s = |S_z|, walker by walker.  Bound 1e-12 (deviations seen: 1.4e-15 on lih, 8.8e-14 on bcc_li)."""
    from deepsolid_amd import estimator
    ref = sp.shared_reference(which)
    nu, nd = ref['nelec']
    B = len(ref['x'])
    q = ref['q_all'].reshape(B, nu, nd)
    assert np.all(np.isfinite(q))
    over_larger = q.sum(axis=1) if nu >= nd else q.sum(axis=2)
    print(f'{which}: max |sum over the larger channel - 1| = {np.abs(over_larger - 1).max():.3e}')
    assert np.abs(over_larger - 1).max() <= 1e-12
    t = q.sum(axis=(1, 2))
    assert np.abs(t - min(nu, nd)).max() <= 1e-12
    s = 0.5 * abs(nu - nd)
    acc = estimator.SpinSquared.from_state_dict({'nelec': np.asarray([nu, nd]), 'pairs_per_walker': nu * nd, 'n_walkers': B,
                                                 'sums': np.asarray([t.real.sum(), t.imag.sum(), (t.real ** 2).sum(), B]),
                                                 'n_bad': np.zeros(1, np.int64)})
    r = acc.spin_squared()
    assert abs(r['value'] - s * (s + 1)) <= 1e-12 and abs(r['imag']) <= 1e-12 and r['sz'] == 0.5 * (nu - nd)
    assert r['error'] <= 1e-12


def test_two_electrons_same_and_orthogonal_orbitals():
    """The two checks of the sign and of the n_dn term, from the closed form alone: one up and one down electron in the same
    plane wave give <S^2> = 0; in two different plane waves q = exp(i (k_u - k_d) . (r_j - r_i)), whose average over the cell
    vanishes, so <S^2> = S_z (S_z + 1) + n_dn - 0 = 1."""
    cell, klist = sp.small_cell((1, 1))
    from deepsolid_amd import estimator, systems
    kpts, _ = estimator.momentum_kpoints(cell, klist, 1)
    x = systems.synthetic_walkers(cell, 4, seed=3)
    same = sp.plane_wave_pair_ratios(x, (kpts[:1], kpts[:1]), (1, 1))
    np.testing.assert_allclose(same, 1.0, atol=1e-14)
    assert sp.spin_value((1, 1), 1, same.real.sum(), 4) == pytest.approx(0.0, abs=1e-13)
    # a uniform grid of the down electron over the cell averages the orthogonal pair to 0 exactly
    a = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    grid = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(3) / 3.0] * 3, indexing='ij')], axis=1) @ a
    xg = np.concatenate([np.broadcast_to(x[0, :3], (27, 3)), x[0, 3:6] + grid], axis=1)
    other = sp.plane_wave_pair_ratios(xg, (kpts[:1], kpts[1:2]), (1, 1))
    assert np.abs(np.abs(other) - 1).max() <= 1e-13
    assert sp.spin_value((1, 1), 1, other.real.sum(), 27) == pytest.approx(1.0, abs=1e-13)


@pytest.mark.parametrize('name', ['lih_twist', 'bcc_li'])
def test_distinct_k_closed_form_equals_the_oracle(name):
    """The plane-wave network of onebody_helpers (distinct k per spin): the oracle's exchange ratios equal the closed form per pair
    to 1e-10 max(1, |q|)."""
    fx, cell, klist, _, _ = sh.case(name)
    pw_klist, net_kw, params, _, _ = oh.plane_wave_case(cell, klist)
    nelec = tuple(int(v) for v in cell.nelec)
    x = np.asarray(fx['x'], dtype=np.float64)
    P = nelec[0] * nelec[1]
    q = sp.oracle_ratios(sh.Oracle(cell, pw_klist, net_kw, params), x, nelec, P, 0)
    want = sp.plane_wave_pair_ratios(x, pw_klist, nelec)
    err = np.abs(q - want) / np.maximum(1.0, np.abs(want))
    print(f'{name}: max scaled |q_oracle - q_closed| = {err.max():.3e}, |q| in [{np.abs(want).min():.3g}, {np.abs(want).max():.3g}]')
    assert np.all(np.isfinite(want)) and err.max() <= 1e-10


# ------------------------------------------------------------------------------------------------ host algebra of SpinSquared
def _accumulator(name='bcc_li', **kw):
    from deepsolid_amd import estimator, network
    _, cell, klist, net_kw, _ = sh.case(name)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    return estimator.SpinSquared(net, None, **kw)


def _fill(acc, t, n_bad=0, seen=None):
    t = np.asarray(t, dtype=np.complex128)
    acc.sums = torch.as_tensor(np.asarray([t.real.sum(), t.imag.sum(), (t.real ** 2).sum(), len(t)], dtype=np.float64))
    acc.n_bad = torch.as_tensor(np.asarray([n_bad], dtype=np.int64))
    acc.n_walkers = len(t) + n_bad if seen is None else seen


def test_spin_squared_host_algebra(tmp_path):
    from deepsolid_amd import estimator
    rng = np.random.default_rng(7)
    full = _accumulator()
    assert full.nelec == (12, 12) and full.n_pairs_total == 144 and full.pairs_per_walker == 144 and full.first_pair == 0
    acc = _accumulator(pairs_per_walker=12)
    assert acc.pairs_per_walker == 12
    with pytest.raises(ValueError):
        _accumulator(pairs_per_walker=0)
    t = rng.standard_normal(50) + 1j * rng.standard_normal(50)
    _fill(acc, t, n_bad=3)
    r = acc.spin_squared()
    scale = 144 / 12
    mean = t.real.mean()
    assert r['value'] == pytest.approx(0.0 + 12 - scale * mean, rel=1e-13)            # S_z = 0, n_dn = 12, P / M = 12
    assert r['error'] == pytest.approx(scale * np.sqrt(t.real.var(ddof=0) / 49), rel=1e-10)
    assert r['imag'] == pytest.approx(-scale * t.imag.mean(), rel=1e-13)
    assert (r['n_walkers'], r['n_bad'], r['sz']) == (53, 3, 0.0)
    # merge adds sums and counts; another setup is refused
    other = _accumulator(pairs_per_walker=12)
    t2 = rng.standard_normal(30) + 1j * rng.standard_normal(30)
    _fill(other, t2, n_bad=1)
    acc.merge(other)
    both = np.concatenate([t, t2])
    r = acc.spin_squared()
    assert r['value'] == pytest.approx(12 - scale * both.real.mean(), rel=1e-13)
    assert (r['n_walkers'], r['n_bad']) == (84, 4) and float(acc.sums[3]) == 80
    with pytest.raises(ValueError):
        acc.merge(full)
    # state_dict round trip into a fresh accumulator, save / load
    acc.first_pair = 36
    sd = acc.state_dict()
    for k in ('sums', 'n_bad', 'n_walkers', 'nelec', 'pairs_per_walker', 'first_pair', 'reduced'):
        assert k in sd, k
    fresh = _accumulator(pairs_per_walker=12)
    fresh.load_state_dict(sd)
    assert fresh.spin_squared() == acc.spin_squared() and fresh.first_pair == 36 and fresh.n_walkers == 84
    with pytest.raises(ValueError):
        full.load_state_dict(sd)
    path = tmp_path / 's2.npz'
    acc.save(path, results=True)
    with np.load(path) as f:
        assert float(f['value']) == acc.spin_squared()['value'] and float(f['error']) == acc.spin_squared()['error']
    loaded = estimator.SpinSquared.load(path)
    assert loaded.spin_squared() == acc.spin_squared() and loaded.first_pair == 36 and loaded.nelec == (12, 12)
    with pytest.raises(RuntimeError):
        loaded.update(torch.zeros(1, 72))                       # no network behind a loaded accumulator
    # reduce: the identity on one rank, refused twice, and no update afterwards
    before = acc.spin_squared()
    acc.reduce()
    assert acc.spin_squared() == before
    with pytest.raises(RuntimeError):
        acc.reduce()
    with pytest.raises(RuntimeError):
        acc.update(torch.zeros(1, 72))


def test_spin_squared_reduce_over_two_identical_ranks(monkeypatch):
    """`reduce` is one packed all-reduce of (sums, n_bad, n_walkers): with a collective that doubles its input (two ranks holding
    the same numbers) every count doubles and value, error-free quantities and imag stay what they were."""
    from deepsolid_amd import constants
    acc = _accumulator(pairs_per_walker=12)
    rng = np.random.default_rng(8)
    _fill(acc, rng.standard_normal(20) + 1j * rng.standard_normal(20), n_bad=2)
    before = acc.spin_squared()
    calls = []

    def doubled(t, axis_name=None):
        calls.append(tuple(t.shape))
        return 2 * t
    monkeypatch.setattr(constants, 'world_size', lambda: 2)
    monkeypatch.setattr(constants, 'psum_if_pmap', doubled)
    acc.reduce()
    assert calls == [(6,)]                                       # ONE collective of six numbers
    after = acc.spin_squared()
    assert after['value'] == before['value'] and after['imag'] == before['imag']
    assert (after['n_walkers'], after['n_bad']) == (2 * before['n_walkers'], 2 * before['n_bad']) and float(acc.sums[3]) == 40
    assert after['error'] == pytest.approx(before['error'] * np.sqrt(19 / 39), rel=1e-12)
    with pytest.raises(RuntimeError):
        acc.reduce()
    assert calls == [(6,)]


def test_spin_squared_without_opposite_spins():
    """li_polarized, nelec (3, 0): P = 0, nothing to sample.  `update` only counts walkers (it needs no device and makes no
    library call), value = S_z (S_z + 1) = 15/4 exactly, error 0."""
    acc = _accumulator('li_polarized')
    assert acc.nelec == (3, 0) and acc.n_pairs_total == 0
    acc.update(torch.zeros(7, 9))                                # CPU walkers: a library call would refuse them
    acc.update(torch.zeros(2, 9))
    r = acc.spin_squared()
    assert r == dict(value=3.75, error=0.0, imag=0.0, n_walkers=9, n_bad=0, sz=1.5)
    acc.reduce()
    assert acc.spin_squared()['value'] == 3.75
    # the formula keeps its n_dn term for the mirror image (0, 3): S_z = -3/2, S_z (S_z + 1) + n_dn = 15/4 as well
    from deepsolid_amd import estimator
    mirrored = estimator.SpinSquared.from_state_dict({'nelec': np.asarray([0, 3]), 'pairs_per_walker': 0, 'n_walkers': 4,
                                                      'sums': np.zeros(4), 'n_bad': np.zeros(1, np.int64)})
    assert mirrored.spin_squared()['value'] == 3.75 and mirrored.spin_squared()['sz'] == -1.5
