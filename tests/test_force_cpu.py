"""CPU checks of the ionic forces (csrc/ds_force.h, `ewaldsum.ion_ion_forces`, `estimator.IonForces`): the
references of force_helpers.py against finite differences of the oracle's Ewald energy, the host ion-ion force, the closed form
of the zero-variance term against autograd, the exported symbols, and the host logic of the accumulator on hand-made sums."""
import os
import re

import numpy as np
import pytest
import torch

import force_helpers as fh
from common import load_case
from oracle import ewaldsum as oew

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. helper HF force vs finite differences
@pytest.mark.parametrize('name', ['lih', 'graphene_hex'])
def test_helper_hf_force_vs_finite_differences(name):
    """-d(E_ei + E_ii)/dR_a from autograd against central differences of `EwaldSum.energy` on cells with one atom displaced by
    +-h, h = 1e-4 bohr, for two walkers whose electrons all stay 0.3 bohr away from every ion.  Tolerance 1e-6 max(1, |F|): the
    truncation error h^2 |E'''| / 6 is about 1e-7 and the round-off eps E / h about 1e-11."""
    _, cell, _, _, _ = load_case(name)
    ew = fh.ewald(cell)
    x = fh.spread_walkers(cell, ew, 2, seed=5)
    assert fh.min_ion_distance(ew, x).min() > 0.3
    xt = torch.as_tensor(x)
    # the rebuilt energies are the oracle's at zero displacement
    for b in range(2):
        ei, ii = fh.energies_from_atoms(ew, ew.atom_coords, xt[b])
        _, ei_ref, ii_ref = ew.energy(xt[b])
        assert abs(float(ei) - float(ei_ref)) <= 1e-12 * max(1.0, abs(float(ei_ref)))
        assert abs(float(ii) - float(ii_ref)) <= 1e-12 * max(1.0, abs(float(ii_ref)))
    F = fh.hf_force(ew, x)
    assert np.isfinite(F).all()
    h = 1e-4
    atoms = np.asarray(cell.atom_coords(), np.float64)
    worst = 0.0
    for a in range(len(atoms)):
        for k in range(3):
            e = []
            for sgn in (+1, -1):
                moved = atoms.copy()
                moved[a, k] += sgn * h
                # (the G points depend on the lattice alone; they all lie within |n| <= 100, so the smaller scan selects the same
                #  ones eight times faster: checked by their number)
                ews = oew.EwaldSum(fh.ShiftedCell(cell, moved), ewald_gmax=100)
                assert len(ews.gweight) == len(ew.gweight)
                e.append([float(ews.energy(xt[b])[1] + ews.energy(xt[b])[2]) for b in range(2)])
            fd = -(np.array(e[0]) - np.array(e[1])) / (2 * h)
            err = np.abs(fd - F[:, a, k]) / np.maximum(1.0, np.abs(F[:, a, k]))
            worst = max(worst, err.max())
    print(f'{name}: max scaled |F(autograd) - F(finite differences)| = {worst:.3e} (tolerance 1e-6)')
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------------ 2. the host ion-ion force
@pytest.mark.parametrize('name', ['lih', 'graphene_hex', 'lih_2x1x1', 'li_polarized', 'lih_displaced', 'graphene_hex_displaced'])
def test_ion_ion_forces_vs_helper(name):
    """`ewaldsum.ion_ion_forces` against the helper's autograd of the ion-ion energy, 1e-10; the sum over the ions vanishes; one
    atom alone feels nothing.  The forces of the perfect crystals vanish by symmetry, so the displaced cells (the last atom moved by
    (0.3, -0.2, 0.1) bohr) are the ones that check signs and magnitudes."""
    from deepsolid_amd import ewaldsum
    _, cell, _, _, _ = load_case(name.replace('_displaced', ''))
    if name.endswith('_displaced'):
        moved = np.asarray(cell.atom_coords(), np.float64).copy()
        moved[-1] += [0.3, -0.2, 0.1]
        cell = fh.ShiftedCell(cell, moved)
    ew = fh.ewald(cell)
    x = fh.spread_walkers(cell, ew, 1, seed=1)
    _, f_ii = fh.hf_parts(ew, x)
    got = ewaldsum.ion_ion_forces(cell)
    assert got.shape == f_ii.shape == (len(cell.atom_charges()), 3) and got.dtype == np.float64
    print(f'{name}: max |F_ii - helper| = {np.abs(got - f_ii).max():.3e}, |sum_a F_ii| = {np.abs(got.sum(axis=0)).max():.3e}')
    assert np.abs(got - f_ii).max() <= 1e-10
    assert np.abs(got.sum(axis=0)).max() <= 1e-10
    if name == 'li_polarized':
        assert got.shape[0] == 1 and np.abs(got).max() <= 1e-10
    if name.endswith('_displaced'):
        assert np.abs(f_ii).max() > 1e-2


# ------------------------------------------------------------------------------------------------ 3. closed form vs autograd
@pytest.mark.parametrize('name', ['h2', 'lih', 'li_polarized'])
def test_zero_variance_closed_form_vs_autograd(name):
    """The closed form of dF against -1/2 lap Q - grad Q . d from autograd, 1e-10 relative, with the first electron of walker 0 at
    r = 0.9 r_c from ion 0 and the second one beyond r_c of every ion where the cell has room (checked below), and a random drift."""
    from deepsolid_amd import estimator
    _, cell, _, _, _ = load_case(name)
    ew = fh.ewald(cell)
    r_c = estimator.wigner_seitz_radius(cell.lattice_vectors()) * (0.6 if name == 'lih' else 1.0)
    rng = np.random.default_rng(3)
    x = fh.spread_walkers(cell, ew, 2, seed=7).reshape(2, -1, 3)
    atoms = np.asarray(cell.atom_coords(), np.float64)
    u = rng.standard_normal(3)
    x[0, 0] = atoms[0] + 0.9 * r_c * u / np.linalg.norm(u)
    # an electron beyond the cutoff of every ion: scan the cell for such a point
    for _ in range(10000):
        p = rng.uniform(size=3) @ np.asarray(cell.lattice_vectors())
        xx = x[0].copy()
        xx[1] = p
        v = fh.nearest_image(ew, torch.as_tensor(xx.reshape(-1))).numpy()
        if np.linalg.norm(v[1], axis=-1).min() > r_c:
            x[0, 1] = p
            break
    x = x.reshape(2, -1)
    v = fh.nearest_image(ew, torch.as_tensor(x[0])).numpy()
    r = np.linalg.norm(v, axis=-1)
    assert abs(r[0, 0] - 0.9 * r_c) <= 1e-12 * r_c and r[1].min() > r_c
    d = rng.standard_normal(x.shape)
    auto = fh.zv_delta_autograd(ew, x, d, r_c)
    closed = fh.zv_delta_closed(ew, x, d, r_c)
    scale = np.maximum(np.abs(auto), np.abs(auto).max())
    print(f'{name}: max relative |closed - autograd| = {(np.abs(closed - auto) / scale).max():.3e}, max |dF| = {np.abs(auto).max():.3e}')
    assert np.abs(auto).max() > 1e-3
    assert (np.abs(closed - auto) / scale).max() <= 1e-10


# ------------------------------------------------------------------------------------------------ 3b. the image of the zero-variance term
@pytest.mark.parametrize('name', ['bcc_li', 'li_polarized', 'lih', 'lih_fcc', 'graphene_hex', 'h2'])
def test_zero_variance_image_is_the_true_nearest_one(name):
    """Q_a must be a periodic, continuous function of r_i: inside r_c <= the Wigner-Seitz radius the image it uses has to be the true
    nearest one.  The handle's minimal image is not: on the bcc cells the lattice takes the fractional wrap (dist_mode 1), which is
    the nearest image only within half the smallest plane spacing (bcc_li: 4.58 bohr, Wigner-Seitz radius 5.61), and in dist_mode 2
    it looks one cell around the raw difference, which the fixture walkers outside the cell defeat.  The kernel's own rule
    (`force_helpers.kernel_zv_image`: fractional wrap, then the nearest of the 27 images around it) is checked against brute force
    over the lattice vectors with coefficients in -5..5 on 1500 points uniform in a box of three cells per ion, 200 points within
    the Wigner-Seitz radius of an image of ion 0 and the fixture walkers, for every pair closer than the Wigner-Seitz radius."""
    from deepsolid_amd import distance, estimator
    from deepsolid_amd.ewaldsum import EwaldTables
    fx, cell, _, _, _ = load_case(name)
    t = EwaldTables(cell)
    r_ws = estimator.wigner_seitz_radius(t.latvec)
    assert r_ws < estimator.plane_spacings(t.latvec).min()          # the entry condition of the search (csrc/ds_force.h)
    rng = np.random.default_rng(9)
    close = rng.standard_normal((200, 3))
    close = t.atom_coords[0] + r_ws * rng.uniform(size=(200, 1)) * close / np.linalg.norm(close, axis=1, keepdims=True)
    pts = np.concatenate([rng.uniform(-1.0, 2.0, size=(1500, 3)) @ t.latvec, close + rng.integers(-2, 3, size=(200, 3)) @ t.latvec,
                          np.asarray(fx['x'], np.float64).reshape(-1, 3)])
    n = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(-5, 6)] * 3, indexing='ij')], axis=1) @ t.latvec
    checked = mi_differs = 0
    for R in t.atom_coords:
        for p in pts:
            cand = (p - R)[None, :] + n
            true = cand[np.argmin((cand ** 2).sum(axis=1))]
            if np.linalg.norm(true) >= r_ws:
                continue
            checked += 1
            assert np.abs(fh.kernel_zv_image(t.latvec, p - R) - true).max() <= 1e-11
            mi_differs += np.abs(distance.minimal_image_host(t.latvec, t.dist_mode, p - R) - true).max() > 1e-9
    print(f'{name}: dist_mode {t.dist_mode}, {checked} pairs inside r_ws = {r_ws:.3f}, the minimal image is not the nearest for {mi_differs}')
    assert checked >= 200
    if name in ('bcc_li', 'li_polarized'):
        assert mi_differs > 0


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def _declared():
    src = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\b(ds_[a-z0-9_]+)\s*\(', src))


def test_library_exports_the_force_symbols():
    from deepsolid_amd import _lib
    lib = _lib.load()
    for n in ('ds_ion_forces', 'ds_ion_forces_workspace_bytes'):
        assert n in _declared(), f'{n} is not declared in include/deepsolid_hip.h'
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert lib.ds_ion_forces_workspace_bytes(None, 4) == -1
    # refused before anything touches a device: a null handle
    rc = lib.ds_ion_forces(None, None, None, 4, 1.0, None, None, None, None, None, None, 0, None)
    assert rc != 0 and b'null' in lib.ds_last_error()


# ------------------------------------------------------------------------------------------------ 5. the accumulator on the host
class _Net:
    """What `IonForces` reads of a network before the first update."""

    def __init__(self, cell):
        self.simulation_cell = cell


def _accumulator(cutoff=None, **kw):
    from deepsolid_amd import estimator
    _, cell, _, _, _ = load_case('lih')
    return estimator.IonForces(_Net(cell), None, cutoff=cutoff, **kw), cell


def test_ion_forces_refusals():
    from deepsolid_amd import estimator
    acc, cell = _accumulator()
    r_ws = estimator.wigner_seitz_radius(cell.a)
    assert acc.cutoff == r_ws and acc.n_atoms == 2 and acc.sums.shape == (25,)
    assert _accumulator(cutoff=0.5 * r_ws)[0].cutoff == 0.5 * r_ws
    for bad in (0.0, -1.0, 1.01 * r_ws, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='cutoff'):
            _accumulator(cutoff=bad)
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        _accumulator(pseudopotential=object())
    with pytest.raises(ValueError, match='coordinates'):
        acc.update(torch.zeros(2, 9))


def test_ion_forces_host_algebra(tmp_path, monkeypatch):
    from deepsolid_amd import constants, estimator
    acc, cell = _accumulator()
    rng = np.random.default_rng(0)
    f_hf, f_zv = rng.standard_normal((7, 2, 3)), rng.standard_normal((7, 2, 3))
    acc.sums = torch.as_tensor(fh.sums_model(np.zeros(25), f_hf, f_zv))
    acc.n_walkers, acc.n_bad = 9, torch.tensor([2])
    r = acc.forces()
    assert set(r) == {'hf', 'hf_error', 'zv', 'zv_error', 'n_walkers', 'n_bad', 'atoms', 'cutoff'}
    np.testing.assert_allclose(r['hf'], f_hf.mean(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(r['zv'], f_zv.mean(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(r['hf_error'], f_hf.std(axis=0, ddof=0) / np.sqrt(6), rtol=1e-12)
    np.testing.assert_allclose(r['zv_error'], f_zv.std(axis=0, ddof=0) / np.sqrt(6), rtol=1e-12)
    assert r['n_walkers'] == 9 and r['n_bad'] == 2 and r['cutoff'] == acc.cutoff
    np.testing.assert_array_equal(r['atoms'], np.asarray(cell.atom_coords()))
    # no good walker: NaN; one: no error
    empty, _ = _accumulator()
    assert np.isnan(empty.forces()['hf']).all() and np.isnan(empty.forces()['zv_error']).all()
    one, _ = _accumulator()
    one.sums = torch.as_tensor(fh.sums_model(np.zeros(25), f_hf[:1], f_zv[:1]))
    assert np.array_equal(one.forces()['zv'], f_zv[0]) and np.isnan(one.forces()['hf_error']).all()
    # state_dict round trip, save / load, load_state_dict
    sd = acc.state_dict()
    fresh = estimator.IonForces.from_state_dict(sd)
    assert fresh.apply is None and fresh.n_walkers == 9 and not fresh.reduced
    for k in ('hf', 'hf_error', 'zv', 'zv_error'):
        np.testing.assert_array_equal(fresh.forces()[k], r[k])
    with pytest.raises(RuntimeError, match='no network'):
        fresh.update(torch.zeros(1, 12))
    path = str(tmp_path / 'forces.npz')
    acc.save(path)
    with np.load(path) as f:
        np.testing.assert_array_equal(f['zv'], r['zv'])
        np.testing.assert_array_equal(f['hf_error'], r['hf_error'])
    loaded = estimator.IonForces.load(path)
    np.testing.assert_array_equal(loaded.forces()['zv'], r['zv'])
    assert loaded.cutoff == acc.cutoff and loaded.n_walkers == 9 and int(loaded.n_bad) == 2
    other, _ = _accumulator()
    other.load_state_dict(sd)
    np.testing.assert_array_equal(other.forces()['hf'], r['hf'])
    with pytest.raises(ValueError, match='cutoff'):
        _accumulator(cutoff=0.5 * acc.cutoff)[0].load_state_dict(sd)
    # merge: sums, counts and walkers add; another cutoff is refused
    before = acc.sums.clone()
    acc.merge(loaded)
    assert torch.equal(acc.sums, 2 * before) and acc.n_walkers == 18 and int(acc.n_bad) == 4
    np.testing.assert_allclose(acc.forces()['zv'], r['zv'], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='differ'):
        acc.merge(_accumulator(cutoff=0.5 * acc.cutoff)[0])
    # reduce: once; afterwards no update; a reduced and a rank-local side do not merge on several ranks
    acc.reduce()
    assert acc.reduced and torch.equal(acc.sums, 2 * before)
    with pytest.raises(RuntimeError, match='already'):
        acc.reduce()
    with pytest.raises(RuntimeError, match='reduce'):
        acc.update(torch.zeros(1, 12))
    monkeypatch.setattr(constants, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='rank-local'):
        acc.merge(loaded)


def test_ion_forces_reduce_over_two_identical_ranks(monkeypatch):
    """ONE packed all-reduce of 12 A + 3 numbers: with two ranks holding the same sums everything doubles and the means stay."""
    from deepsolid_amd import constants
    acc, _ = _accumulator()
    rng = np.random.default_rng(1)
    acc.sums = torch.as_tensor(fh.sums_model(np.zeros(25), rng.standard_normal((5, 2, 3)), rng.standard_normal((5, 2, 3))))
    acc.n_walkers, acc.n_bad = 6, torch.tensor([1])
    before = acc.forces()
    calls = []
    monkeypatch.setattr(constants, 'world_size', lambda: 2)
    monkeypatch.setattr(constants, 'psum_if_pmap', lambda t: (calls.append(tuple(t.shape)), 2 * t)[1])
    acc.reduce()
    assert calls == [(27,)]
    after = acc.forces()
    assert after['n_walkers'] == 12 and after['n_bad'] == 2 and float(acc.sums[24]) == 10.0
    np.testing.assert_allclose(after['zv'], before['zv'], rtol=0, atol=1e-15)
