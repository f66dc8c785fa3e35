"""CPU tests of the pseudopotential forces (csrc/ds_ecp_force.h): the numpy model of ecp_force_helpers.py
against central differences of the ENERGY model of ecp_helpers.py in the ion positions, the exported symbols, and the host algebra of
`estimator.PseudopotentialForces`."""
import os

import numpy as np
import pytest
import torch

import ecp_force_helpers as fh
import ecp_helpers as eh
import force_helpers
from common import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the model against differences
@pytest.mark.parametrize('name,n_quad', [('lih', 12), ('lih_twist', 12), ('li_polarized', 12), ('lih', 6)])
def test_force_model_equals_central_differences_of_the_energy_model(name, n_quad):
    """-(E(R_I + h) - E(R_I - h)) / 2h of E_loc + E_nl (local_energy, weights, energy of ecp_helpers; oracle psi untouched, the same
    explicit rotations) against F^loc + F^nl of the force model, per walker, ion and axis, real and imaginary part together.
    h = 1e-4 Bohr; the tolerance is the h^2 truncation term of the difference itself: four times its Richardson estimate
    |D(2h) - D(h)| / 3.  No pair can enter or leave (asserted in the helper).  Measured: |error| / tolerance = 0.25 throughout (the
    error IS the truncation term), largest error 1.0e-6 at forces up to 7.9 Ha/Bohr."""
    ref = fh.reference(name, n_quad)
    d = fh.energy_differences(name, n_quad)
    f = ref['f_loc'] + ref['f_nl']
    err = np.abs(f - d['d1'])
    counts = np.asarray(eh.CASES[name][1])
    print(f'{name}, N_q = {n_quad}: max |F - D(h)| = {err.max():.3e}, max |F| = {np.abs(f).max():.3f}, '
          f'largest error / tolerance = {np.max(err[d["bound"] > 0] / d["bound"][d["bound"] > 0]):.3f}')
    assert np.abs(f).max() > 1.0 and np.abs(ref['f_nl']).max() > 0.1 and np.abs(ref['f_loc']).max() > 0.1
    assert np.all(err <= d['bound'])
    if name != 'lih':
        assert (counts == 0).any()                                                # a walker without pairs: F^nl exactly 0
    assert np.all(ref['f_nl'][counts == 0] == 0)
    if name == 'lih_twist':
        assert np.abs(ref['f_nl'].imag).max() > 1e-3                              # complex psi: the imaginary part is really there


def test_radial_derivative_equals_differences_of_the_radial_function():
    """v'(r) of every table of the synthetic species (n_k = 0..4 all occur) against central differences of ecp_helpers.radial."""
    r = np.linspace(0.3, 2.5, 23)
    h = 1e-5
    for sp in (eh.SPECIES_A, eh.SPECIES_B):
        for terms in [sp['local']] + sp['channels']:
            d1 = (eh.radial(terms, r + h) - eh.radial(terms, r - h)) / (2 * h)
            d2 = (eh.radial(terms, r + 2 * h) - eh.radial(terms, r - 2 * h)) / (4 * h)
            scale = fh.radial_deriv_terms(terms, r)[1].sum(axis=0)
            assert np.all(np.abs(fh.radial_deriv(terms, r) - d1) <= 4 * np.abs(d2 - d1) / 3 + 8 * eh.EPS * scale / h)
    assert {int(n) for sp in (eh.SPECIES_A, eh.SPECIES_B) for t in [sp['local']] + sp['channels'] for n, _, _ in t} == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ 2. symbols
def test_header_and_library_have_the_force_symbols():
    from deepsolid_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    lib = _lib.load()
    for n in ('ds_ecp_forces_workspace_bytes', 'ds_ecp_forces'):
        assert n + '(' in header, n
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert lib.ds_ecp_forces_workspace_bytes(None, None, 4, 4) == -1
    # refused before anything touches a device: a null handle
    rc = lib.ds_ecp_forces(None, None, None, None, 4, 0, 0, None, 4, None, None, None, None, None, None, None, 0, None)
    assert rc != 0 and b'null' in lib.ds_last_error()


# ------------------------------------------------------------------------------------------------ 3. the accumulator on the host
class _Net:
    """What `PseudopotentialForces` reads of a network before the first update."""

    def __init__(self, cell):
        self.simulation_cell = cell


def _accumulator(n_quad=12, key=0):
    from deepsolid_amd import estimator
    _, cell, _, _, _ = load_case('lih')
    ecp = eh.make_ecp(cell, eh.CASES['lih'][0], n_quad)
    return estimator.PseudopotentialForces(_Net(cell), None, ecp, key=key), cell, ecp


def test_pseudopotential_forces_refusals():
    from deepsolid_amd import estimator
    acc, cell, ecp = _accumulator(key=5)
    assert acc.n_atoms == 2 and acc.sums.shape == (25,) and acc.seed == 5 and acc.offset == 0
    with pytest.raises(ValueError, match='needs a pseudopotential'):
        estimator.PseudopotentialForces(_Net(cell), None, None)
    _, other, _, _, _ = load_case('bcc_li')
    with pytest.raises(ValueError, match='another simulation cell'):
        estimator.PseudopotentialForces(_Net(other), None, ecp)
    with pytest.raises(ValueError, match='coordinates'):
        acc.update(torch.zeros(2, 9))
    # the all-electron accumulator still refuses a pseudopotential
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        estimator.IonForces(_Net(cell), None, pseudopotential=ecp)


def test_pseudopotential_forces_host_algebra(tmp_path, monkeypatch):
    from deepsolid_amd import constants, estimator
    acc, cell, _ = _accumulator()
    rng = np.random.default_rng(0)
    f_pp, f_tot = rng.standard_normal((7, 2, 3)), rng.standard_normal((7, 2, 3))
    acc.sums = torch.as_tensor(force_helpers.sums_model(np.zeros(25), f_pp, f_tot))
    acc.n_walkers, acc.n_bad, acc.offset = 9, torch.tensor([2]), 3
    r = acc.forces()
    assert set(r) == {'pp', 'pp_error', 'total', 'total_error', 'n_walkers', 'n_bad', 'atoms'}
    np.testing.assert_allclose(r['pp'], f_pp.mean(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(r['total'], f_tot.mean(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(r['pp_error'], f_pp.std(axis=0, ddof=0) / np.sqrt(6), rtol=1e-12)
    np.testing.assert_allclose(r['total_error'], f_tot.std(axis=0, ddof=0) / np.sqrt(6), rtol=1e-12)
    assert r['n_walkers'] == 9 and r['n_bad'] == 2
    np.testing.assert_array_equal(r['atoms'], np.asarray(cell.atom_coords()))
    # no good walker: NaN; one: no error
    empty = _accumulator()[0]
    assert np.isnan(empty.forces()['pp']).all() and np.isnan(empty.forces()['total_error']).all()
    one = _accumulator()[0]
    one.sums = torch.as_tensor(force_helpers.sums_model(np.zeros(25), f_pp[:1], f_tot[:1]))
    assert np.array_equal(one.forces()['total'], f_tot[0]) and np.isnan(one.forces()['pp_error']).all()
    # state_dict round trip, save / load, load_state_dict
    sd = acc.state_dict()
    fresh = estimator.PseudopotentialForces.from_state_dict(sd)
    assert fresh.apply is None and fresh.n_walkers == 9 and not fresh.reduced and fresh.offset == 3
    for k in ('pp', 'pp_error', 'total', 'total_error'):
        np.testing.assert_array_equal(fresh.forces()[k], r[k])
    with pytest.raises(RuntimeError, match='no network'):
        fresh.update(torch.zeros(1, 12))
    path = str(tmp_path / 'forces_ecp.npz')
    acc.save(path)
    with np.load(path) as f:
        np.testing.assert_array_equal(f['total'], r['total'])
        np.testing.assert_array_equal(f['pp_error'], r['pp_error'])
    loaded = estimator.PseudopotentialForces.load(path)
    assert isinstance(loaded, estimator.PseudopotentialForces)
    np.testing.assert_array_equal(loaded.forces()['total'], r['total'])
    assert loaded.n_walkers == 9 and int(loaded.n_bad) == 2 and loaded.seed == acc.seed
    other = _accumulator()[0]
    other.load_state_dict(sd)
    np.testing.assert_array_equal(other.forces()['pp'], r['pp'])
    assert other.offset == 3                                                     # the rotations continue behind the loaded ones
    with pytest.raises(ValueError, match='another pseudopotential'):
        _accumulator(n_quad=6)[0].load_state_dict(sd)
    # merge: sums, counts and walkers add; another potential and the all-electron accumulator are refused
    before = acc.sums.clone()
    acc.merge(loaded)
    assert torch.equal(acc.sums, 2 * before) and acc.n_walkers == 18 and int(acc.n_bad) == 4
    np.testing.assert_allclose(acc.forces()['total'], r['total'], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='differ'):
        acc.merge(_accumulator(n_quad=6)[0])
    with pytest.raises(ValueError, match='differ'):
        acc.merge(estimator.IonForces(_Net(cell), None))
    # reduce at world size 1: the identity, once; afterwards no update; a reduced and a rank-local side do not merge on several ranks
    acc.reduce()
    assert acc.reduced and torch.equal(acc.sums, 2 * before) and acc.n_walkers == 18
    with pytest.raises(RuntimeError, match='already'):
        acc.reduce()
    with pytest.raises(RuntimeError, match='reduce'):
        acc.update(torch.zeros(1, 12))
    monkeypatch.setattr(constants, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='rank-local'):
        acc.merge(loaded)
