"""CPU checks of the stress tensor (csrc/ds_stress.h, `ewaldsum.ion_ion_stress`, `estimator.StressTensor`): the
closed form of stress_helpers.py against central differences of the oracle's Ewald energy on strained cells, the host ion-ion
constant, the trace identity tr(dE / d eps) = -E_ewald, the exported symbols, and the host logic of the accumulator on hand-made
sums."""
import os
import re

import numpy as np
import pytest
import torch

import stress_helpers as sth
from common import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tr(dE / d eps) + E_ewald of one uniform walker per cell, measured with the oracle when the estimator was designed: the truncation of
# the sums at fixed alpha (weight cut-off 1e-12, 27 real-space cells), not the code.  The bound of the trace test is ten times this.
TRACE_RESIDUAL = {'lih': 4.2e-8, 'bcc_li_s1': 3.9e-8, 'graphene_s1': 1.1e-6, 'h2': 4.0e-6}


def cell_of(name):
    """lih and h2: the fixture cells; bcc_li_s1 / graphene_s1: the one-primitive-cell bcc lithium and graphene cells."""
    from deepsolid_amd import systems
    if name == 'bcc_li_s1':
        return systems.build('bcc_li', S=1)[0]
    if name == 'graphene_s1':
        return systems.build('graphene', S=1)[0]
    return load_case(name)[1]


_CELLS = {}


def setup(name, nb=2):
    """-> (oracle EwaldSum, walkers (nb, 3N) uniform in the cell with every electron 0.3 bohr from every ion, cell), cached."""
    if name not in _CELLS:
        cell = cell_of(name)
        ew = sth.ewald(cell)
        _CELLS[name] = (ew, sth.fh.spread_walkers(cell, ew, nb, seed=9), cell)
    return _CELLS[name]


# ------------------------------------------------------------------------------------------------ 1. closed form vs finite differences
@pytest.mark.parametrize('name', ['lih', 'bcc_li_s1', 'graphene_s1', 'h2'])
def test_closed_form_vs_strained_oracle(name):
    """dE_ee / d eps, dE_ei / d eps (two walkers) and dE_ii / d eps from the closed form against central differences, h = 1e-5, of the
    oracle's energies on the strained cell with the electrons scaled along.  Bound 1e-6 max(1, |ref|), that of the force test for the
    same kind of comparison (truncation h^2 |E'''| / 6 ~ 1e-9, round-off eps E / h ~ 1e-10; measured <= 8.4e-9 absolute).  The strained
    oracle at zero strain is the oracle."""
    ew, x, _ = setup(name)
    e0, _ = sth.strained(ew, np.zeros((3, 3)))
    for xb in x:
        for got, want in zip(e0.energy(torch.as_tensor(xb)), ew.energy(torch.as_tensor(xb))):
            assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    ee, ei, ii = sth.closed_form(ew, x)
    fee, fei, fii = sth.fd_strain(ew, x, h=1e-5)
    worst = 0.0
    for what, a, b in (('ee', ee, fee), ('ei', ei, fei), ('ii', ii, fii)):
        err = np.abs(a - b)
        print(f'{name} {what}: max |closed form - finite differences| = {err.max():.3e}, scale {np.abs(b).max():.3g}')
        worst = max(worst, (err / np.maximum(1.0, np.abs(b))).max())
        assert np.allclose(a, np.swapaxes(a, -1, -2), rtol=0, atol=1e-12 * max(1.0, np.abs(a).max()))
    assert worst <= 1e-6
    assert np.abs(fei).max() > 1e-2 and np.abs(fii).max() > 1e-2


# ------------------------------------------------------------------------------------------------ 2. the host ion-ion constant
@pytest.mark.parametrize('name', ['lih', 'bcc_li_s1', 'graphene_s1', 'h2'])
def test_ion_ion_stress_vs_strained_oracle(name):
    """`ewaldsum.ion_ion_stress` against the same central differences (1e-6 max(1, |ref|)) and against the helper's closed form
    (1e-10 relative: the same formula, coded twice)."""
    from deepsolid_amd import ewaldsum
    ew, x, cell = setup(name)
    got = ewaldsum.ion_ion_stress(cell)
    assert got.shape == (3, 3) and got.dtype == np.float64 and np.array_equal(got, got.T)
    _, _, fii = sth.fd_strain(ew, x[:1], h=1e-5)
    _, _, ii = sth.closed_form(ew, x[:1])
    print(f'{name}: max |ion_ion_stress - finite differences| = {np.abs(got - fii).max():.3e}, - helper = {np.abs(got - ii).max():.3e}, '
          f'scale {np.abs(fii).max():.3g}')
    assert (np.abs(got - fii) / np.maximum(1.0, np.abs(fii))).max() <= 1e-6
    assert np.abs(got - ii).max() <= 1e-10 * max(1.0, np.abs(ii).max())


# ------------------------------------------------------------------------------------------------ 3. the trace identity
@pytest.mark.parametrize('name', ['lih', 'bcc_li_s1', 'graphene_s1', 'h2'])
def test_trace_identity(name):
    """For the Coulomb interaction tr(dE_ewald / d eps) = -E_ewald (a uniform scaling by lambda divides every distance by it).  The
    truncated sums at fixed alpha obey it to their convergence error: bound = ten times the residual measured per cell with the
    oracle (TRACE_RESIDUAL), per walker."""
    ew, x, _ = setup(name)
    ee, ei, ii = sth.closed_form(ew, x)
    worst = 0.0
    for b, xb in enumerate(x):
        e = sum(float(t) for t in ew.energy(torch.as_tensor(xb)))
        worst = max(worst, abs(np.trace(ee[b] + ei[b] + ii) + e))
    print(f'{name}: max |tr(dE/d eps) + E_ewald| = {worst:.3e} (bound {10 * TRACE_RESIDUAL[name]:.1e})')
    assert worst <= 10 * TRACE_RESIDUAL[name]


# ------------------------------------------------------------------------------------------------ 4. symbols
def test_library_exports_the_stress_symbols():
    from deepsolid_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    for n in ('ds_stress', 'ds_stress_workspace_bytes'):
        assert re.search(r'\b' + n + r'\(', header), f'{n} is not declared in include/deepsolid_hip.h'
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert lib.ds_stress_workspace_bytes(None, 4) == -1
    # refused before anything touches a device: a null handle
    rc = lib.ds_stress(None, None, None, 4, None, None, None, None, None, 0, None)
    assert rc != 0 and b'null' in lib.ds_last_error()


# ------------------------------------------------------------------------------------------------ 5. the accumulator on synthetic sums
def synthetic(seed, B):
    """Per-walker rows (B, 4, 6) with total = kin + ee + ei + a constant, as `ds_stress` writes them."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((B, 4, 6))
    p[:, 3] = p[:, 0] + p[:, 1] + p[:, 2] + np.arange(6) * 0.1
    return p


def filled(parts, latvec):
    from deepsolid_amd import estimator
    acc = estimator.StressTensor.from_state_dict(
        {'sums': sth.sums_model(np.zeros(49), parts), 'trace_sums': np.array([parts[:, 3, :3].sum(), (parts[:, 3, :3].sum(axis=1) ** 2).sum()]),
         'n_bad': np.zeros(1, np.int64), 'n_walkers': len(parts), 'atoms': np.zeros((1, 3)), 'charges': np.ones(1), 'latvec': latvec,
         'n_elec': 2})
    return acc


def test_stress_tensor_arithmetic(tmp_path):
    """sigma = mean(total) / V as a symmetric matrix, P = -tr sigma / 3, the naive errors, the GPa factor, merge and the state_dict
    round trip, on hand-made per-walker rows."""
    from deepsolid_amd import constants, estimator
    latvec = np.array([[3.0, 0.0, 0.0], [0.5, 4.0, 0.0], [0.0, 0.2, 5.0]])
    V = 60.0
    pa, pb = synthetic(1, 7), synthetic(2, 5)
    acc = filled(pa, latvec).merge(filled(pb, latvec))
    parts = np.concatenate([pa, pb])
    r = acc.stress()
    assert r['n_walkers'] == 12 and r['n_bad'] == 0 and abs(r['volume'] - V) <= 1e-12
    mean = parts.mean(axis=0)
    want = estimator.voigt_to_matrix(mean[3]) / V
    assert want[1, 2] == want[2, 1] == mean[3, 3] / V and want[0, 2] == mean[3, 4] / V and want[0, 1] == mean[3, 5] / V
    np.testing.assert_allclose(r['sigma'], want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(r['sigma_error'], estimator.voigt_to_matrix(parts[:, 3].std(axis=0, ddof=1) / np.sqrt(12)) / V, rtol=1e-10)
    for k, name in enumerate(('kin', 'ee', 'ei')):
        np.testing.assert_allclose(r['parts'][name], estimator.voigt_to_matrix(mean[k]) / V, rtol=0, atol=1e-14)
    np.testing.assert_allclose(r['parts']['ii'], estimator.voigt_to_matrix(np.arange(6) * 0.1) / V, rtol=0, atol=1e-14)
    tr = parts[:, 3, :3].sum(axis=1)
    assert abs(r['pressure'] + tr.mean() / (3 * V)) <= 1e-14
    assert abs(r['pressure_error'] - tr.std(ddof=1) / np.sqrt(12) / (3 * V)) <= 1e-12
    # 1 Ha / bohr^3 = E_h / a_0^3 = 29421.02 GPa (CODATA 2018)
    assert abs(constants.HARTREE_PER_BOHR3_IN_GPA - 29421.0157) < 1e-3
    assert r['pressure_gpa'] == r['pressure'] * constants.HARTREE_PER_BOHR3_IN_GPA
    # round trips
    path = str(tmp_path / 'stress.npz')
    acc.save(path)
    loaded = estimator.StressTensor.load(path)
    np.testing.assert_array_equal(loaded.stress()['sigma'], r['sigma'])
    assert loaded.stress()['pressure_error'] == r['pressure_error']
    with np.load(path) as f:
        for k in ('sums', 'trace_sums', 'n_bad', 'n_walkers', 'latvec', 'sigma', 'sigma_error', 'pressure', 'pressure_gpa', 'volume'):
            assert k in f.files, k
    fresh = filled(pa, latvec).load_state_dict(acc.state_dict())
    np.testing.assert_array_equal(fresh.stress()['sigma'], r['sigma'])
    # refusals of the host logic
    with pytest.raises(ValueError, match='differ'):
        acc.merge(filled(pa, 2 * latvec))
    with pytest.raises(RuntimeError, match='no network'):
        loaded.update(torch.zeros(1, 6))
    acc.reduce()
    with pytest.raises(RuntimeError, match='already'):
        acc.reduce()
    # no good walker: NaN everywhere; one: no error
    empty = filled(pa[:0], latvec).stress()
    assert np.isnan(empty['sigma']).all() and np.isnan(empty['pressure'])
    one = filled(pa[:1], latvec).stress()
    assert np.isfinite(one['sigma']).all() and np.isnan(one['sigma_error']).all() and np.isnan(one['pressure_error'])


def test_pseudopotential_is_refused():
    from deepsolid_amd import estimator
    with pytest.raises(NotImplementedError, match='pseudopotential'):
        estimator.StressTensor(object(), None, pseudopotential=object())


# ------------------------------------------------------------------------------------------------ 6. the wave-function term on the CPU
@pytest.mark.parametrize('name', ['lih', 'lih_twist'])
def test_strained_cell_keeps_fractions_and_twist(name):
    """`supercell.strained`: lattice and atoms times 1 + eps, k points times its inverse, for the simulation cell and its primitive
    cell; fractional atom coordinates, k . a, the supercell matrix, electron numbers and the feature lattices' duality unchanged."""
    from deepsolid_amd import supercell
    _, cell, klist, _, _ = load_case(name)
    eps = np.array([[1e-2, 3e-3, -2e-3], [3e-3, -2e-2, 1e-3], [-2e-3, 1e-3, 5e-3]])
    F = np.eye(3) + eps
    c2, k2 = supercell.strained(cell, klist, eps)
    for a, b in ((cell, c2), (cell.original_cell, c2.original_cell)):
        np.testing.assert_allclose(b.a, np.asarray(a.a) @ F, rtol=0, atol=1e-13)
        fa, fb = a.atom_coords() @ np.linalg.inv(a.a), b.atom_coords() @ np.linalg.inv(b.a)
        assert np.abs(fa - fb).max() <= 1e-13
        assert [b.atom_symbol(i) for i in range(b.natm)] == [a.atom_symbol(i) for i in range(a.natm)]
        np.testing.assert_allclose(b.BV @ b.AV.T, a.BV @ a.AV.T, rtol=0, atol=1e-12)
        np.testing.assert_allclose(b.BV, a.BV @ np.linalg.inv(F), rtol=0, atol=1e-13)
    assert c2.nelec == cell.nelec and c2.scale == cell.scale and np.array_equal(c2.S, cell.S)
    for ka, kb in zip(klist, k2):
        assert np.abs(np.asarray(ka) @ np.asarray(cell.a).T - kb @ c2.a.T).max() <= 1e-13          # k . a, the twist included
    if name == 'lih_twist':
        assert np.abs(np.asarray(klist[0]) @ np.asarray(cell.a).T / (2 * np.pi) % 1.0).max() > 0.05      # there is a twist
    with pytest.raises(ValueError, match='symmetric'):
        supercell.strained(cell, klist, np.array([[0, 1e-3, 0], [0, 0, 0], [0, 0, 0]]))


@pytest.mark.parametrize('name', ['lih', 'lih_twist'])
def test_oracle_log_derivative_is_converged_in_h(name):
    """O = d log psi_eps((1 + eps) x) / d eps of the oracle network on strained cells, two walkers, by central differences at h = 1e-4
    (the step of `StressTensor`) and h / 2.  A central difference errs by c h^2 + r(h) with r the round-off of the two forwards,
    |r(h)| <= 2 u / 2h, u = 64 eps max(1, |log psi|) (a forward of a few thousand operations).  c h^2 is measured by the step
    2h: |O(2h) - O(h)| = 3 c h^2.  So |O(h) - O(h / 2)| = 3/4 c h^2 + round-off <= |O(2h) - O(h)| / 4 + the round-off of the four
    differences involved, which is the bound; and the difference itself must be small against O (1e-6 max(1, |O|)), or h would be
    no step to differentiate with."""
    fx, cell, klist, net_kw, params = load_case(name)
    x = fx['x'][:2]
    h = 1e-4
    O2, _ = sth.oracle_log_derivative(cell, klist, net_kw, params, x, 2 * h)
    O1, big = sth.oracle_log_derivative(cell, klist, net_kw, params, x, h)
    Oh, _ = sth.oracle_log_derivative(cell, klist, net_kw, params, x, h / 2)
    u = 64 * 2.0 ** -52 * max(1.0, big)
    roundoff = u / (2 * h) + 2 * u / h + 2 * u / h           # r(2h) / 4 ... bounded by r(2h), + r(h) twice, + r(h / 2)
    diff = np.abs(O1 - Oh)
    bound = np.abs(O2 - O1) / 4 + roundoff
    print(f'{name}: max |O| = {np.abs(O1).max():.4g}, max |O(h) - O(h/2)| = {diff.max():.3e}, max |O(2h) - O(h)| / 4 = '
          f'{(np.abs(O2 - O1) / 4).max():.3e}, round-off allowance {roundoff:.3e}')
    assert np.all(diff <= bound)
    assert diff.max() <= 1e-6 * max(1.0, np.abs(O1).max())
    assert np.abs(O1.real).max() > 1e-2
    if name == 'lih_twist':
        assert np.abs(O1.imag).max() > 1e-3


def test_wavefunction_term_block_arithmetic():
    """`stress()` on hand-made block rows: per block sum total / n / V + 2 sum t / (n - 1) / V, weighted by n; the state_dict round
    trip keeps the rows; float32 networks are refused."""
    from deepsolid_amd import estimator
    latvec = np.diag([3.0, 4.0, 5.0])
    V = 60.0
    rng = np.random.default_rng(4)
    rows = np.concatenate([np.array([[10.0], [14.0], [12.0]]), rng.standard_normal((3, 14))], axis=1)
    acc = filled(synthetic(1, 7), latvec)
    sd = acc.state_dict()
    sd.update(wavefunction_term=np.bool_(True), strain_step=np.float64(1e-4), rows=rows)
    acc = estimator.StressTensor.from_state_dict(sd)
    assert acc.vmc_only
    r = acc.stress()
    n = rows[:, 0]
    wf = 2 * rows[:, 9:] / (n - 1)[:, None] / V
    tot = rows[:, 3:9] / n[:, None] / V + wf
    np.testing.assert_allclose(r['wavefunction'], estimator.voigt_to_matrix((wf * n[:, None]).sum(0) / n.sum()), rtol=1e-13)
    np.testing.assert_allclose(r['sigma_total'], estimator.voigt_to_matrix((tot * n[:, None]).sum(0) / n.sum()), rtol=1e-13)
    np.testing.assert_allclose(r['sigma_total_error'], estimator.voigt_to_matrix(tot.std(axis=0, ddof=1) / np.sqrt(3)), rtol=1e-10)
    assert abs(r['pressure_total'] + np.trace(r['sigma_total']) / 3) <= 1e-15 and r['n_blocks'] == 3
    again = estimator.StressTensor.from_state_dict(acc.state_dict())
    np.testing.assert_array_equal(again.stress()['sigma_total'], r['sigma_total'])
    with pytest.raises(ValueError, match='differ'):
        acc.merge(filled(synthetic(1, 7), latvec))             # one with and one without the wave-function term

    class Net32:
        dtype = torch.float32
    with pytest.raises(ValueError, match='float64'):
        estimator.StressTensor(Net32(), None, wavefunction_term=True)
