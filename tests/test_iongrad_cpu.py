"""CPU checks of the ion gradient of log psi (csrc/ds_iongrad.h): the autograd reference of
tests/iongrad_helpers.py against central differences and the two translation identities, the host logic of
`estimator.PrimitiveForces` against a numpy model, and the C ABI.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import iongrad_helpers as H
from common import load_case
from deepsolid_amd import systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize('name', ['lih', 'lih_tri', 'bcc_li'])
def test_reference_vs_finite_differences_and_translations(name):
    """Autograd in the atoms against central differences (h = 1e-5: round-off eps |log psi| / h ~ 1e-9 and truncation
    h^2 f''' / 6 ~ 1e-8 near a nucleus, so 1e-7 of max(1, |ref|)), and the two identities of a rigid translation of electrons
    and atoms: the real parts cancel (5e-13 of the largest entry), the imaginary parts sum to the occupied k-points (1e-13
    likewise; bcc-Li: (11.643, 9.703, 9.703))."""
    fx, cell, klist, net_kw, params = load_case(name)
    x = systems.synthetic_walkers(cell, 2, seed=77)
    O, lp = H.ion_grad_ref(cell, klist, net_kw, params, x)
    assert O.shape == (2, len(cell.original_cell.atom_coords()), 3) and np.isfinite(O).all()
    fd = H.ion_grad_fd(cell, klist, net_kw, params, x)
    assert np.abs(O - fd).max() <= 1e-7 * max(1.0, np.abs(O).max()), np.abs(O - fd).max()
    g = H.walker_grad_ref(cell, klist, net_kw, params, x).reshape(2, sum(cell.nelec), 3)
    s = O.sum(1) + g.sum(1)
    scale = max(np.abs(O).max(), np.abs(g).max())
    ksum = H.klist_row_sum(klist, cell.nelec)
    assert np.abs(s.real).max() <= 5e-13 * scale
    assert np.abs(s.imag - ksum).max() <= 1e-13 * max(scale, np.abs(ksum).max())
    if name == 'bcc_li':
        np.testing.assert_allclose(ksum, [11.643, 9.703, 9.703], atol=5e-4)


# ------------------------------------------------------------------------------------------------ 2. the fold onto the primitive atoms
@pytest.mark.parametrize('name,scale', [('lih_2x1x1', 2), ('graphene', None), ('lih', 1)])
def test_primitive_fold(name, scale):
    from deepsolid_amd import estimator
    _, cell, _, _, _ = load_case(name)
    prim = cell.original_cell
    sim, pa = np.asarray(cell.atom_coords()), np.asarray(prim.atom_coords())
    owner, sc = estimator.primitive_fold(sim, pa, prim.a)
    assert sc == len(sim) // len(pa) and (scale is None or sc == scale)
    np.testing.assert_array_equal(owner, np.arange(len(sim)) // sc)
    np.testing.assert_array_equal(owner, H.fold_model(sim, pa, prim.a))
    # the images of an atom carry its charge
    q, pq = np.asarray(cell.atom_charges()), np.asarray(prim.atom_charges())
    np.testing.assert_array_equal(q, pq[owner])
    if sc > 1:
        # image-major order (all atoms of image 0, then of image 1, ...): refused, by the model too
        perm = np.arange(len(sim)).reshape(len(pa), sc).T.reshape(-1)
        with pytest.raises(ValueError, match='atom-major'):
            estimator.primitive_fold(sim[perm], pa, prim.a)
        with pytest.raises(ValueError):
            H.fold_model(sim[perm], pa, prim.a)
    with pytest.raises(ValueError, match='multiple'):
        estimator.primitive_fold(sim[:-1], pa, prim.a)


# ------------------------------------------------------------------------------------------------ 3. the accumulator on the host
class _System:
    """Stands in for `DeviceSystem` on CPU tensors: deterministic synthetic per-walker numbers; a walker whose first coordinate is
    not finite is bad in `ion_forces` (NaN rows), as on the device."""

    def __init__(self, n_elec, As, A):
        self.n, self.As, self.A, self.calls = n_elec, As, A, []

    def _rng(self, x, salt):
        return np.random.default_rng(abs(hash((salt, float(torch.nan_to_num(x).sum())))) % 2 ** 32)

    def local_energy(self, params, x):
        self.calls.append('local_energy')
        r = self._rng(x, 1).normal(size=(x.shape[0], 3))
        return torch.as_tensor(r[:, :2].copy()), torch.as_tensor(r[:, 2].copy()), None, None

    def logpsi_grad(self, params, x):
        self.calls.append('logpsi_grad')
        return None, torch.complex(x.clone(), x.clone())

    def ion_forces(self, x, drift, cutoff=None, want_walker=True):
        self.calls.append('ion_forces')
        r = self._rng(x, 2).normal(size=(2, x.shape[0], self.As, 3))
        r[:, ~np.isfinite(x[:, 0].numpy())] = np.nan
        return dict(hf=torch.as_tensor(r[0]), zv=torch.as_tensor(r[1]), n_bad=torch.zeros(1, dtype=torch.int64), sums=None)

    def ion_grad(self, x):
        r = self._rng(x, 3).normal(size=(2, x.shape[0], self.A, 3))
        return r[0] + 1j * r[1]

    def logpsi_ion_vjp(self, params, x, cot):
        self.calls.append('logpsi_ion_vjp')
        O = self.ion_grad(x)
        c = cot.numpy()
        out = c[:, 0, None, None] * O.real + c[:, 1, None, None] * O.imag
        out[~np.isfinite(x[:, 0].numpy())] = np.nan            # (0 x NaN: what a bad walker's sweep returns)
        return torch.as_tensor(out), None, None


class _Net:
    def __init__(self, cell, system):
        self.simulation_cell, self.system = cell, system


def _accumulator(name='lih_2x1x1'):
    from deepsolid_amd import estimator
    _, cell, _, _, _ = load_case(name)
    As, A = len(cell.atom_coords()), len(cell.original_cell.atom_coords())
    system = _System(sum(cell.nelec), As, A)
    return estimator.PrimitiveForces(_Net(cell, system), None), cell, system


def _walkers(cell, B, seed):
    return torch.as_tensor(systems.synthetic_walkers(cell, B, seed=seed))


def _model_row(acc, system, x, E=None):
    if E is None:
        ke, ew, _, _ = system.local_energy(None, x)
        E = (ke[:, 0] + ew).numpy() + 1j * ke[:, 1].numpy()
    f = system.ion_forces(x, None)
    return H.block_row_model(np.asarray(E), f['zv'].numpy(), f['hf'].numpy(), system.ion_grad(x), acc.owner, acc.n_atoms)


def test_primitive_forces_host_logic(tmp_path):
    from deepsolid_amd import dmc, estimator
    acc, cell, system = _accumulator()
    A = acc.n_atoms
    assert acc.scale == 2 and A == 2 and acc.row_len == 3 + 9 * A and acc.cutoff == estimator.wigner_seitz_radius(cell.a)
    np.testing.assert_array_equal(acc.atoms, np.asarray(cell.original_cell.atom_coords()))
    with pytest.raises(ValueError, match='coordinates'):
        acc.update(torch.zeros(2, 9))
    empty = acc.forces()
    assert empty['n_blocks'] == 0 and np.isnan(empty['total']).all()
    sizes = [40, 25, 33, 40, 40, 17, 40, 40, 29, 40]
    xs = [_walkers(cell, B, seed=100 + i) for i, B in enumerate(sizes)]
    xs[1][3, 0] = float('nan')                                     # one bad walker in block 1
    xs[4][0, 0] = float('inf')
    model = []
    for i, x in enumerate(xs):
        system.calls.clear()
        if i % 2:
            ke, ew, _, _ = system.local_energy(None, x)
            E = torch.complex(ke[:, 0] + ew, ke[:, 1])
            system.calls.clear()
            acc.update(x, energies=E)
            assert system.calls == ['logpsi_grad', 'ion_forces', 'logpsi_ion_vjp']
        else:
            acc.update(x)
            assert system.calls == ['local_energy', 'logpsi_grad', 'ion_forces', 'logpsi_ion_vjp']      # four calls, one sweep
        model.append(_model_row(acc, system, x))
    rows = acc.rows.numpy()
    model = np.asarray(model)
    assert rows.shape == (len(sizes), 3 + 9 * A)
    np.testing.assert_allclose(rows, model, rtol=1e-12, atol=1e-12)
    assert rows[1, 0] == sizes[1] - 1 and rows[4, 0] == sizes[4] - 1 and int(acc.n_bad) == 2 and acc.n_walkers == sum(sizes)
    # normalisation: per block sum / n and -2 sum t / (n - 1), weighted by n, reblocked errors
    f = acc.forces()
    ref = H.forces_model(model, A, dmc.reblock)
    for k in ('total', 'zv', 'hf', 'pulay'):
        np.testing.assert_allclose(f[k], ref[k][0], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(f[k + '_error'], ref[k][1], rtol=1e-12, atol=1e-14)
        assert (f[k + '_error'] > 0).all()
    n = model[:, 0]
    t = model[:, 3:].reshape(-1, A, 3, 3)[..., 2]
    np.testing.assert_allclose(f['pulay'], (-2 * t / (n - 1)[:, None, None] * n[:, None, None]).sum(0) / n.sum(), rtol=1e-12)
    np.testing.assert_allclose(f['total'], f['zv'] + f['pulay'], rtol=1e-12, atol=1e-14)
    assert f['n_blocks'] == len(sizes) and f['n_bad'] == 2 and f['n_walkers'] == sum(sizes)
    np.testing.assert_allclose(f['energy'], (model[:, 1].sum() + 1j * model[:, 2].sum()) / n.sum(), rtol=1e-13)
    # state_dict round trip, save / load
    back = estimator.PrimitiveForces.from_state_dict(acc.state_dict())
    np.testing.assert_array_equal(back.rows.numpy(), rows)
    assert back.n_walkers == acc.n_walkers and int(back.n_bad) == 2 and back.apply is None
    with pytest.raises(RuntimeError, match='no network'):
        back.update(xs[0])
    acc.save(tmp_path / 'f.npz')
    loaded = estimator.PrimitiveForces.load(tmp_path / 'f.npz')
    np.testing.assert_array_equal(loaded.forces()['total'], f['total'])
    with np.load(tmp_path / 'f.npz') as z:
        np.testing.assert_array_equal(z['pulay'], f['pulay'])
    # merge: the other's blocks continue the series
    a2, _, s2 = _accumulator()
    extra = _walkers(cell, 21, seed=7)
    a2.update(extra)
    merged = estimator.PrimitiveForces.from_state_dict(acc.state_dict()).merge(a2)
    np.testing.assert_allclose(merged.rows.numpy(), np.concatenate([rows, _model_row(a2, s2, extra)[None]]), rtol=1e-12, atol=1e-12)
    assert merged.n_walkers == sum(sizes) + 21
    other, _, _ = _accumulator('lih')
    with pytest.raises(ValueError, match='differ'):
        acc.merge(other)
    # a block with one good walker has no covariance: left out of the normalisation
    a2.update(extra[:1])
    assert a2.rows.shape[0] == 2 and a2.forces()['n_blocks'] == 1
    # update after reduce() raises; so does a second reduce
    acc.reduce()
    with pytest.raises(RuntimeError, match='reduce'):
        acc.update(xs[0])
    with pytest.raises(RuntimeError, match='already'):
        acc.reduce()
    np.testing.assert_array_equal(acc.forces()['total'], f['total'])        # the identity at world size 1


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def _declared():
    src = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return set(re.findall(r'\b(ds_[a-z0-9_]+)\s*\(', src))


def test_library_exports_the_ion_gradient_symbols():
    from deepsolid_amd import _lib
    lib = _lib.load()
    for n in ('ds_logpsi_ion_vjp', 'ds_ion_vjp_workspace_bytes'):
        assert n in _declared(), f'{n} is not declared in include/deepsolid_hip.h'
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert lib.ds_ion_vjp_workspace_bytes(None, 4) == -1
    rc = lib.ds_logpsi_ion_vjp(None, None, None, 4, None, None, None, None, None, 0, None)
    assert rc != 0 and b'null' in lib.ds_last_error()
    assert 'ion_vjp' in _lib.PROF_KINDS and len(_lib.PROF_KINDS) == 13
