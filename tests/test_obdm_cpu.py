"""CPU checks of the one-body density matrix (`estimator.OneBodyDensityMatrix`, csrc/ds_obdm.h): the normalisation, pinned by the
determinant identity on the numpy model of tests/obdm_helpers.py, the natural orbitals, the refusals at construction, the
persistence round trips and the C-ABI symbols.  Nothing here needs a GPU."""
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import hf_helpers as hh
import obdm_helpers as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def state(nelec, norb, dm, ov, samples, n_bad, sim_a, basis_a, kpts):
    mb = max(norb)
    ri = lambda z: np.stack([np.asarray(z).real, np.asarray(z).imag], axis=-1).reshape(2, mb, mb, 2)
    return {'dm_sums': ri(dm), 'ov_sums': ri(ov), 'samples': np.asarray(samples, np.int64), 'n_bad': np.asarray(n_bad, np.int64),
            'nelec': np.asarray(nelec, np.int64), 'simulation_lattice': np.asarray(sim_a, np.float64),
            'basis_lattice': np.asarray(basis_a, np.float64), 'basis_kpts': np.asarray(kpts, np.float64),
            'basis_norb': np.asarray(norb, np.int64)}


@functools.lru_cache(maxsize=None)
def lih_net():
    from deepsolid_amd import network, systems
    cell = hh.lih_cell()
    go = hh.lih_system().gaussian_orbitals()
    return cell, go, network.make_solid_fermi_net(klist=go.klist, simulation_cell=cell, method_name='eval_logdet',
                                                  **systems.DETNET_DEFAULTS)


def test_determinant_identity_pins_the_normalisation():
    """psi = det[phi_j(r_e)] and a common r' per (walker, spin): sum_e q_e phi_k(r_e) = phi_k(r') sample by sample, so with M = N
    and first_electron = 0 the model's sums give density_matrix() == overlap().  Host orbitals of lih_system(), 3 walkers over
    +-1 cells: relative deviation 3.1e-15 at condition number 64."""
    from deepsolid_amd import estimator
    s = hh.lih_system()
    go = s.gaussian_orbitals()
    cell = hh.lih_cell()
    B, N, nelec = 3, 8, (4, 4)
    x = hh.walkers(s, B, seed=7, spread=1, sim_a=cell.a).reshape(B, N, 3)
    rng = np.random.default_rng(8)
    pts = (rng.uniform(size=(B, 2, 3)) + rng.integers(-1, 2, size=(B, 2, 3))) @ np.asarray(cell.a)
    shifts = ob.common_point_shifts(x, nelec, pts)
    mats = go.eval_orb_mat(x)
    w_idx, e_idx = ob.sample_electrons(B, N, N, 0)
    spin = (e_idx >= nelec[0]).astype(int)
    q = np.empty(B * N, dtype=np.complex128)
    phi_new = np.empty((B * N, 4), dtype=np.complex128)
    phi_old = np.empty((B * N, 4), dtype=np.complex128)
    cond = 0.0
    for sp in range(2):
        at_new = go.eval_orbitals_at(pts[:, sp, :], sp)
        for w in range(B):
            sel = (w_idx == w) & (spin == sp)
            q[sel] = ob.det_ratios(mats[sp][w], at_new[w])
            phi_new[sel] = at_new[w]
            phi_old[sel] = mats[sp][w]
            cond = max(cond, np.linalg.cond(mats[sp][w]))
    # the moved positions are the common points
    moved = x[w_idx, e_idx] + shifts.reshape(B * N, 3)
    assert np.abs(moved - pts[w_idx, spin]).max() < 1e-12
    dm, ov = ob.fold(q, None, phi_new, phi_old, spin)
    acc = estimator.OneBodyDensityMatrix.from_state_dict(
        state(nelec, (4, 4), dm, ov, [B * 4, B * 4], [0, 0], cell.a, s.a, s.kpts))
    for n, o in zip(acc.density_matrix(), acc.overlap()):
        dev = np.abs(n - o).max() / np.abs(o).max()
        print(f'relative deviation {dev:.3e} at condition number {cond:.1f}')
        assert dev <= 1e-12


def test_normalisation_against_a_hand_sum():
    from deepsolid_amd import estimator
    rng = np.random.default_rng(3)
    a = np.diag([3.0, 4.0, 5.0])
    dm = rng.normal(size=(2, 2, 2)) + 1j * rng.normal(size=(2, 2, 2))
    ov = rng.normal(size=(2, 2, 2)) + 1j * rng.normal(size=(2, 2, 2))
    acc = estimator.OneBodyDensityMatrix.from_state_dict(state((3, 0), (2, 1), dm, ov, [10, 0], [2, 0], 2 * a, a, np.zeros((1, 3))))
    n, s = acc.density_matrix(), acc.overlap()
    assert np.allclose(n[0], 3 * 60.0 * dm[0] / 8, rtol=1e-15, atol=0) and np.allclose(s[0], 60.0 * ov[0] / 8, rtol=1e-15, atol=0)
    assert n[1].shape == (1, 1) and np.all(n[1] == 0)                     # no electrons of that spin
    assert s[1].shape == (1, 1) and np.all(np.isnan(s[1]))                # and no samples to estimate an overlap from


def test_natural_orbitals_on_a_synthetic_pair():
    from deepsolid_amd import estimator
    rng = np.random.default_rng(5)
    M = 6
    r = rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))
    S = r @ r.conj().T / M + 0.5 * np.eye(M)
    d = rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M))
    D = d + d.conj().T
    z = np.zeros((M, M))
    a = np.eye(3) * 4.0
    # sums such that density_matrix()[0] = D and overlap()[0] = S: N = 2, Omega_p = 64, good = 128
    acc = estimator.OneBodyDensityMatrix.from_state_dict(state((2, 0), (M, 0), [D, z], [2 * S, z], [128, 0], [0, 0], a, a, np.zeros((1, 3))))
    assert np.abs(acc.density_matrix()[0] - D).max() < 1e-13 and np.abs(acc.overlap()[0] - S).max() < 1e-13
    occ, c = acc.natural_orbitals(0)
    ev, u = np.linalg.eigh(S)
    sm12 = (u / np.sqrt(ev)) @ u.conj().T
    want = np.sort(np.linalg.eigvalsh(sm12 @ D @ sm12))[::-1]
    assert np.all(np.diff(occ) <= 0) and np.abs(occ - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(c.conj().T @ S @ c - np.eye(M)).max() <= 1e-12
    assert np.abs(D @ c - S @ c @ np.diag(occ)).max() <= 1e-11
    occ1, c1 = acc.natural_orbitals(0, overlap='identity')
    assert np.abs(occ1 - np.sort(np.linalg.eigvalsh(D))[::-1]).max() <= 1e-12 * np.abs(D).max()
    assert np.abs(c1.conj().T @ c1 - np.eye(M)).max() <= 1e-12
    with pytest.raises(ValueError):
        acc.natural_orbitals(0, overlap='exact')


def test_refusals_at_construction():
    from deepsolid_amd import estimator
    cell, go, net = lih_net()
    params = None
    estimator.OneBodyDensityMatrix(net, params, go)                      # the basis of the network's own cell is accepted
    stub = lambda **kw: types.SimpleNamespace(**{**dict(a=go.a, kpts=go.kpts, nelec=go.nelec), **kw})
    with pytest.raises(ValueError, match='superlattice'):
        estimator.OneBodyDensityMatrix(net, params, stub(a=1.1 * go.a))
    with pytest.raises(ValueError, match='Bloch'):
        estimator.OneBodyDensityMatrix(net, params, stub(kpts=go.kpts + np.array([0.05, 0.0, 0.0])))
    with pytest.raises(ValueError, match='65'):
        estimator.OneBodyDensityMatrix(net, params, stub(nelec=(65, 0)))
    with pytest.raises(ValueError, match='samples_per_walker'):
        estimator.OneBodyDensityMatrix(net, params, go, samples_per_walker=0)
    # the simulation cell itself as the basis cell, and a doubled k list that stays on the allowed grid
    g = 2 * np.pi * np.linalg.inv(np.asarray(cell.a)).T
    estimator.OneBodyDensityMatrix(net, params, stub(a=np.asarray(cell.a), kpts=go.kpts[:1] + np.array([[1, -2, 3]]) @ g))


def test_round_trips(tmp_path):
    from deepsolid_amd import estimator
    cell, go, net = lih_net()
    rng = np.random.default_rng(9)
    c = lambda: rng.normal(size=(2, 4, 4)) + 1j * rng.normal(size=(2, 4, 4))
    sd1 = state((4, 4), (4, 4), c(), c(), [40, 24], [1, 0], cell.a, go.a, go.kpts)
    sd2 = state((4, 4), (4, 4), c(), c(), [8, 8], [0, 3], cell.a, go.a, go.kpts)
    a, b = estimator.OneBodyDensityMatrix.from_state_dict(sd1), estimator.OneBodyDensityMatrix.from_state_dict(sd2)
    a.merge(b)
    assert np.array_equal(a.dm_sums.numpy(), sd1['dm_sums'] + sd2['dm_sums']) and a.samples.tolist() == [48, 32]
    assert a.n_bad.tolist() == [1, 3]
    path = str(tmp_path / 'obdm.npz')
    a.save(path)
    with np.load(path) as f:
        assert {'dm_up', 'dm_dn', 'overlap_up', 'overlap_dn', 'basis_lattice', 'basis_kpts', 'basis_norb'} <= set(f.files)
        assert np.array_equal(f['dm_up'], a.density_matrix()[0])
    back = estimator.OneBodyDensityMatrix.load(path)
    for k, v in a.state_dict().items():
        assert np.array_equal(np.asarray(v), np.asarray(back.state_dict()[k])), k
    with pytest.raises(RuntimeError, match='no network'):
        back.update(torch.zeros(2, 24))
    back.reduce()
    with pytest.raises(RuntimeError, match='already'):
        back.reduce()
    # another basis cell is another setup
    other = estimator.OneBodyDensityMatrix.from_state_dict(state((4, 4), (4, 4), c(), c(), [8, 8], [0, 0], cell.a, cell.a, go.kpts))
    with pytest.raises(ValueError):
        a.merge(other)
    # an accumulator with a network takes a saved state of its own setup and is open for updates again
    live = estimator.OneBodyDensityMatrix(net, None, go)
    live.load_state_dict(a.state_dict())
    assert np.array_equal(live.ov_sums.numpy(), a.ov_sums.numpy()) and not live.reduced and live.apply is not None
    with pytest.raises(ValueError):
        live.load_state_dict(other.state_dict())


def test_host_orbitals_at_equal_the_rows_of_the_orbital_matrices():
    s = hh.lih_system()
    go = s.gaussian_orbitals()
    x = hh.walkers(s, 2, seed=3, spread=1).reshape(2, 8, 3)
    mats = go.eval_orb_mat(x)
    for sp in range(2):
        rows = go.eval_orbitals_at(x[:, 4 * sp:4 * sp + 4].reshape(-1, 3), sp)
        assert rows.shape == (8, 4) and rows.dtype == np.complex128
        assert np.abs(rows - mats[sp].reshape(8, 4)).max() <= 1e-14
    t = go.eval_orbitals_at(torch.as_tensor(x[0, :3]), 1)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.complex128 and tuple(t.shape) == (3, 4)
    empty = ob.hex_basis((3, 0)).gaussian_orbitals().eval_orbitals_at(np.zeros((5, 3)), 1)
    assert empty.shape == (5, 0)


def test_library_exports_the_obdm_symbols():
    from deepsolid_amd import _lib, device
    src = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for n in ('ds_hf_orbitals_at', 'ds_obdm_workspace_bytes', 'ds_obdm_accumulate'):
        assert re.search(r'\b%s\s*\(' % n, src), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.ds_obdm_workspace_bytes(None, 4, 4) == -1
    kern = open(os.path.join(ROOT, 'deepsolid_amd', 'csrc', 'ds_obdm.h')).read()
    assert int(re.search(r'constexpr int OBDM_GROUP = (\d+);', kern).group(1)) == device.OBDM_GROUP
