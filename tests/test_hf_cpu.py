"""CPU checks of deepsolid_amd/hf.py (GaussianOrbitals, the PySCF-free holder of a Hartree-Fock solution) and of the restatement
tests/hf_helpers.py that the GPU tests compare the kernel with.  No PySCF exists where these run: the conventions are fixed by an
independent reciprocal-space evaluation instead (hf_helpers module docstring)."""
import inspect
import math

import numpy as np
import pytest

import hf_helpers as hh
from deepsolid_amd import hf

K_OFF_GRID = np.array([0.137, 0.291, 0.413])      # fractions of the reciprocal vectors: on no supercell grid


@pytest.mark.parametrize('kind', ['triclinic', 'fcc'])
def test_direct_image_sum_equals_reciprocal_space_sum(kind):
    """The helper's AOs two ways, s, p and d shells, k = 0 and an off-grid k: 1e-11 of the largest AO magnitude (both sums are
    truncated below 1e-16 and hold fewer than 1e4 terms of O(1)).  Fixes the sign of the Bloch phase and the order and the
    factors of the harmonics; then the package's own host path is held to the helper's direct sum."""
    s = hh.pin_system(kind)
    recip = 2 * math.pi * np.linalg.inv(s.a).T
    kpts = np.array([np.zeros(3), K_OFF_GRID @ recip])
    r = np.random.default_rng(8).uniform(size=(6, 3)) @ s.a
    direct = hh.ao_direct(s, r, kpts=kpts)
    rec, n_g = hh.ao_recip(s, r, kpts=kpts)
    assert s.images.shape[0] < 10000 and n_g < 10000
    scale = np.abs(direct).max()
    col = 0
    for _, l, _, _ in s.shells:                            # every shell takes part in the comparison
        assert np.abs(direct[:, :, col:col + 2 * l + 1]).max() > 1e-3 * scale
        col += 2 * l + 1
    dev = np.abs(direct - rec).max() / scale
    print(f'{kind}: {s.images.shape[0]} images, {n_g} G vectors, deviation {dev:.3e}')
    assert dev <= 1e-11
    go = hf.GaussianOrbitals(s.a, s.atoms, s.shells, kpts, [[np.zeros((s.nao, 1)), np.zeros((s.nao, 0))]] * 2, (1, 1), images=s.images)
    assert np.abs(go.eval_aos_host(r) - direct).max() <= 1e-11 * scale


def test_bloch_property():
    """ao_k(r + a_j) = exp(i k.a_j) ao_k(r) for the direct sum (with translations out to one more cell), and eval_orb_mat of a
    walker moved by primitive vectors changes by the wrap phase of each orbital's k point alone."""
    s = hh.hex_system((5, 4))
    r = np.random.default_rng(2).uniform(size=(5, 3)) @ s.a
    base = hh.ao_direct(s, r)
    far = hh.lattice_points(s.a, np.linalg.norm(s.images, axis=1).max() + np.linalg.norm(s.a, axis=1).max())
    scale = np.abs(base).max()
    for j in range(3):
        moved = hh.ao_direct(s, r + s.a[j], images=far)
        want = base * np.exp(1j * s.kpts @ s.a[j])[:, None, None]
        assert np.abs(moved - want).max() <= 1e-11 * scale, j
    go = s.gaussian_orbitals()
    x = hh.walkers(s, 4, seed=9).reshape(4, -1, 3)
    n = np.random.default_rng(3).integers(-3, 4, size=x.shape)
    m0, m1 = go.eval_orb_mat(x), go.eval_orb_mat(x + n @ s.a)
    i0 = 0
    for sp in range(2):
        ne = s.nelec[sp]
        shift = (n @ s.a)[:, i0:i0 + ne]                                        # (B, ne, 3)
        phase = np.exp(1j * np.einsum('bec,oc->beo', shift, go.klist[sp]))
        assert np.abs(m1[sp] - m0[sp] * phase).max() <= 1e-11 * np.abs(m0[sp]).max()
        i0 += ne
    for got, want in zip(m0, hh.orb_mats(s, x)):
        assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize('l,exps,coefs', [(0, [0.7], [1.0]), (1, [0.4], [1.0]), (2, [1.1], [1.0]), (0, [1.8, 0.45, 0.13], [0.3, 0.5, 0.4]),
                                          (1, [1.5, 0.5, 0.2], [0.2, -0.6, 0.9]), (2, [1.2, 0.6, 0.15], [0.5, 0.3, 0.4])])
def test_normalize_shell_gives_unit_norm(l, exps, coefs):
    """int |chi|^2 d^3r = 1: the closed form sum_ij c_i c_j Gamma(l + 3/2) / (2 (a_i + a_j)^(l + 3/2)), and the same integral by
    quadrature (radial Simpson rule times a Gauss-Legendre x uniform-azimuth rule on the sphere for every m)."""
    e = np.asarray(exps)
    c = hf.normalize_shell(l, exps, coefs)
    closed = sum(ci * cj * math.gamma(l + 1.5) / (2 * (ai + aj) ** (l + 1.5)) for ci, ai in zip(c, e) for cj, aj in zip(c, e))
    assert abs(closed - 1.0) <= 1e-13
    r = np.linspace(0.0, 30.0, 60001)
    f = r ** 2 * (np.exp(-np.outer(r * r, e)) @ c) ** 2              # the r^l of the harmonic is taken on the sphere below
    w = np.full(r.size, 2.0)
    w[1::2] = 4.0
    w[0] = w[-1] = 1.0
    ct, wt = np.polynomial.legendre.leggauss(12)
    ph = 2 * math.pi * (np.arange(24) + 0.5) / 24
    st = np.sqrt(1 - ct * ct)
    u = np.stack([np.outer(st, np.cos(ph)), np.outer(st, np.sin(ph)), np.outer(ct, np.ones(24))], axis=-1)
    ylm = hh.solid_harmonics(l, u)                                  # unit vectors: (12, 24, m)
    gram = np.einsum('tpm,tpn,t->mn', ylm, ylm, wt) * (2 * math.pi / 24)
    assert np.abs(gram - np.eye(2 * l + 1)).max() <= 1e-13           # orthonormal on the sphere
    radial = float((f * r ** (2 * l) * w).sum() * (r[1] - r[0]) / 3.0)
    assert abs(radial - 1.0) <= 1e-10


def test_save_load_klist_and_signature(tmp_path):
    for nelec in ((3, 0), (5, 4)):                                   # an empty spin channel travels through the file as well
        s = hh.hex_system(nelec)
        go = s.gaussian_orbitals()
        path = tmp_path / f'hf{nelec[1]}.npz'
        go.save(path)
        with np.load(path, allow_pickle=False) as z:                 # numbers only
            assert all(z[k].dtype.kind in 'ifc' for k in z.files)
        back = hf.GaussianOrbitals.load(path)
        a, b = go._arrays(), back._arrays()
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        assert back.nelec == nelec and back.nao == 18 and back.on_device is True
        x = hh.walkers(s, 2, seed=1).reshape(2, -1, 3)
        assert all(np.array_equal(p, q) for p, q in zip(go.eval_orb_mat(x), back.eval_orb_mat(x)))
    # hf.py:99-104: per spin, every k point repeated by its occupation
    for sp, occ in enumerate(([2, 2, 1], [2, 1, 1])):
        want = np.concatenate([np.tile(k[None], (n, 1)) for k, n in zip(s.kpts, occ)])
        assert np.array_equal(go.klist[sp], want)
    assert hh.hex_system((3, 0)).gaussian_orbitals().klist[1].shape == (0, 3)
    # a file without `images` gets the default translations
    arrays = {k: v for k, v in a.items() if k != 'images'}
    np.savez(tmp_path / 'noimg.npz', **arrays)
    assert np.array_equal(hf.GaussianOrbitals.load(tmp_path / 'noimg.npz').images, hf.default_images(s.a, a['exps']))
    from deepsolid_amd import inference, pretrain
    sig = inspect.signature(pretrain.pretrain_hartree_fock_usingHF)
    assert list(sig.parameters) == ['params', 'data', 'batch_orbitals', 'sharded_key', 'cell', 'scf_approx', 'iterations',
                                    'learning_rate', 'nsteps', 'full_det', 'history', 'noise']
    assert [sig.parameters[k].default for k in ('iterations', 'learning_rate', 'nsteps', 'full_det', 'history', 'noise')] == \
        [1000, 5e-3, 1, False, None, None]
    sig = inspect.signature(inference.run_training)
    assert sig.parameters['pretrain_method'].default == 'net' and sig.parameters['pretrain_steps'].default == 1
    for name in ('kinetic', 'laplacian', 'eval_inverse'):            # stated as not provided
        assert not hasattr(go, name) and name in hf.__doc__


def test_construction_refusals():
    s = hh.lih_system()
    ok = dict(a=s.a, atoms=s.atoms, shells=s.shells, kpts=s.kpts, mo_coeff=s.mo, nelec=s.nelec)
    hf.GaussianOrbitals(**ok)
    z = lambda n: np.zeros((s.nao, n))
    with pytest.raises(ValueError, match='l = 3'):
        hf.GaussianOrbitals(**{**ok, 'shells': s.shells + [(0, 3, [0.5], [1.0])]})
    many = [(0, 2, [0.5], [1.0])] * 26                                # 130 AOs
    with pytest.raises(ValueError, match='130 atomic orbitals'):
        hf.GaussianOrbitals(**{**ok, 'shells': many, 'mo_coeff': [[np.zeros((130, 2))] * 2] * 2})
    with pytest.raises(ValueError, match='65 k points'):
        hf.GaussianOrbitals(**{**ok, 'kpts': np.zeros((65, 3)), 'mo_coeff': [[z(0)] * 65] * 2, 'nelec': (0, 0)})
    with pytest.raises(ValueError, match='electrons per spin'):
        hf.GaussianOrbitals(**{**ok, 'mo_coeff': [[z(33), z(32)], [z(2), z(2)]], 'nelec': (65, 4)})
    with pytest.raises(ValueError, match='occupied orbitals'):
        hf.GaussianOrbitals(**{**ok, 'nelec': (4, 3)})
    for name in ('atoms', 'kpts'):                                    # a NaN must not reach the phase table
        bad = np.array(ok[name], dtype=np.float64)
        bad[1, 2] = np.nan
        with pytest.raises(ValueError, match=f'`{name}` holds a value that is not finite'):
            hf.GaussianOrbitals(**{**ok, name: bad})
    with pytest.raises(ValueError, match='`images` holds a value that is not finite'):
        hf.GaussianOrbitals(**ok, images=np.array([[0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]]))
    with pytest.raises(ValueError, match='occupied orbitals'):
        hf.GaussianOrbitals(**{**ok, 'mo_coeff': [[z(2), z(1)], [z(2), z(2)]]})


@pytest.mark.parametrize('kind', ['triclinic', 'fcc', 'hex'])
def test_default_images_hold_every_term_above_the_precision(kind):
    """Brute force over a box well beyond the radius: every L whose largest possible term exp(-alpha_min max(0, |L| - D)^2) (the
    walker and the atom anywhere in the cell, D the longest body diagonal) exceeds the precision is in the list; the list is
    sorted by length and holds no vector twice."""
    s = hh.hex_system((5, 4)) if kind == 'hex' else hh.pin_system(kind)
    for precision in (1e-12, 1e-6):
        got = hf.default_images(s.a, [s.alpha_min, 1.0], precision)
        D = hh.body_diagonal(s.a)
        n = np.array(np.meshgrid(*[np.arange(-14, 15)] * 3, indexing='ij')).reshape(3, -1).T
        L = n @ s.a
        norm = np.linalg.norm(L, axis=1)
        need = L[np.exp(-s.alpha_min * np.maximum(0.0, norm - D) ** 2) > precision]
        assert norm.max() > np.linalg.norm(got, axis=1).max() + 1.0 and need.shape[0] > 27
        have = {tuple(v) for v in np.round(got @ np.linalg.inv(s.a)).astype(int)}
        assert len(have) == got.shape[0]
        assert {tuple(v) for v in np.round(need @ np.linalg.inv(s.a)).astype(int)} <= have
        gn = np.linalg.norm(got, axis=1)
        assert np.all(np.diff(gn) >= -1e-8) and gn[0] == 0.0


def test_sampler_seed_leaves_every_decision_decidable():
    """The seed of the GPU sampler test (tools/find_hf_sampler_seed.py), from the helper alone: every walker, every move has
    |lp2 - lp1 - log u| > 1e-6, both decisions occur."""
    s = hh.lih_system()
    sim_a = hh.lih_cell().a
    normals, uniforms = hh.sampler_noise(hh.SAMPLER_SEED, sum(s.nelec))
    _, dec, margin = hh.replay_sampler(s, sim_a, hh.sampler_start(s, sim_a), normals, uniforms)
    assert dec.shape == (hh.SAMPLER_ITERATIONS, hh.SAMPLER_NSTEPS, hh.SAMPLER_BATCH)
    assert np.abs(margin).min() > hh.SAMPLER_MARGIN
    assert dec.any() and (~dec).any()


def test_library_refuses_bad_descriptors_before_touching_the_device():
    """`ds_hf_create` checks its descriptor on the host: a shell with l = 3, an occupation that does not sum to the electron count,
    a NaN among the atoms, k points or images and a null handle come back as errors with a message, without a GPU."""
    import ctypes as C
    from deepsolid_amd import _lib
    lib = _lib.load()
    s = hh.lih_system()
    tables = t = s.gaussian_orbitals()._arrays()
    pd = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))

    def create(shell_l, nocc_up, poison=None):
        t = dict(tables)
        if poison:
            t[poison] = t[poison].copy()
            t[poison][1, 2] = np.nan
        keep = [np.ascontiguousarray(v) for v in (t['atoms'], t['shell_atom'], np.asarray(shell_l, np.int32), t['shell_nprim'], t['exps'],
                                                  t['coefs'], t['kpts'], t['images'], np.asarray(nocc_up, np.int32), t['nocc'][1],
                                                  t['mo_up'].view(np.float64), t['mo_dn'].view(np.float64))]
        d = _lib.HfDesc()
        d.a[:] = t['a'].reshape(-1).tolist()
        d.n_atoms, d.atoms, d.n_shells = 2, pd(keep[0]), len(shell_l)
        d.shell_atom, d.shell_l, d.shell_nprim, d.exps, d.coefs = pi(keep[1]), pi(keep[2]), pi(keep[3]), pd(keep[4]), pd(keep[5])
        d.n_k, d.kpts, d.n_images, d.images = 2, pd(keep[6]), keep[7].shape[0], pd(keep[7])
        d.n_up, d.n_dn, d.nocc_up, d.nocc_dn, d.mo_up, d.mo_dn = 4, 4, pi(keep[8]), pi(keep[9]), pd(keep[10]), pd(keep[11])
        h = C.c_void_p()
        rc = lib.ds_hf_create(C.byref(d), C.byref(h))
        return rc, lib.ds_last_error().decode(), h

    rc, msg, h = create([0, 0, 3, 0], [2, 2])
    assert rc != 0 and 'l = 3' in msg and not h
    rc, msg, h = create(t['shell_l'], [2, 1])
    assert rc != 0 and '3 occupied orbitals' in msg and not h
    for name in ('atoms', 'kpts', 'images'):
        rc, msg, h = create(t['shell_l'], [2, 2], poison=name)
        assert rc != 0 and f'{name}[1][2] is not finite' in msg and not h
    assert lib.ds_hf_orbitals(None, 0, None, 1, None, None, None) != 0
    lib.ds_hf_destroy(None)
