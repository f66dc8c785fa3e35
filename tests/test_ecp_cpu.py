"""CPU tests of the pseudopotential energy: the numpy model of ecp_helpers.py against exact statements -- the
degree of the two quadrature rules, the uniqueness of the minimum image, the closed-form angular integral of a plane-wave
determinant, the unbiasedness of the rotated rule -- and the host side of the package: `pseudopotential.SemiLocalECP` (validation,
cutoff search, save / load), the refusals of `ds_ecp_create` (which come before it touches a device) and the exported symbols."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import ecp_helpers as eh
import onebody_helpers as oh
import sampler_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ symbols
def test_header_and_library_have_the_ecp_symbols():
    from deepsolid_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    lib = _lib.load()
    for n in ('ds_ecp_create', 'ds_ecp_destroy', 'ds_ecp_workspace_bytes', 'ds_ecp_energy'):
        assert n + '(' in header, n
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f'{n} is not bound in _lib.py'
    assert 'typedef struct ds_ecp_desc' in header
    assert lib.ds_ecp_workspace_bytes(None, None, 4, 4) == -1


def test_auxiliary_data_gains_a_trailing_field_that_stays_out_of_the_way():
    """`pseudopotential` is the last field and defaults to None; the mapping of a loss without one holds the six fields it always
    held (the benchmark dumps every entry of it as an array)."""
    from deepsolid_amd import train
    assert train.AuxiliaryLossData._fields[-1] == 'pseudopotential' and len(train.AuxiliaryLossData._fields) == 7
    aux = train.AuxiliaryLossData(variance=1.0, local_energy=2.0, imaginary=3.0, kinetic=4.0, ewald=5.0)
    assert aux.pseudopotential is None and aux.n_nonfinite is None
    assert list(aux._asdict()) == ['variance', 'local_energy', 'imaginary', 'kinetic', 'ewald', 'n_nonfinite']
    assert list(aux._replace(pseudopotential=6.0)._asdict())[-1] == 'pseudopotential'
    assert type(aux)(*aux) == aux


# ------------------------------------------------------------------------------------------------ quadrature
def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return eh.quaternion_matrix(q[:, 0], q[:, 1], q[:, 2], q[:, 3])


def sphere_monomial(a, b, c):
    """int dOmega / (4 pi) x^a y^b z^c = prod (k - 1)!! / (a + b + c + 1)!! for even exponents, 0 otherwise."""
    if a % 2 or b % 2 or c % 2:
        return 0.0
    df = lambda k: float(np.prod(np.arange(k, 0, -2))) if k > 0 else 1.0
    return df(a - 1) * df(b - 1) * df(c - 1) / df(a + b + c + 1)


@pytest.mark.parametrize('n_quad,degree', [(6, 3), (12, 5)])
def test_rules_integrate_every_monomial_up_to_their_degree(n_quad, degree):
    """Equal weights 1 / N_q on the rotated points: exact to 1e-14 for every x^a y^b z^c with a + b + c <= degree, under 50 random
    rotations and under the Philox rotations of the kernel; the first degree beyond is NOT integrated (the rule is no better
    than stated)."""
    rots = np.concatenate([random_rotations(np.random.default_rng(3), 50), eh.replay_rotations(eh.SEED, eh.OFFSET, 50)])
    assert np.abs(np.einsum('wij,wkj->wik', rots, rots) - np.eye(3)).max() < 1e-14
    U = eh.rotated_points(rots, n_quad)
    assert U.shape == (100, n_quad, 3) and np.abs(np.linalg.norm(U, axis=2) - 1).max() < 1e-15
    worst = 0.0
    for a, b, c in itertools.product(range(degree + 1), repeat=3):
        if a + b + c > degree:
            continue
        got = (U[..., 0] ** a * U[..., 1] ** b * U[..., 2] ** c).mean(axis=1)
        worst = max(worst, np.abs(got - sphere_monomial(a, b, c)).max())
    print(f'N_q = {n_quad}: max error up to degree {degree} = {worst:.2e}')
    assert worst <= 1e-14
    beyond = max(np.abs((U[..., 0] ** a * U[..., 1] ** b * U[..., 2] ** c).mean(axis=1) - sphere_monomial(a, b, c)).max()
                 for a, b, c in itertools.product(range(degree + 2), repeat=3) if a + b + c == degree + 1)
    assert beyond > 1e-3


def test_point_sets_of_the_package_equal_the_model():
    from deepsolid_amd import pseudopotential as pp
    for n in (6, 12):
        assert np.array_equal(pp.quadrature_points(n), eh.points(n))
    ico = eh.points(12)
    assert np.allclose(ico[0] * np.sqrt(1 + ((1 + np.sqrt(5)) / 2) ** 2), [0, 1, (1 + np.sqrt(5)) / 2])
    assert np.allclose(ico[:6:1] + ico[[3, 2, 1, 0, 7, 6]], 0)               # antipodal pairs: (+,+) with (-,-), (+,-) with (-,+)
    with pytest.raises(ValueError):
        pp.quadrature_points(8)


# ------------------------------------------------------------------------------------------------ minimum image
def test_minimum_image_is_the_only_image_inside_half_the_smallest_height():
    """Random triclinic cells, random electron positions: among the 125 nearest images at most one lies below half the smallest
    height, and when one does it is the one the wrap picks; r >= |f_c| height_c holds for every image and component."""
    rng = np.random.default_rng(11)
    n_inside = 0
    for _ in range(40):
        a = np.diag(rng.uniform(3, 7, 3)) + rng.uniform(-1.5, 1.5, (3, 3))
        h = eh.heights(a)
        assert np.allclose(h, 1 / np.linalg.norm(np.linalg.inv(a), axis=0))
        atoms = rng.uniform(-5, 5, (3, 3))
        x = rng.uniform(-15, 15, (8, 12))
        r, d, _ = eh.min_image(x, atoms, a)
        shifts = np.asarray(list(itertools.product(range(-2, 3), repeat=3))) @ a
        img = d[..., None, :] + shifts                                            # (B, N, A, 125, 3)
        ri = np.linalg.norm(img, axis=-1)
        f = img @ np.linalg.inv(a)
        assert np.all(ri[..., None] >= np.abs(f) * h - 1e-12)
        inside = ri < 0.5 * h.min()
        assert inside.sum(axis=-1).max() <= 1
        zero = 62                                                                 # the shift (0, 0, 0)
        assert np.array_equal(inside.any(axis=-1), inside[..., zero])
        assert np.all(np.abs(d @ np.linalg.inv(a)) <= 0.5 + 1e-12)
        n_inside += int(inside.sum())
    assert n_inside > 50


def test_fixture_cases_have_the_counted_pairs_away_from_every_cutoff():
    for name in eh.CASES:
        for f32 in (False, True):
            fx = eh.fixture(name, 12, f32)
            assert fx['pairs']['counts'].tolist() == eh.CASES[name][1]
    assert eh.fixture('lih', 6)['pairs']['counts'].tolist() == eh.CASES['lih'][1]
    # electrons outside every sphere, as counted: 0-1 per walker on lih, 8-10 on bcc_li
    for name, lo, hi in (('lih', 0, 1), ('bcc_li', 8, 10)):
        fx = eh.fixture(name)
        N = fx['x'].shape[1] // 3
        outside = [N - len(set(fx['pairs']['i'][fx['pairs']['w'] == w])) for w in range(len(fx['x']))]
        assert lo <= min(outside) and max(outside) <= hi, (name, outside)


# ------------------------------------------------------------------------------------------------ SemiLocalECP
def lih_cell():
    return sh.case('lih')[1]


def test_validation_refuses_what_it_should():
    from deepsolid_amd.pseudopotential import SemiLocalECP, cell_heights
    cell = lih_cell()
    limit = 0.5 * cell_heights(cell.a).min()
    assert abs(limit - 2.182) < 1e-3
    good = dict(local=[(1, 1.0, -1.0)], channels=[[(2, 1.0, 1.0)], [(2, 1.0, 1.0)]], r_cut_loc=1.0, r_cut_nl=2.0)
    SemiLocalECP(cell, [good], [0, 0])
    cases = [
        ('cutoff', dict(good, r_cut_nl=limit + 1e-3), {}),
        ('cutoff', dict(good, r_cut_loc=limit + 1e-3), {}),
        ('n_quad', good, dict(n_quad=8)),
        ('n_l = 3', dict(good, channels=[[(2, 1.0, 1.0)]] * 3), dict(n_quad=6)),
        ('l = 3', dict(good, channels=[[(2, 1.0, 1.0)]] * 4), {}),
        ('n_l must be in 0..4', dict(good, channels=[[(2, 1.0, 1.0)]] * 5), {}),
        ('at most 16 terms', dict(good, local=[(2, 1.0, 1.0)] * 17), {}),
        ('n_k must be in 0..4', dict(good, local=[(5, 1.0, 1.0)]), {}),
        ('n_k must be in 0..4', dict(good, channels=[[(-1, 1.0, 1.0)]]), {}),
        ('not finite', dict(good, local=[(2, np.inf, 1.0)]), {}),
    ]
    for word, sp, kw in cases:
        with pytest.raises(ValueError, match=word):
            SemiLocalECP(cell, [sp], [0, 0], **kw)
    with pytest.raises(ValueError, match=r'atom 1 .*cutoff 2\.5.*limit is 2\.18'):     # names the atom, the cutoff and the limit
        SemiLocalECP(cell, [good, dict(good, r_cut_nl=2.5)], [0, 1])
    with pytest.raises(ValueError, match='atom_species'):
        SemiLocalECP(cell, [good], [0, 1])
    with pytest.raises(ValueError, match='atom_species'):
        SemiLocalECP(cell, [good], [0])
    SemiLocalECP(cell, [good], [0, 0], z_eff=cell.atom_charges())
    with pytest.raises(ValueError, match='z_eff'):
        SemiLocalECP(cell, [good], [0, 0], z_eff=[1, 1])
    # three channels run with 12 points, two with 6; a species without channels takes no cutoff from them
    assert SemiLocalECP(cell, [dict(good, channels=[[(2, 1.0, 1.0)]] * 3)], [0, 0]).n_l.tolist() == [3]
    assert SemiLocalECP(cell, [dict(local=[(2, 3.0, 1.0)], channels=[])], [0, 0]).r_cut_nl.tolist() == [0.0]
    by_name = SemiLocalECP(cell, dict(Li=good, H=dict(good, r_cut_nl=1.5)), ['Li', 'H'])
    assert by_name.atom_species.tolist() == [0, 1] and by_name.r_cut_nl.tolist() == [2.0, 1.5]


def test_library_repeats_the_creation_refusals_before_touching_a_device():
    """`ds_ecp_create` checks the descriptor before its first allocation: every refusal listed in the header comes back as a message,
    here without a GPU."""
    from deepsolid_amd import _lib, device
    lib = _lib.load()
    fx = eh.fixture('lih')
    ecp = fx['ecp']
    t = ecp.tables()
    bad_n = t['term_n'].copy()
    bad_n[0] = 5
    many = np.concatenate([[0], np.full(len(t['term_offset']) - 1, 17)]).astype(np.int32)
    cases = [
        ('n_quad must be 6 or 12', dict(n_quad=7)),
        ('cutoff', dict(r_cut_nl=[2.19, 1.0])),
        ('cutoff', dict(r_cut_loc=[1.0, 2.19])),
        ('n_l = 4', dict(n_l=[4, 2])),
        ('n_l must be in 0..4', dict(n_l=[5, 2])),
        ('n_l = 3', dict(n_l=[3, 2], n_quad=6)),
        ('n_k must be in 0..4', dict(term_n=bad_n)),
        ('at most 16 terms', dict(term_offset=many, term_n=np.full(17, 2), term_zeta=np.ones(17), term_c=np.ones(17))),
        ('names species', dict(atom_species=[0, 2])),
    ]
    for word, kw in cases:
        d, keep = device.ecp_desc(ecp, **kw)
        out = C.c_void_p()
        assert lib.ds_ecp_create(C.byref(d), C.byref(out)) != 0, kw
        msg = lib.ds_last_error().decode()
        assert word in msg, (kw, msg)
        assert not out.value
    d, keep = device.ecp_desc(ecp, r_cut_nl=[1.0, 2.5])
    assert lib.ds_ecp_create(C.byref(d), C.byref(C.c_void_p())) != 0
    msg = lib.ds_last_error().decode()
    assert 'atom 1' in msg and '2.5' in msg and '2.18' in msg, msg                    # the atom, the cutoff and the limit


def test_cutoff_search():
    """The smallest grid radius beyond which |v| <= tol on the whole grid up to 10 Bohr; for one Gaussian it is the grid point
    after sqrt(log(c / tol) / zeta)."""
    from deepsolid_amd.pseudopotential import SemiLocalECP, eval_radial, find_cutoff
    for c, z, tol in ((3.0, 1.1, 1e-5), (0.5, 4.0, 1e-5), (3.0, 1.1, 1e-3), (-2.0, 2.5, 1e-7)):
        rc = find_cutoff([(2, z, c)], tol)
        exact = np.sqrt(np.log(abs(c) / tol) / z)
        assert exact <= rc < exact + 1.001e-3, (rc, exact)
        assert abs(rc / 1e-3 - round(rc / 1e-3)) < 1e-6
    # a function with a node: the search looks from outside in and is not fooled by the sign change
    terms = [(2, 1.0, 1.0), (4, 1.0, -1.0)]                                           # (1 - r^2) exp(-r^2): zero at r = 1
    rc = find_cutoff(terms, 1e-5)
    grid = np.arange(1, 10001) * 1e-3
    v = np.abs(eval_radial(terms, grid))
    assert np.all(v[grid >= rc - 1e-9] <= 1e-5) and v[int(round(rc / 1e-3)) - 2] > 1e-5 and rc > 3
    assert find_cutoff([], 1e-5) == 0.0 and find_cutoff([(2, 1.0, 1e-6)], 1e-5) == 0.0
    with pytest.raises(ValueError, match='no cutoff'):
        find_cutoff([(1, 0.0, 1.0)], 1e-5)                                            # 1 / r: 0.1 Ha at 10 Bohr
    cell = sh.case('bcc_li')[1]
    found = SemiLocalECP(cell, [dict(local=[(2, 1.5, 2.0)], channels=[[(2, 1.1, 3.0)], [(2, 2.0, -1.0)]])], [0] * 8)
    assert found.r_cut_loc[0] == find_cutoff([(2, 1.5, 2.0)], 1e-5)
    assert found.r_cut_nl[0] == max(find_cutoff([(2, 1.1, 3.0)]), find_cutoff([(2, 2.0, -1.0)]))
    looser = SemiLocalECP(cell, [dict(local=[(2, 1.5, 2.0)], channels=[[(2, 1.1, 3.0)]])], [0] * 8, tol=1e-3)
    assert looser.r_cut_nl[0] < found.r_cut_nl[0]


def test_save_load_round_trip(tmp_path):
    from deepsolid_amd.pseudopotential import SemiLocalECP
    fx = eh.fixture('bcc_li')
    ecp = fx['ecp']
    path = str(tmp_path / 'ecp.npz')
    ecp.save(path)
    back = SemiLocalECP.load(path, fx['cell'])
    assert back.local == ecp.local and back.channels == ecp.channels and back.n_quad == ecp.n_quad and back.tol == ecp.tol
    for k in ('a', 'atoms', 'atom_species', 'r_cut_loc', 'r_cut_nl', 'n_l'):
        assert np.array_equal(getattr(back, k), getattr(ecp, k)), k
    for k, v in ecp.tables().items():
        assert np.array_equal(back.tables()[k], v), k
    r = np.linspace(0.1, 3, 7)
    assert np.array_equal(back.radial(1, 1, r), eh.radial(eh.SPECIES_B['channels'][1], r))
    assert np.array_equal(back.radial(0, 'loc', r), eh.radial(eh.SPECIES_A['local'], r))
    with pytest.raises(ValueError, match='another simulation cell'):
        SemiLocalECP.load(path, lih_cell())


# ------------------------------------------------------------------------------------------------ closed form
def plane_wave_walkers(n_quad):
    """lih fixture walkers with electron 0 of walker w put at distance RADII[w] from atom 0: pairs from k r = 0.4 to 4.8."""
    fx = eh.fixture('lih', n_quad)
    rng = np.random.default_rng(2)
    x = np.array(fx['x'])
    radii = [0.15, 0.3, 0.5, 0.8, 1.2, 1.8]
    for w, r in enumerate(radii):
        n = rng.standard_normal(3)
        x[w, 0:3] = fx['ecp'].atoms[0] + r * n / np.linalg.norm(n)
    return x, fx['ecp'], radii


@pytest.mark.parametrize('n_quad,degree', [(12, 5), (6, 3)])
def test_plane_wave_determinant_meets_the_exact_angular_integral(n_quad, degree):
    """Plane-wave determinant of onebody_helpers on the LiH cell, potential of ecp_helpers (cutoff 2.18 Bohr), occupied k up to
    |k| = 2.67 / Bohr.  Per pair, |model - exact| is within the a-priori error of the rule (docstring of
    ecp_helpers.plane_wave_exact_terms: sum_l |(2l + 1) v_l| sum_j |c_j| sum_{L > D - l} (2L + 1) |j_L(k_j r)|) for every one of 20
    Philox rotations.  Measured here from the model, largest error over the rotations / that bound, for the pair of the electron put
    at r = 0.15, 0.3, 0.5, 0.8, 1.2, 1.8 Bohr:
        N_q = 12:  5.7e-06 / 4.5e-05,  7.2e-05 / 6.6e-04,  5.7e-04 / 4.9e-03,  4.5e-03 / 5.0e-02,  6.3e-03 / 8.0e-02,  6.6e-03 / 1.0e-01
        N_q = 6:   2.6e-04 / 1.1e-03,  1.1e-03 / 5.8e-03,  5.2e-03 / 3.6e-02,  3.7e-02 / 2.4e-01,  3.6e-02 / 2.2e-01,  1.5e-02 / 1.3e-01
    (Ha; the radial functions fall beyond 1 Bohr, so the last entries do not grow.)  The error follows the bound over three orders
    of magnitude, which a wrong weight, point or Legendre polynomial would not."""
    fxl, cell, klist, _, _ = sh.case('lih')
    pw_klist, _, _, _, _ = oh.plane_wave_case(cell, klist)
    nelec = (2, 2)
    x, ecp, radii = plane_wave_walkers(n_quad)
    pl = eh.pair_list(ecp, x)
    exact, bound = eh.plane_wave_exact_terms(x, pl, ecp, pw_klist, nelec)
    b = bound(degree)
    worst = np.zeros(len(exact))
    for k in range(20):
        rot = eh.replay_rotations(eh.SEED, k, len(x))
        q = eh.plane_wave_config_ratios(x, pl, rot, n_quad, pw_klist, nelec)
        model = (eh.weights(ecp, pl, rot, n_quad) * n_quad * q.reshape(-1, n_quad)).mean(axis=1)
        worst = np.maximum(worst, np.abs(model - exact))
    placed = [int(np.nonzero((pl['w'] == w) & (pl['i'] == 0) & (pl['I'] == 0))[0][0]) for w in range(len(radii))]
    print(f'N_q = {n_quad}: ' + ',  '.join(f'{worst[p]:.1e} / {b[p]:.1e}' for p in placed))
    assert np.all(worst <= b + 1e-13 * np.abs(exact).max())
    assert b[placed[0]] < 2e-3 * np.abs(exact[placed[0]])                         # the bound bites where k r is small
    assert worst[placed[-1]] > 1e-3                                               # ... and the rule IS inexact where it is large


def test_mean_over_philox_rotations_approaches_the_exact_value():
    """A rotated equal-weight rule is exact in expectation: for the pair at r = 1.8 Bohr (6 points, visibly inexact per rotation)
    the mean over n Philox rotations is within 5 standard errors of the exact integral for n = 100, 1600, 25600, and the standard
    error falls as 1 / sqrt(n) by construction."""
    fxl, cell, klist, _, _ = sh.case('lih')
    pw_klist, _, _, _, _ = oh.plane_wave_case(cell, klist)
    x, ecp, radii = plane_wave_walkers(6)
    pl = eh.pair_list(ecp, x)
    p = int(np.nonzero((pl['w'] == 5) & (pl['i'] == 0) & (pl['I'] == 0))[0][0])
    one = {k: v[p:p + 1] for k, v in pl.items() if k != 'counts'}
    one['w'] = np.zeros(1, dtype=int)
    exact, _ = eh.plane_wave_exact_terms(x[5:6], one, ecp, pw_klist, (2, 2))
    n = 25600
    rots = eh.replay_rotations(eh.SEED, 7, n)
    # the same pair under every rotation: walker index = rotation index
    many = {k: np.repeat(v, n, axis=0) for k, v in one.items()}
    many['w'] = np.arange(n)
    U = eh.rotated_points(rots, 6)
    s = -one['d'][0][None, None, :] + one['r'][0] * U                             # (n, 6, 3)
    k = np.asarray(pw_klist[0], dtype=np.float64)
    rr = x[5].reshape(4, 3)
    mat = np.exp(1j * rr[:2] @ k.T)
    coef = mat[0] * np.linalg.inv(mat)[:, 0]
    q = np.einsum('nqj,j->nq', np.exp(1j * np.einsum('nqc,jc->nqj', s, k)), coef)
    vals = (eh.weights(ecp, many, rots, 6) * q).sum(axis=1)
    assert np.abs(vals - exact[0]).max() > 1e-2
    for m in (100, 1600, 25600):
        err = abs(vals[:m].mean() - exact[0])
        se = np.sqrt((vals[:m].real.var() + vals[:m].imag.var()) / m)
        print(f'n = {m}: |mean - exact| = {err:.2e}, standard error {se:.2e}')
        assert err <= 5 * se
    assert se < 1e-3
