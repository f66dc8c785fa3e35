"""CPU checks of the walker observables (deepsolid_amd/estimator.py, reference DeepSolid/estimator.py): the q-grid order and
the packed-sum -> (P, S(k)) algebra against tests/golden/estimators.npz (made by tools/make_estimator_golden.py, which
executes the reference's estimator.py), the 2-rank combination over gloo, the structure_factor.csv row format against pandas,
and the host side of the `ds_observables` C ABI (symbols, workspace size, argument errors -- all answered before any launch).
Also the long-double reference, the a-priori error bound and the point lists that tests/test_gpu_estimator.py uses above 64
electrons, with a float64 replay of the kernel's recurrence that keeps the bound checkable without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepsolid_amd import estimator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'estimators.npz')
CELLS = ('lih', 'bcc_li', 'graphene', 'h_chain')


def fixture():
    return dict(np.load(GOLDEN))


def recvec(a):
    return 2 * np.pi * np.linalg.inv(a).T


def np_sums(x, rv, grid, pol_dir):
    """float64 numpy restatement of the packed batch sums of `ds_observables` (exp(i q.r) evaluated directly)."""
    B = x.shape[0]
    r = np.asarray(x, dtype=np.float64).reshape(B, -1, 3)
    Q = grid.shape[0]
    out = np.zeros(2 + 3 * Q)
    if pol_dir >= 0:
        ph = (r @ rv[pol_dir]).sum(axis=1)
        out[0], out[1] = np.cos(ph).sum(), np.sin(ph).sum()
    if Q:
        rho = np.exp(1j * (r @ (grid @ rv).T)).sum(axis=1)          # (B, Q)
        out[2:2 + Q] = rho.real.sum(axis=0)
        out[2 + Q:2 + 2 * Q] = rho.imag.sum(axis=0)
        out[2 + 2 * Q:] = (np.abs(rho) ** 2).sum(axis=0)
    return out


# ----------------------------------------------------------------------------- beyond one 64-electron chunk, general point lists
TRICLINIC = np.array([[7.0, 0.3, 0.0], [0.2, 8.0, 0.5], [-1.0, 0.4, 9.0]])
U = 2.0 ** -53


def cell_walkers(n_elec, batch, seed=0):
    """(batch, 3 n_elec) float64 walkers of the triclinic cell, uniform over the cells -3 .. +4 in every direction."""
    rng = np.random.default_rng(100000 * seed + 1000 * n_elec + batch)
    return (rng.uniform(-3.0, 4.0, size=(batch, n_elec, 3)) @ TRICLINIC).reshape(batch, 3 * n_elec)


def point_lists():
    """name -> (Q, 3) int32 lattice coordinates:
    cubic8   the 8^3 grid, 512 points: 8 points per lane;
    box720   150 points drawn (with repeats) from n1 <= 7, n2 <= 2, n3 = 0: three points per lane (the kernel instance of four),
             a different largest power in every direction, the table depth 8 set by direction 1 alone;
    box111   130 points drawn from the eight with all coordinates <= 1: table depth 2;
    origin   the single point (0, 0, 0): rho = N."""
    rng = np.random.default_rng(720)
    box720 = np.stack([rng.integers(0, 8, 150), rng.integers(0, 3, 150), np.zeros(150, np.int64)], axis=1)
    box720[:3] = [[7, 0, 0], [0, 2, 0], [7, 2, 0]]
    box111 = rng.integers(0, 2, size=(130, 3))
    box111[:2] = [[1, 1, 1], [0, 0, 0]]
    return {'cubic8': estimator.structure_factor_grid(8), 'box720': box720.astype(np.int32), 'box111': box111.astype(np.int32),
            'origin': np.zeros((1, 3), np.int32)}


def ld_sums(x, rv, grid, pol_dir):
    """`np_sums` in np.longdouble (64-bit significand here), whose own rounding is 2^-11 of float64's -> (packed sums, rho (B, Q)).
    exp(i q.r) is taken as the product over the three directions of exp(i n_j g_j.r), every factor a direct long-double sincos
    of n_j (g_j.r): the same number, at 24 sincos per electron instead of Q.  The electron sum runs over every (n1, n2, n3)
    below the list's largest coordinate as one long-double matrix product, and the list's points are read out of that."""
    LD = np.longdouble
    B = x.shape[0]
    r = np.asarray(x, dtype=np.float64).reshape(B, -1, 3).astype(LD)
    th = r @ np.asarray(rv, dtype=np.float64).astype(LD).T            # (B, N, 3): g_j . r
    Q = grid.shape[0]
    out = np.zeros(2 + 3 * Q, dtype=LD)
    rho = np.zeros((B, Q), dtype=np.clongdouble)
    if pol_dir >= 0:
        ph = th[:, :, pol_dir].sum(axis=1)
        out[0], out[1] = np.cos(ph).sum(), np.sin(ph).sum()
    if Q:
        ang = th[..., None] * np.arange(int(grid.max()) + 1).astype(LD)      # (B, N, 3, n)
        z = np.cos(ang) + 1j * np.sin(ang)
        n1, n2, n3 = (int(m) + 1 for m in grid.max(axis=0))
        for b0 in range(0, B, 64):                                   # every point of the list's box once, then the list's points
            zb = z[b0:b0 + 64]
            w = (zb[:, :, 0, :n1, None] * zb[:, :, 1, None, :n2]).reshape(zb.shape[0], -1, n1 * n2)
            full = np.matmul(w.transpose(0, 2, 1), zb[:, :, 2, :n3])         # (64, n1 n2, n3): the sum over the electrons
            rho[b0:b0 + 64] = full[:, grid[:, 0] * n2 + grid[:, 1], grid[:, 2]]
        out[2:2 + Q] = rho.real.sum(axis=0)
        out[2 + Q:2 + 2 * Q] = rho.imag.sum(axis=0)
        out[2 + 2 * Q:] = (rho.real ** 2 + rho.imag ** 2).sum(axis=0)
    return out, rho


def sums_bound(x, rv, grid, pol_dir, rho):
    """A-priori bound on |device - exact| of every packed sum of `ds_observables`, u = 2^-53, A_je = sum_k |g_jk| |r_ek|.
    One term exp(i q.r_e) of the point (n1, n2, n3):  eps = u (8 sum_j n_j A_je + 64)  -- the three-product dot amplified by n_j,
    and 64 for the sincos and at most 7 + 2 complex multiplications.
    Re rho_b, Im rho_b:  d_b = sum_e eps + N^2 u  (any summation order).   Batch sums: sum_b d_b + B u sum_b |rho_b|.
    |rho|^2:  sum_b (2 |rho_b| d_b + d_b^2) + B u sum_b |rho_b|^2.
    Polarization: phase error u (N + 4) sum_e A_pe, |dP_b| <= that + 4 u, and B^2 u for the batch sum.
    `rho` (B, Q): the exact per-walker rho of `ld_sums`."""
    B = x.shape[0]
    r = np.abs(np.asarray(x, dtype=np.float64).reshape(B, -1, 3))
    N, Q = r.shape[1], grid.shape[0]
    A = (r @ np.abs(np.asarray(rv, dtype=np.float64)).T).sum(axis=1)         # (B, 3): sum_e A_je
    out = np.zeros(2 + 3 * Q)
    if pol_dir >= 0:
        out[0] = out[1] = (U * (N + 4) * A[:, pol_dir] + 4 * U).sum() + B * B * U
    if Q:
        mag = np.abs(rho).astype(np.float64)
        d = U * (8 * A @ grid.T.astype(np.float64) + 64 * N) + N * N * U     # (B, Q)
        out[2:2 + Q] = out[2 + Q:2 + 2 * Q] = d.sum(axis=0) + B * U * mag.sum(axis=0)
        out[2 + 2 * Q:] = (2 * mag * d + d * d).sum(axis=0) + B * U * (mag ** 2).sum(axis=0)
    return out


def ratio_to_bound(got, ref, bound):
    """max |got - ref| / bound over the packed sums; an entry whose bound is 0 (no polarization asked) must be exact."""
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def replay_sums(x, rv, grid, pol_dir):
    """float64 numpy replay of k_obs_partial's arithmetic: the three-product dot, one sincos per direction, the powers by
    repeated multiplication, (z1^n1 z2^n2) z3^n3 out of the table, the electrons added one after the other (here in index order; the kernel orders a
    chunk's electrons by their coordinates, and the bound holds for any order)."""
    B = x.shape[0]
    r = np.asarray(x, dtype=np.float64).reshape(B, -1, 3)
    N, Q = r.shape[1], grid.shape[0]
    d = np.stack([rv[c, 0] * r[..., 0] + rv[c, 1] * r[..., 1] + rv[c, 2] * r[..., 2] for c in range(3)], axis=-1)
    out = np.zeros(2 + 3 * Q)
    if pol_dir >= 0:
        ph = d[:, :, pol_dir].sum(axis=1)
        out[0], out[1] = np.cos(ph).sum(), np.sin(ph).sum()
    if Q:
        z = np.cos(d) + 1j * np.sin(d)
        n_pow = int(grid.max()) + 1
        tab = np.empty((B, N, 3, n_pow), dtype=np.complex128)
        w = np.ones_like(z)
        for p in range(n_pow):
            tab[..., p] = w
            w = w * z
        rho = np.zeros((B, Q), dtype=np.complex128)
        for e in range(N):
            rho += tab[:, e, 0, grid[:, 0]] * tab[:, e, 1, grid[:, 1]] * tab[:, e, 2, grid[:, 2]]
        out[2:2 + Q] = rho.real.sum(axis=0)
        out[2 + Q:2 + 2 * Q] = rho.imag.sum(axis=0)
        out[2 + 2 * Q:] = (rho.real ** 2 + rho.imag ** 2).sum(axis=0)
    return out


@pytest.mark.parametrize('n_elec', [65, 96, 128])
def test_sums_bound_holds_for_a_float64_replay(n_elec):
    """The bound of `sums_bound`, which the GPU tests assert, is checkable without a GPU: a float64 replay of the kernel's
    recurrence stays inside it against the long-double reference, on every point list and polarization direction.
    Worst ratio: 8.2e-3 (N = 65, the 8^3 grid), 7.5e-3 on the 150-point list, 4.1e-3 on the 130-point list, 0 on the origin."""
    rv = recvec(TRICLINIC)
    x = cell_walkers(n_elec, 5)
    worst = 0.0
    for pol_dir, (name, grid) in zip((0, 1, 2, -1), point_lists().items()):
        ref, rho = ld_sums(x, rv, grid, pol_dir)
        ratio = ratio_to_bound(replay_sums(x, rv, grid, pol_dir), ref, sums_bound(x, rv, grid, pol_dir, rho))
        print(f'replay N={n_elec} {name} pol={pol_dir}: max err / bound = {ratio:.3e}')
        worst = max(worst, ratio)
    assert worst <= 1.0


def test_grid_order_matches_reference_meshgrid():
    """jnp.meshgrid indexes 'xy': point p = i nq^2 + j nq + k is (n1, n2, n3) = (j, i, k)."""
    for nq in (1, 2, 3, 4, 8):
        g = estimator.structure_factor_grid(nq)
        assert g.shape == (nq ** 3, 3) and g.dtype == np.int32
        for i in range(nq):
            for j in range(nq):
                for k in range(nq):
                    assert tuple(g[i * nq * nq + j * nq + k]) == (j, i, k)
    g = estimator.structure_factor_grid(4)
    assert tuple(g[1]) == (0, 0, 1) and tuple(g[4]) == (1, 0, 0) and tuple(g[16]) == (0, 1, 0)


@pytest.mark.parametrize('name', CELLS)
def test_packed_sums_algebra_against_reference(name):
    fx = fixture()
    x, a = fx[f'{name}_x'], fx[f'{name}_a']
    nelec = int(fx[f'{name}_nelec'].sum())
    rv = recvec(a)
    for d in (0, 1, 2):
        sums = torch.as_tensor(np_sums(x, rv, np.zeros((0, 3), np.int32), d))
        pol, sk = estimator.combine_sums(sums, x.shape[0], 0, True, nelec)
        assert sk is None and pol.dtype == torch.complex128
        assert abs(complex(pol) - complex(fx[f'{name}_pol{d}'])) < 1e-12
    for nq in range(1, 9):
        grid = estimator.structure_factor_grid(nq)
        sums = torch.as_tensor(np_sums(x, rv, grid, 1))
        pol, sk = estimator.combine_sums(sums, x.shape[0], grid.shape[0], True, nelec)
        assert sk.dtype == torch.float64 and sk.shape == (nq ** 3,)
        np.testing.assert_allclose(sk.numpy(), fx[f'{name}_sk{nq}'], rtol=0, atol=1e-10)
        assert abs(complex(pol) - complex(fx[f'{name}_pol1'])) < 1e-12
        _, sk32 = estimator.combine_sums(sums, x.shape[0], grid.shape[0], False, nelec, torch.float32)
        assert sk32.dtype == torch.float32


def test_no_reduction_at_world_size_one(monkeypatch):
    from deepsolid_amd import constants
    calls = []
    monkeypatch.setattr(constants.dist, 'all_reduce', lambda t, **kw: calls.append(t.numel()))
    sums = torch.arange(2 + 3 * 8, dtype=torch.float64)
    estimator.combine_sums(sums, 4, 8, True, 4)
    assert calls == [] and constants.world_size() == 1


def test_two_rank_combination_over_gloo(tmp_path):
    """Each rank holds half of the fixture walkers and its own batch sums; one packed all-reduce of the per-rank means per
    call, carrying only the requested observables, reproduces the reference's pmean(<rho>), pmean(<|rho|^2>) algebra."""
    script = tmp_path / 'worker.py'
    script.write_text('''
import sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from deepsolid_amd import constants, estimator
from test_estimator_cpu import fixture, np_sums, recvec
dist.init_process_group('gloo')
r = dist.get_rank()
sizes = []
orig = dist.all_reduce
def recording(t, *a, **k):
    sizes.append(t.numel())
    return orig(t, *a, **k)
constants.dist.all_reduce = recording
fx = fixture()
for name in ('lih', 'bcc_li', 'graphene', 'h_chain'):
    x_all = fx[name + '_x']
    half = x_all.shape[0] // 2
    x = x_all[r * half:(r + 1) * half]
    nelec = int(fx[name + '_nelec'].sum())
    rv = recvec(fx[name + '_a'])
    grid = estimator.structure_factor_grid(4)
    Q = grid.shape[0]
    sums = torch.as_tensor(np_sums(x, rv, grid, 0))
    del sizes[:]
    pol, sk = estimator.combine_sums(sums, half, Q, True, nelec)
    assert sizes == [2 + 3 * Q], sizes
    assert abs(complex(pol) - complex(fx[name + '_pol0'])) < 1e-12
    np.testing.assert_allclose(sk.numpy(), fx[name + '_sk4'], rtol=0, atol=1e-10)
    del sizes[:]
    pol1, sk1 = estimator.combine_sums(sums, half, 0, True, nelec)
    assert sizes == [2] and sk1 is None and complex(pol1) == complex(pol)
    del sizes[:]
    pol2, sk2 = estimator.combine_sums(sums, half, Q, False, nelec)
    assert sizes == [3 * Q] and pol2 is None and torch.equal(sk2, sk)
dist.destroy_process_group()
print('rank', r, 'ok')
''' % (ROOT, os.path.join(ROOT, 'tests')))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                          '--master-addr', '127.0.0.1', '--master-port', '29547', str(script)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count('ok') == 2


def test_per_rank_structure_factors_would_differ():
    """Why the ranks reduce <rho> and <|rho|^2> and not S(k): the mean of the halves' S(k) is a different number."""
    fx = fixture()
    x, nelec, rv = fx['bcc_li_x'], 24, recvec(fx['bcc_li_a'])
    grid = estimator.structure_factor_grid(4)
    halves = [estimator.combine_sums(torch.as_tensor(np_sums(x[h * 24:(h + 1) * 24], rv, grid, -1)), 24, 64, False, nelec)[1]
              for h in (0, 1)]
    assert np.abs(0.5 * (halves[0] + halves[1]).numpy() - fx['bcc_li_sk4']).max() > 1e-4


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_structure_factor_row_matches_pandas(tmp_path, dtype):
    pd = pytest.importorskip('pandas')
    fx = fixture()
    rng = np.random.default_rng(5)
    rows = [fx['graphene_sk4'].astype(dtype), fx['lih_sk8'].astype(dtype)[:64],
            (rng.normal(size=64) * 10.0 ** rng.integers(-20, 20, size=64)).astype(dtype),
            np.array([0.0, -0.0, 1.0, 1e16, 1e-5, 1e-4, np.inf, -np.inf, np.nan, 123456.789], dtype=dtype)]
    a, b = tmp_path / 'pandas.csv', tmp_path / 'ours.csv'
    for sk in rows:
        pd.DataFrame(sk[None, :]).to_csv(str(a), mode='a', sep=',', header=False)
        estimator.append_structure_factor_row(str(b), sk)
        estimator.append_structure_factor_row(str(b) + '.t', torch.as_tensor(sk))
    assert a.read_text() == b.read_text() == open(str(b) + '.t').read()
    assert b.read_text().splitlines()[0].startswith('0,')


def test_observables_off_keeps_the_schema():
    from deepsolid_amd import inference, systems
    cell, _ = systems.build('lih')
    schema, observe = inference._observables(cell, False, False, 4, None)
    assert schema == inference.TRAIN_SCHEMA and observe is None
    schema, observe = inference._observables(cell, True, True, 4, None)
    assert schema == inference.TRAIN_SCHEMA + ['complex_polarization'] and observe is not None
    schema, _ = inference._observables(cell, False, True, 4, None)
    assert schema == inference.TRAIN_SCHEMA


def test_factory_argument_errors():
    from deepsolid_amd import systems
    cell, _ = systems.build('lih')
    with pytest.raises(ValueError, match='ndim'):
        estimator.make_structure_factor(cell, ndim=2)
    with pytest.raises(ValueError, match='nq'):
        estimator.make_structure_factor(cell, nq=9)
    with pytest.raises(ValueError, match='direction'):
        estimator.make_complex_polarization(cell, direction=3)


# ----------------------------------------------------------------------------- C ABI (host side)
def _lib():
    from deepsolid_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L, L.load()


def test_cabi_exports_observables():
    L, lib = _lib()
    for name in ('ds_observables', 'ds_observables_workspace_bytes'):
        assert hasattr(lib, name) and name in L.SIGNATURES
    hdr = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    assert 'int ds_observables(' in hdr and 'int64_t ds_observables_workspace_bytes(' in hdr


def test_cabi_workspace_bytes():
    _, lib = _lib()
    assert lib.ds_observables_workspace_bytes(4096, 64) == 1024 * (2 + 3 * 64) * 8
    assert lib.ds_observables_workspace_bytes(10, 0) == 10 * 2 * 8
    assert lib.ds_observables_workspace_bytes(0, 64) < 0
    assert lib.ds_observables_workspace_bytes(10, 513) < 0


def test_cabi_argument_errors_without_a_launch():
    """Every bad argument is answered by ds_last_error before anything touches a device."""
    _, lib = _lib()
    rv = np.ascontiguousarray(recvec(np.eye(3) * 5.0))
    prv = rv.ctypes.data_as(C.POINTER(C.c_double))
    grid = estimator.structure_factor_grid(4)
    bad = grid.copy()
    bad[5, 2] = 8
    fake = C.c_void_p(0x1000)           # never dereferenced: every call below fails validation first

    def call(rvp=prv, dtype=0, x=fake, B=4, n=4, q=grid, n_q=None, pol=0, out=fake, ws=fake, ws_bytes=1 << 20):
        qa = np.ascontiguousarray(q if q is not None else np.zeros((0, 3)), dtype=np.int32)
        qp = qa.ctypes.data_as(C.POINTER(C.c_int32)) if q is not None else None
        rc = lib.ds_observables(rvp, dtype, x, B, n, qp, qa.shape[0] if n_q is None else n_q, pol, out, ws, ws_bytes, None)
        return rc, lib.ds_last_error().decode()

    cases = [(dict(rvp=None), 'null argument'), (dict(x=None), 'null argument'), (dict(out=None), 'null argument'),
             (dict(ws=None), 'null argument'), (dict(dtype=2), 'dtype'), (dict(B=0), 'B must be'),
             (dict(n=0), 'n_elec'), (dict(n=129), 'n_elec'), (dict(n_q=513), 'n_q'), (dict(n_q=-1), 'n_q'),
             (dict(q=None, n_q=3), 'q_int'), (dict(pol=3), 'pol_direction'), (dict(pol=-2), 'pol_direction'),
             (dict(ws_bytes=100), 'workspace too small'), (dict(q=bad), 'outside 0..7'), (dict(q=-grid - 1), 'outside 0..7')]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
    rv_nan = rv.copy()
    rv_nan[1, 1] = np.nan
    rc, err = call(rvp=rv_nan.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc != 0 and 'not finite' in err
