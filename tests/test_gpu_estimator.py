"""GPU checks of the walker observables (`ds_observables`, csrc/ds_obs.h, through deepsolid_amd.estimator) against the
reference-executed fixture tests/golden/estimators.npz and a float64 numpy restatement, and of the driver switches
(process.py:277-283, 337-342, 361-362).

float32 tolerance: the kernel widens float32 walkers to float64 and does all its arithmetic in float64, so against a float64
evaluation AT THE SAME (float32-rounded) walkers the only float32 step is the final rounding of each result: |dS| <= 2^-24 |S|
for S(k), and 2^-24 |P| per component for the complex64 polarization (plus the float64 noise, 1e-12 here).

The fixture cells hold at most 48 electrons and every grid above is cubic.  The second half of the module takes
`device.observable_sums` beyond that: 63 .. 128 electrons (a second 64-electron chunk in k_obs_partial), a triclinic cell with
walkers several cells out, more walkers than workgroups, and point lists that are no grid, against a long-double reference
and an a-priori bound (test_estimator_cpu.ld_sums, sums_bound)."""
import numpy as np
import pytest
import torch

from deepsolid_amd import device, estimator, systems

from test_estimator_cpu import (CELLS, TRICLINIC, U, cell_walkers, fixture, ld_sums, np_sums, point_lists, ratio_to_bound, recvec,
                                sums_bound)

pytestmark = pytest.mark.gpu


class _Cell:
    def __init__(self, a, nelec):
        self.a = np.asarray(a, dtype=np.float64)
        self.nelec = tuple(int(n) for n in nelec)
        self.nelectron = sum(self.nelec)

    def reciprocal_vectors(self):
        return 2 * np.pi * np.linalg.inv(self.a).T


def _cell(fx, name):
    return _Cell(fx[f'{name}_a'], fx[f'{name}_nelec'])


@pytest.mark.parametrize('name', CELLS)
def test_fixture_cells_f64(name):
    fx = fixture()
    cell = _cell(fx, name)
    x = torch.as_tensor(fx[f'{name}_x'], device='cuda')
    for d in (0, 1, 2):
        pol = estimator.make_complex_polarization(cell, direction=d)(x)
        assert pol.dtype == torch.complex128 and pol.dim() == 0
        assert abs(complex(pol) - complex(fx[f'{name}_pol{d}'])) < 1e-10
    for nq in range(1, 9):
        sk = estimator.make_structure_factor(cell, nq=nq)(x)
        assert sk.dtype == torch.float64 and sk.shape == (nq ** 3,) and sk.is_cuda
        np.testing.assert_allclose(sk.cpu().numpy(), fx[f'{name}_sk{nq}'], rtol=0, atol=1e-10)
    pol, sk = estimator.make_observables(cell, polarization_direction=2, nq=4)(x)
    assert abs(complex(pol) - complex(fx[f'{name}_pol2'])) < 1e-10
    np.testing.assert_allclose(sk.cpu().numpy(), fx[f'{name}_sk4'], rtol=0, atol=1e-10)


def test_bcc_li_headline_batch_against_numpy():
    """4096 walkers of the 24-electron bcc-Li cell: more walkers than workgroups (1024), so every workgroup visits several."""
    cell, _ = systems.build('bcc_li')
    x = systems.synthetic_walkers(cell, 4096, seed=77)
    grid = estimator.structure_factor_grid(4)
    rv = cell.reciprocal_vectors()
    ref = np_sums(x, rv, grid, 0)
    got = device.observable_sums(rv, torch.as_tensor(x, device='cuda'), grid, 0).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-8)
    pol, sk = estimator.make_observables(cell, polarization_direction=0, nq=4)(torch.as_tensor(x, device='cuda'))
    pol_ref, sk_ref = estimator.combine_sums(torch.as_tensor(ref), 4096, 64, True, 24)
    assert abs(complex(pol) - complex(pol_ref)) < 1e-12
    np.testing.assert_allclose(sk.cpu().numpy(), sk_ref.numpy(), rtol=0, atol=1e-10)


@pytest.mark.parametrize('name', ['bcc_li', 'graphene'])
def test_float32_walkers(name):
    fx = fixture()
    cell = _cell(fx, name)
    x32 = torch.as_tensor(fx[f'{name}_x'], dtype=torch.float32, device='cuda')
    x64 = x32.double()                        # the same rounded walkers
    for nq in (3, 4, 8):
        pol32, sk32 = estimator.make_observables(cell, polarization_direction=1, nq=nq)(x32)
        pol64, sk64 = estimator.make_observables(cell, polarization_direction=1, nq=nq)(x64)
        assert sk32.dtype == torch.float32 and pol32.dtype == torch.complex64
        s64 = sk64.cpu().numpy()
        assert np.all(np.abs(sk32.cpu().numpy().astype(np.float64) - s64) <= 2.0 ** -24 * np.abs(s64) + 1e-12)
        p32, p64 = complex(pol32), complex(pol64)
        assert abs(p32.real - p64.real) <= 2.0 ** -24 * abs(p64.real) + 1e-12
        assert abs(p32.imag - p64.imag) <= 2.0 ** -24 * abs(p64.imag) + 1e-12
        rv = recvec(fx[f'{name}_a'])
        ref = np_sums(x64.cpu().numpy(), rv, estimator.structure_factor_grid(nq), 1)
        np.testing.assert_allclose(device.observable_sums(rv, x32, estimator.structure_factor_grid(nq), 1).cpu().numpy(), ref,
                                   rtol=1e-12, atol=1e-9)


def test_two_calls_bit_identical():
    cell, _ = systems.build('graphene')
    x = torch.as_tensor(systems.synthetic_walkers(cell, 3000, seed=5), device='cuda')
    rv, grid = cell.reciprocal_vectors(), estimator.structure_factor_grid(8)
    a = device.observable_sums(rv, x, grid, 0)
    b = device.observable_sums(rv, x, grid, 0)
    assert torch.equal(a, b)
    c = device.observable_sums(rv, x.float(), grid, 0)
    assert torch.equal(c, device.observable_sums(rv, x.float(), grid, 0))


# ----------------------------------------------------------------------------- beyond one 64-electron chunk, general point lists
# k_obs_partial walks a walker's electrons in chunks of 64 and reuses one LDS table between barriers; the fixture cells stop at 48
# electrons and cubic grids.  Here: N = 63 .. 128 (one chunk, a full one, a second chunk of 1, 32, 63 and 64 electrons), a
# triclinic cell with walkers -3 .. +4 cells out, B = 1030 walkers on 1024 workgroups, and the point lists of
# test_estimator_cpu.point_lists (8, 3 and 1 points per lane; a different largest power per direction).  The reference is
# `ld_sums` (long double), the bound `sums_bound` (a priori; a float64 replay of the kernel's recurrence is held to it on the
# CPU).  float32 walkers are widened on load, so they are compared at their rounded values with the same bound.
NS = [63, 64, 65, 96, 127, 128]
POLS = (0, 1, 2, -1)                 # one direction per point list, in the order of `point_lists`


def _walkers(n_elec, batch, dtype, seed=0):
    """(device tensor of `dtype`, its values in float64)"""
    x = torch.as_tensor(cell_walkers(n_elec, batch, seed), dtype=getattr(torch, dtype))
    return x.cuda(), x.double().numpy()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('batch', [1, 5, 1030])
@pytest.mark.parametrize('n_elec', NS)
def test_above_64_electrons_against_long_double(n_elec, batch, dtype, record_property):
    """Every packed sum within `sums_bound` of the long-double reference.  A point that occurs twice in a list sits in two lanes
    (or two registers of one lane) and must come out with the same bits.
    Measured on the MI355X: at most 0.020 of the bound (N = 63, B = 1, the 8^3 grid); 0.018 on the 150-point list, 0.0081 on the
    130-point list, 0 on the origin.  The bound is a worst case over the electrons and the walkers; the errors add as a random
    walk."""
    rv = recvec(TRICLINIC)
    xd, x = _walkers(n_elec, batch, dtype)
    worst = 0.0
    for pol_dir, (name, grid) in zip(POLS, point_lists().items()):
        Q = grid.shape[0]
        got = device.observable_sums(rv, xd, grid, pol_dir).cpu().numpy()
        assert got.shape == (2 + 3 * Q,) and np.isfinite(got).all()
        ref, rho = ld_sums(x, rv, grid, pol_dir)
        ratio = ratio_to_bound(got, ref, sums_bound(x, rv, grid, pol_dir, rho))
        print(f'obs N={n_elec} B={batch} {dtype} {name} pol={pol_dir}: max err / bound = {ratio:.3e}')
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
        _, first, inverse = np.unique(grid, axis=0, return_index=True, return_inverse=True)
        same = first[inverse.reshape(-1)]                              # the first occurrence of every point
        for part in got[2:].reshape(3, Q):
            assert np.array_equal(part, part[same]), name
    record_property('max_err_over_bound', worst)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_two_calls_bit_identical_at_128_electrons(dtype):
    rv, grid = recvec(TRICLINIC), point_lists()['cubic8']
    xd, _ = _walkers(128, 1030, dtype, seed=1)
    assert torch.equal(device.observable_sums(rv, xd, grid, 2), device.observable_sums(rv, xd, grid, 2))


@pytest.mark.parametrize('n_elec', [65, 128])
@pytest.mark.parametrize('batch', [5, 1030])
def test_copies_of_one_walker(n_elec, batch):
    """B copies of one walker: every walker's rho and P have the bits of the B = 1 call, so the batch sums are B times the
    B = 1 sums up to the accumulation term of the bound alone: B u sum_b |rho_b|, B u sum_b |rho_b|^2, B^2 u."""
    rv = recvec(TRICLINIC)
    xd, _ = _walkers(n_elec, 1, 'float64', seed=2)
    for pol_dir, (name, grid) in zip(POLS, point_lists().items()):
        Q = grid.shape[0]
        one = device.observable_sums(rv, xd, grid, pol_dir).cpu().numpy()
        many = device.observable_sums(rv, xd.expand(batch, -1).contiguous(), grid, pol_dir).cpu().numpy()
        sq = one[2 + 2 * Q:]
        acc = np.concatenate([np.full(2, 1.0 if pol_dir >= 0 else 0.0), np.sqrt(sq), np.sqrt(sq), sq]) * batch * batch * U
        assert np.all(np.abs(many - batch * one) <= acc), (name, float((np.abs(many - batch * one) / np.maximum(acc, 1e-300)).max()))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('n_elec', NS)
def test_origin_point_is_exact(n_elec, dtype):
    """q = (0, 0, 0): every factor is 1 + 0i, so Re rho = B N, Im rho = 0, |rho|^2 = B N^2 without a rounding."""
    xd, _ = _walkers(n_elec, 1030, dtype, seed=3)
    got = device.observable_sums(recvec(TRICLINIC), xd, point_lists()['origin'], -1).cpu().numpy()
    assert got.tolist() == [0.0, 0.0, 1030.0 * n_elec, 0.0, 1030.0 * n_elec ** 2]


def _permuted(x, n_elec, perm):
    return np.ascontiguousarray(x.reshape(x.shape[0], n_elec, 3)[:, perm].reshape(x.shape[0], -1))


@pytest.mark.parametrize('n_elec', [96, 128])
def test_permuting_electrons_within_a_chunk(n_elec):
    """Electrons permuted inside each chunk of 64 (the second chunk of N = 96 holds 32): every bit stays.

    This test found that the kernel added a chunk's terms in the order of the electrons' indices, so that renumbering identical
    particles changed the rounding: with 5 walkers 1290 (N = 96) and 1305 (N = 128) of the 1538 sums of the 8^3 grid moved, by
    at most 9.1e-13, 2.3e-3 of `sums_bound`.  k_obs_partial now gives every electron the table row of its slot in the chunk's
    order by coordinate bit patterns (ds_obs.h), and no sum changes."""
    rv = recvec(TRICLINIC)
    x = cell_walkers(n_elec, 5, seed=4)
    rng = np.random.default_rng(n_elec)
    perm = np.concatenate([rng.permutation(64), 64 + rng.permutation(n_elec - 64)])
    changed = []
    for pol_dir, (name, grid) in zip(POLS, point_lists().items()):
        a = device.observable_sums(rv, torch.as_tensor(x, device='cuda'), grid, pol_dir).cpu().numpy()
        b = device.observable_sums(rv, torch.as_tensor(_permuted(x, n_elec, perm), device='cuda'), grid, pol_dir).cpu().numpy()
        bound = sums_bound(x, rv, grid, pol_dir, ld_sums(x, rv, grid, pol_dir)[1])
        ratio = float((np.abs(a - b)[bound > 0] / bound[bound > 0]).max())
        print(f'obs N={n_elec} {name}: {int((a != b).sum())} of {a.size} sums change under a permutation within the chunks, '
              f'largest change {np.abs(a - b).max():.3e}, {ratio:.3e} of the bound')
        assert np.all(np.abs(a - b) <= bound), name
        if not np.array_equal(a, b):
            changed.append(name)
    assert not changed, changed


def test_permuting_electrons_that_share_a_first_coordinate():
    """The slot of an electron is decided by its first coordinate unless two electrons of a chunk share that coordinate's bits;
    then all three decide, and two electrons at the same place are told apart by their lane.  Walkers with such electrons in
    both chunks stay within the bound of the reference, and permuting inside the chunks leaves every bit."""
    rv, n_elec = recvec(TRICLINIC), 96
    x = cell_walkers(n_elec, 5, seed=6).reshape(5, n_elec, 3)
    x[:, [3, 17, 40], 0] = x[:, [9], 0]              # four electrons of chunk 0 with one first coordinate,
    x[:, 17, 1] = x[:, 9, 1]                         # two of them with the second as well,
    x[:, 40] = x[:, 3]                               # two at the same place;
    x[:, 70, 0] = x[:, 80, 0]                        # two in chunk 1
    x[0, 64:, 0] = -0.0                              # and a walker whose whole second chunk shares it
    x = x.reshape(5, -1)
    rng = np.random.default_rng(7)
    perm = np.concatenate([rng.permutation(64), 64 + rng.permutation(n_elec - 64)])
    for pol_dir, (name, grid) in zip(POLS, point_lists().items()):
        a = device.observable_sums(rv, torch.as_tensor(x, device='cuda'), grid, pol_dir)
        b = device.observable_sums(rv, torch.as_tensor(_permuted(x, n_elec, perm), device='cuda'), grid, pol_dir)
        assert torch.equal(a, b), name
        ref, rho = ld_sums(x, rv, grid, pol_dir)
        assert ratio_to_bound(a.cpu().numpy(), ref, sums_bound(x, rv, grid, pol_dir, rho)) <= 1.0, name


@pytest.mark.parametrize('n_elec', [96, 128])
def test_permuting_electrons_across_the_chunk_border(n_elec):
    """Electrons permuted over the whole walker: another summation order, so the sums move by at most the bound."""
    rv = recvec(TRICLINIC)
    x = cell_walkers(n_elec, 5, seed=4)
    perm = np.random.default_rng(n_elec + 1).permutation(n_elec)
    assert (perm[:64] >= 64).any()
    for pol_dir, (name, grid) in zip(POLS, point_lists().items()):
        a = device.observable_sums(rv, torch.as_tensor(x, device='cuda'), grid, pol_dir).cpu().numpy()
        b = device.observable_sums(rv, torch.as_tensor(_permuted(x, n_elec, perm), device='cuda'), grid, pol_dir).cpu().numpy()
        bound = sums_bound(x, rv, grid, pol_dir, ld_sums(x, rv, grid, pol_dir)[1])
        assert np.all(np.abs(a - b) <= bound), name


def test_argument_errors():
    cell, _ = systems.build('lih')
    rv, grid = cell.reciprocal_vectors(), estimator.structure_factor_grid(4)
    x = torch.as_tensor(systems.synthetic_walkers(cell, 8), device='cuda')
    with pytest.raises(RuntimeError, match='outside 0..7'):
        device.observable_sums(rv, x, grid + 5, 0)
    with pytest.raises(RuntimeError, match='pol_direction'):
        device.observable_sums(rv, x, grid, 3)
    with pytest.raises(ValueError, match='empty'):
        device.observable_sums(rv, x[:0], grid, 0)
    with pytest.raises(RuntimeError, match='n_elec'):
        device.observable_sums(rv, torch.zeros(2, 3 * 129, dtype=torch.float64, device='cuda'), grid, 0)
    most = device.observable_sums(rv, torch.zeros(1, 3 * 128, dtype=torch.float64, device='cuda'), grid, 0).cpu().numpy()
    assert most.shape == (2 + 3 * 64,) and most[0] == 1.0 and np.all(most[2:66] == 128.0) and np.all(most[130:] == 128.0 ** 2)
    with pytest.raises(RuntimeError, match='n_q'):
        device.observable_sums(rv, x, estimator.structure_factor_grid(9), 0)
    with pytest.raises(TypeError):
        device.observable_sums(rv, x.half(), grid, 0)
    with pytest.raises(RuntimeError, match='ROCm device'):
        device.observable_sums(rv, x.cpu(), grid, 0)
    with pytest.raises(ValueError, match='electrons'):
        estimator.make_structure_factor(cell)(x[:, :9])


def _drivers(tmp_path):
    from deepsolid_amd import init_guess, network as dnet
    from common import load_case
    from test_gpu_grad import dev_params
    fx, cell, klist, net_kw, params = load_case('lih')
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    ld = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    x0 = torch.as_tensor(init_guess.init_electrons(3, cell, cell.a, cell.nelec, 64, init_width=0.8), device='cuda')
    return cell, slog, ld, dev_params(params), x0


def _check_outputs(path, cell, data, rows, iterations, nq):
    header = (path / 'train_stats.csv').read_text().splitlines()
    assert header[0] == 'step,energy,variance,pmove,imaginary,kinetic,ewald,complex_polarization'
    sk_lines = (path / 'structure_factor.csv').read_text().splitlines()
    assert len(sk_lines) == iterations
    assert all(line.startswith('0,') and len(line.split(',')) == nq ** 3 + 1 for line in sk_lines)
    pol, sk = estimator.make_observables(cell, polarization_direction=0, nq=nq)(data)
    np.testing.assert_array_equal(np.array([float(v) for v in sk_lines[-1].split(',')[1:]]), sk.cpu().numpy())
    np.testing.assert_array_equal(rows[-1]['structure_factor'], sk.cpu().numpy())
    assert complex(rows[-1]['complex_polarization']) == complex(pol)
    assert header[-1].split(',')[-1] == str(np.asarray(pol.cpu().numpy()))
    return header


def test_run_inference_with_observables(tmp_path):
    from deepsolid_amd import inference
    cell, slog, ld, dp, x0 = _drivers(tmp_path)
    data, _, rows = inference.run_inference(slog, ld, dp, x0, cell, iterations=4, key=11, move_width=0.3, mcmc_steps=4,
                                            burn_in=3, adapt_frequency=2, save_path=str(tmp_path), complex_polarization=True,
                                            structure_factor=True, structure_factor_nq=3)
    header = _check_outputs(tmp_path, cell, data, rows, 4, 3)
    assert len(header) == 5 and len(rows) == 4
    # with the switches off the run is what it was: no S(k) file, the reference schema, the same walkers
    off = tmp_path / 'off'
    data2, _, rows2 = inference.run_inference(slog, ld, dp, x0, cell, iterations=4, key=11, move_width=0.3, mcmc_steps=4,
                                              burn_in=3, adapt_frequency=2, save_path=str(off))
    assert not (off / 'structure_factor.csv').exists() and torch.equal(data, data2)
    assert (off / 'train_stats.csv').read_text().splitlines()[0] == ','.join(inference.TRAIN_SCHEMA)
    assert set(rows2[-1]) == set(inference.TRAIN_SCHEMA)
    assert [r['energy'] for r in rows] == [r['energy'] for r in rows2]


def test_run_training_with_observables(tmp_path):
    from deepsolid_amd import inference
    cell, slog, ld, dp, x0 = _drivers(tmp_path)
    data, _, _, _, rows = inference.run_training(slog, ld, dp, x0, cell, iterations=3, key=3, burn_in=5, mcmc_steps=4,
                                                 learning_rate=1e-3, save_path=str(tmp_path), complex_polarization=True,
                                                 structure_factor=True)
    header = _check_outputs(tmp_path, cell, data, rows, 3, 4)
    assert len(header) == 4 and len(rows) == 3
