"""GPU checks of the walker observables (`ds_observables`, csrc/ds_obs.h, through deepsolid_amd.estimator) against the
reference-executed fixture tests/golden/estimators.npz and a float64 numpy restatement, and of the driver switches
(process.py:277-283, 337-342, 361-362).

float32 tolerance: the kernel widens float32 walkers to float64 and does all its arithmetic in float64, so against a float64
evaluation AT THE SAME (float32-rounded) walkers the only float32 step is the final rounding of each result: |dS| <= 2^-24 |S|
for S(k), and 2^-24 |P| per component for the complex64 polarization (plus the float64 noise, 1e-12 here)."""
import numpy as np
import pytest
import torch

from deepsolid_amd import device, estimator, systems

from test_estimator_cpu import CELLS, fixture, np_sums, recvec

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
