"""`ds_minsr_gram`, `ds_minsr_matvec`, `ds_minsr_solve` (csrc/ds_minsr.h) on random matrices, without a system handle.

Gram and mat-vec: every element within  n * 2^-52 * (|J| |J|^T)_ij  (resp. (|J| |v|)_i) of numpy's float64 product of the same
values, n the contraction length: the a-priori bound n u |a|.|b| of ANY summation order (u = 2^-53), doubled because numpy's own
sum carries the same bound.  G exactly symmetric; two calls bit-identical.
Solve: relative to zeta's largest entry, 100 x the disagreement between numpy's LU and Cholesky solutions of the same system
(floor 1e-12): the device elimination is another algorithm again.  A case whose CPU pair disagrees by more than 1e-10 is unfit
and fails as such.
Measured on the MI355X: Gram at most 0.072 of its bound, mat-vec 0.5 (P = 1: one rounding of one product); solve at most 8.1e-11
against the LU solution (R = 166, centred, lambda = 1e-6 of the largest eigenvalue) where the CPU pair disagrees by 5.4e-12, at
most 0.27 of the bound over the 42 systems."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RS = [2, 30, 32, 34, 66, 166, 194]
PS = [1, 37, 4099, 70001]
DTYPES = {'float64': torch.float64, 'float32': torch.float32}


def _jac(R, P, dtype, seed=0):
    """(R, P + 3) device tensor with NaN in the slack, and the float64 numpy values of its first P columns."""
    rng = np.random.default_rng(1000 * R + P + seed)
    J = torch.as_tensor(rng.normal(size=(R, P)), dtype=dtype)
    full = torch.full((R, P + 3), float('nan'), dtype=dtype)
    full[:, :P] = J
    return full.cuda(), J.double().numpy()


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('R', RS)
def test_gram(R, dtype, record_property):
    from deepsolid_amd.device import DeviceSystem
    worst = 0.0
    for P in PS:
        dev, J = _jac(R, P, DTYPES[dtype])
        G = DeviceSystem.minsr_gram(dev, P=P)
        G2 = DeviceSystem.minsr_gram(dev, P=P)
        assert G.dtype == torch.float64 and tuple(G.shape) == (R, R)
        assert torch.equal(G, G2), (R, P)
        assert torch.equal(G, G.T), (R, P)
        g = G.cpu().numpy()
        assert np.isfinite(g).all(), (R, P)
        bound = P * 2.0 ** -52 * (np.abs(J) @ np.abs(J).T)
        err = np.abs(g - J @ J.T)
        worst = max(worst, float((err / bound).max()))
        print(f'gram R={R} P={P} {dtype}: max err / bound = {(err / bound).max():.3e}')
        assert (err <= bound).all(), (R, P, float((err / bound).max()))
    record_property('max_err_over_bound', worst)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('R', RS)
def test_matvec(R, dtype, record_property):
    from deepsolid_amd.device import DeviceSystem
    worst = 0.0
    for P in PS:
        dev, J = _jac(R, P, DTYPES[dtype], seed=7)
        rng = np.random.default_rng(R + P)
        for transpose, n_in, n_sum in ((False, P, P), (True, R, R)):
            v = rng.normal(size=n_in)
            vd = torch.as_tensor(v, device='cuda')
            out = DeviceSystem.minsr_matvec(dev, vd, transpose=transpose, P=P)
            out2 = DeviceSystem.minsr_matvec(dev, vd, transpose=transpose, P=P)
            assert torch.equal(out, out2) and out.dtype == torch.float64
            A = J.T if transpose else J
            o = out.cpu().numpy()
            assert o.shape == (A.shape[0],) and np.isfinite(o).all()
            bound = n_sum * 2.0 ** -52 * (np.abs(A) @ np.abs(v))
            err = np.abs(o - A @ v)
            worst = max(worst, float((err / bound).max()))
            print(f'matvec R={R} P={P} {dtype} transpose={transpose}: max err / bound = {(err / bound).max():.3e}')
            assert (err <= bound).all(), (R, P, transpose, float((err / bound).max()))
    record_property('max_err_over_bound', worst)


def _system(R, block, rel):
    """G = J J^T of a random J (R x (R + 20)), scale = 2 / R, lambda = rel * largest eigenvalue of scale H G H."""
    rng = np.random.default_rng(31 * R + block)
    J = rng.normal(size=(R, R + 20))
    G = J @ J.T
    scale = 2.0 / R
    H = np.eye(R)
    if block:
        H = H - np.kron(np.eye(R // block), np.full((block, block), 1.0 / block))
    M = scale * H @ G @ H
    M = 0.5 * (M + M.T)
    top = np.linalg.eigvalsh(M)[-1]
    if top <= 1e-12 * scale * np.trace(G):        # R = 2, block = 1: H = 0, the matrix is lambda I alone; lambda relative to 1 then
        top = 1.0
    lam = rel * top
    return G, scale, lam, M + lam * np.eye(R), rng.normal(size=R)


@pytest.mark.parametrize('rel', [1e-1, 1e-3, 1e-6])
@pytest.mark.parametrize('centred', [False, True])
@pytest.mark.parametrize('R', RS)
def test_solve(R, centred, rel, record_property):
    from deepsolid_amd.device import DeviceSystem
    block = R // 2 if centred else 0
    G, scale, lam, A, rhs = _system(R, block, rel)
    z_lu = np.linalg.solve(A, rhs)
    L = np.linalg.cholesky(A)
    z_ch = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    top = np.abs(z_lu).max()
    cpu = float(np.abs(z_lu - z_ch).max() / top)
    assert cpu <= 1e-10, f'unfit case: the CPU LU and Cholesky solutions disagree by {cpu:.3e}'
    z = DeviceSystem.minsr_solve(torch.as_tensor(G, device='cuda'), torch.as_tensor(rhs, device='cuda'), scale=scale, damping=lam, block=block)
    z2 = DeviceSystem.minsr_solve(torch.as_tensor(G, device='cuda'), torch.as_tensor(rhs, device='cuda'), scale=scale, damping=lam, block=block)
    assert torch.equal(z, z2)
    dev = float(np.abs(z.cpu().numpy() - z_lu).max() / top)
    record_property('cpu_lu_vs_cholesky', cpu)
    record_property('device_vs_lu', dev)
    print(f'solve R={R} block={block} rel={rel:g}: device vs LU {dev:.3e}, CPU LU vs Cholesky {cpu:.3e}')
    assert dev <= max(100 * cpu, 1e-12), (dev, cpu)


def test_solve_refusals():
    from deepsolid_amd.device import DeviceSystem
    G = torch.eye(6, dtype=torch.float64, device='cuda')
    rhs = torch.ones(6, dtype=torch.float64, device='cuda')
    with pytest.raises(RuntimeError, match='multiple of block'):
        DeviceSystem.minsr_solve(G, rhs, damping=1e-3, block=4)
    for lam in (0.0, -1.0, float('nan')):
        with pytest.raises(RuntimeError, match='lambda must be positive'):
            DeviceSystem.minsr_solve(G, rhs, damping=lam, block=3)
    z = DeviceSystem.minsr_solve(G, rhs, scale=1.0, damping=1.0, block=0)
    assert float((z - 0.5).abs().max()) < 1e-15
