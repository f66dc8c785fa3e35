"""`ds_minsr_gram`, `ds_minsr_matvec`, `ds_minsr_solve` (csrc/ds_minsr.h) on random matrices, without a system handle.

Gram and mat-vec: every element within  n * 2^-52 * (|J| |J|^T)_ij  (resp. (|J| |v|)_i) of numpy's float64 product of the same
values, n the contraction length: the a-priori bound n u |a|.|b| of ANY summation order (u = 2^-53), doubled because numpy's own
sum carries the same bound.  G exactly symmetric; two calls bit-identical.
Solve: relative to zeta's largest entry, 100 x the disagreement between numpy's LU and Cholesky solutions of the same system
(floor 1e-12): the device elimination is another algorithm again.  A case whose CPU pair disagrees by more than 1e-10 is unfit
and fails as such.

Shapes.  RS x PS: one or two rows of 128 x 128 tiles, at most three tiles.  SPRING calls with R = 2 B and block = B, B = 4096 in
the benchmark, so three further lists follow the code that only such shapes reach:
  RS_TILES x PS_TILES   3, 3, 4 and 6 tile rows (R = 258: the last tile holds 2 rows): every (bi, bj) the `while (rem >= nb - bi)`
                        decode of k_minsr_gram produces, with P = 37 written directly (`nsplit` = 1) and P = 4099 through four
                        partials with a ragged last one.  Row r is scaled by 2^((r mod 13) - 6), exact in either format, so
                        that neighbouring rows' norms differ by orders of magnitude and a tile written to another tile's
                        place misses the element-wise bound by as much.
  R_DIRECT, P_DIRECT    23 tile rows, 276 tiles > 256: `gram_plan` gives nsplit = 1 as it does in training, and P = 2053 is 129
                        steps of the prefetch pipeline with a tail of 5 columns: the direct write after a long contraction.
  SOLVE_BLOCKS          block = 300 and 513 take the `t += 256` loops of k_minsr_rowmeans and k_minsr_blockmeans a second
                        and a third time; block = 2 and 3 give 193 and 200 blocks (gridDim.y, M1 of R x nblk).

Measured on the MI355X: Gram at most 0.091 of its bound (R = 300, P = 37, float32; 0.072 over RS x PS), mat-vec 0.5 (P = 1 and
R = 2: one rounding of one product; 0.028 over the new lists); solve at most 8.5e-11 against the LU solution (R = 600, block = 3,
lambda = 1e-6 of the largest eigenvalue) where the CPU pair disagrees by 3.9e-11, at most 0.38 of the bound over the 60 systems
(R = 600, block = 300, lambda = 1e-6: 7.2e-11 against 1.9e-12; 0.27 over the 42 of RS).  At lambda = 0.1 every new system comes
out within 3.6e-15, under the 1e-12 floor by more than two orders: the one refinement step of `solve_run` suffices at R = 1026."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RS = [2, 30, 32, 34, 66, 166, 194]
PS = [1, 37, 4099, 70001]
RS_TILES = [258, 300, 386, 642]
PS_TILES = [37, 4099]
R_DIRECT, P_DIRECT = 2818, 2053
SOLVE_BLOCKS = [(258, 0), (258, 129), (386, 2), (600, 300), (600, 3), (1026, 513)]
DTYPES = {'float64': torch.float64, 'float32': torch.float32}


def _jac(R, P, dtype, seed=0, scaled=False):
    """(R, P + 3) device tensor with NaN in the slack, and the float64 numpy values of its first P columns.
    `scaled`: row r times 2^((r mod 13) - 6)."""
    rng = np.random.default_rng(1000 * R + P + seed)
    J = torch.as_tensor(rng.normal(size=(R, P)), dtype=dtype)
    if scaled:
        J = J * torch.as_tensor(2.0 ** (np.arange(R) % 13 - 6), dtype=dtype)[:, None]
    full = torch.full((R, P + 3), float('nan'), dtype=dtype)
    full[:, :P] = J
    return full.cuda(), J.double().numpy()


def _check_gram(R, P, dtype, dev, J):
    """-> the largest error / bound of G = J J^T on `dev` against the float64 values `J`"""
    from deepsolid_amd.device import DeviceSystem
    G = DeviceSystem.minsr_gram(dev, P=P)
    G2 = DeviceSystem.minsr_gram(dev, P=P)
    assert G.dtype == torch.float64 and tuple(G.shape) == (R, R)
    assert torch.equal(G, G2), (R, P)
    assert torch.equal(G, G.T), (R, P)
    g = G.cpu().numpy()
    assert np.isfinite(g).all(), (R, P)
    bound = P * 2.0 ** -52 * (np.abs(J) @ np.abs(J).T)
    err = np.abs(g - J @ J.T)
    print(f'gram R={R} P={P} {dtype}: max err / bound = {(err / bound).max():.3e}')
    assert (err <= bound).all(), (R, P, float((err / bound).max()))
    return float((err / bound).max())


def _check_matvec(R, P, dtype, dev, J):
    """-> the largest error / bound of J v and J^T v"""
    from deepsolid_amd.device import DeviceSystem
    worst = 0.0
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
    return worst


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('R', RS)
def test_gram(R, dtype, record_property):
    worst = 0.0
    for P in PS:
        dev, J = _jac(R, P, DTYPES[dtype])
        worst = max(worst, _check_gram(R, P, dtype, dev, J))
    record_property('max_err_over_bound', worst)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('R', RS)
def test_matvec(R, dtype, record_property):
    worst = 0.0
    for P in PS:
        dev, J = _jac(R, P, DTYPES[dtype], seed=7)
        worst = max(worst, _check_matvec(R, P, dtype, dev, J))
    record_property('max_err_over_bound', worst)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('R', RS_TILES)
def test_gram_and_matvec_three_tile_rows_and_more(R, dtype, record_property):
    """Rows scaled by powers of two; P = 37 is written directly, P = 4099 goes through four partials."""
    from deepsolid_amd import _lib
    lib = _lib.load()
    assert lib.ds_minsr_gram_workspace_bytes(R, 37) == 0 and lib.ds_minsr_gram_workspace_bytes(R, 4099) == 4 * R * R * 8
    gram = matvec = 0.0
    for P in PS_TILES:
        dev, J = _jac(R, P, DTYPES[dtype], scaled=True)
        gram = max(gram, _check_gram(R, P, dtype, dev, J))
        matvec = max(matvec, _check_matvec(R, P, dtype, dev, J))
    record_property('gram_max_err_over_bound', gram)
    record_property('matvec_max_err_over_bound', matvec)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
def test_gram_and_matvec_direct_write_after_a_long_contraction(dtype, record_property):
    """The branch every training step takes: more than 256 tiles, so no split of P, and a contraction of many pipeline steps."""
    from deepsolid_amd import _lib
    assert _lib.load().ds_minsr_gram_workspace_bytes(R_DIRECT, P_DIRECT) == 0         # no partials: the plan is direct
    dev, J = _jac(R_DIRECT, P_DIRECT, DTYPES[dtype], scaled=True)
    record_property('gram_max_err_over_bound', _check_gram(R_DIRECT, P_DIRECT, dtype, dev, J))
    record_property('matvec_max_err_over_bound', _check_matvec(R_DIRECT, P_DIRECT, dtype, dev, J))


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


def _check_solve(R, block, rel, record_property):
    from deepsolid_amd.device import DeviceSystem
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


@pytest.mark.parametrize('rel', [1e-1, 1e-3, 1e-6])
@pytest.mark.parametrize('centred', [False, True])
@pytest.mark.parametrize('R', RS)
def test_solve(R, centred, rel, record_property):
    _check_solve(R, R // 2 if centred else 0, rel, record_property)


@pytest.mark.parametrize('rel', [1e-1, 1e-3, 1e-6])
@pytest.mark.parametrize('R,block', SOLVE_BLOCKS)
def test_solve_large_blocks_and_many_blocks(R, block, rel, record_property):
    _check_solve(R, block, rel, record_property)


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
