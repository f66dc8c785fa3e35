// ds_jac.h -- per-walker emission of the reverse sweep (ds_grad.h): the Jacobian d log psi_b / d theta behind ds_logpsi_jacobian.
//
// The sweep forms every parameter block's gradient from operand tiles whose contiguous axis carries the PV walkers of a group
// (or, in the pair stream, the NP pairs of one of the five walkers of a tile) and sums over that axis.  The kernels here take the
// same operands and sum over the electron / pair tiles of ONE walker only; the result goes to that walker's row of `jac`
// (row-major, leading dimension ld, packed columns of ds_param_layout).  A workgroup owns one walker: it stages the walker's
// operand columns through LDS -- in the sweep's buffers the walker's values of consecutive rows lie PV elements apart -- and its
// stores run along the parameter axis of the row.  All sums run in index order: two calls give the same bits, and a walker's row
// does not depend on which group or chunk the walker sits in.
//
// Masks.  Rows exist for the walkers of the batch only: the grid runs over them, so the tail of the last group (which repeats the
// last walker and whose activations are not zero) is never read.  In the pair layout the contraction stops at the N^2 pairs of
// the walker: the columns up to NP are padding.
#pragma once
#include "ds_grad.h"

namespace ds {

// cot[b] = (1, 0) (half 0: the log|psi| rows) or (0, 1) (half 1: the phase rows) on every walker
template <typename T>
__global__ void k_jac_seed(T* __restrict__ cot, long n, int half) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cot[2 * i] = half == 0 ? T(1) : T(0);
    cot[2 * i + 1] = half == 0 ? T(0) : T(1);
}

// rows[r][0 .. n) = 0 for r < nrows (the padding columns of the packed layout stay exact zeros).  grid (ceil(n / 256), nrows)
template <typename T>
__global__ void k_jac_zero(T* __restrict__ rows, size_t ld, long n, long nrows) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || (long)blockIdx.y >= nrows) return;
    rows[(size_t)blockIdx.y * ld + p] = T(0);
}

// rows[w][off + k * Nc + n] = sum over the contraction entries of walker w of X[.][k][.] * Z[.][n][.],  k < K, n < Nc.
//   walker layout (NP = 0): [tile][row][PV], entries = the n_tiles tiles at column w % PV            (k_outer_gemm's operands)
//   pair layout   (NP > 0): [5-walker tile][row][5][NP], entries = the Q = N^2 pairs of walker w      (k_two_bwd's operands)
//   X null: a virtual row of ones (K = 1): the bias gradients, per-walker row sums of Z
// A workgroup computes a 32 x 64 block of (k, n) of one walker; the entries are staged 32 at a time.  Thread (tk, tn) owns
// column tn and the rows tk, tk + 4, ...: a wave stores 64 consecutive parameters.  grid (k-blocks * n-blocks, walkers), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_jac_outer(const T* __restrict__ X, size_t x_group_stride, size_t x_tile_stride, int ldx,
                                                   const T* __restrict__ Z, size_t z_group_stride, size_t z_tile_stride, int ldz,
                                                   int n_tiles, int K, int Nc, int NP, int Q, long Bc, T* __restrict__ rows, size_t ld,
                                                   size_t off) {
    constexpr int KR = 32, NR = 64, CC = 32;
    __shared__ T xs[CC][KR + 1];
    __shared__ T zs[CC][NR + 1];
    const long w = blockIdx.y;
    if (w >= Bc) return;
    const int g = (int)(w / PV), c = (int)(w % PV);
    const int nbn = (Nc + NR - 1) / NR, k0 = ((int)blockIdx.x / nbn) * KR, n0 = ((int)blockIdx.x % nbn) * NR;
    const int tn = threadIdx.x & 63, tk = threadIdx.x >> 6;
    const int tile0 = NP > 0 ? c / 5 : 0, col0 = NP > 0 ? (c % 5) * NP : c;
    const int Qn = NP > 0 ? Q : 1, total = (NP > 0 ? 1 : n_tiles) * Qn;
    const T* Xb = X ? X + (size_t)g * x_group_stride + (size_t)tile0 * x_tile_stride + col0 : nullptr;
    const T* Zb = Z + (size_t)g * z_group_stride + (size_t)tile0 * z_tile_stride + col0;
    T acc[KR / 4];
    for (int i = 0; i < KR / 4; ++i) acc[i] = T(0);
    for (int c0 = 0; c0 < total; c0 += CC) {
        __syncthreads();
        for (int e = threadIdx.x; e < (KR + NR) * CC; e += 256) {
            const int r = e / CC, cc = e % CC, ci = c0 + cc, t = ci / Qn, q = ci - t * Qn;
            const bool ok = ci < total;
            if (r < KR) {
                const int k = k0 + r;
                T v = T(0);
                if (ok && k < K) v = Xb ? Xb[(size_t)t * x_tile_stride + (size_t)k * ldx + q] : T(1);
                xs[cc][r] = v;
            } else {
                const int n = n0 + r - KR;
                zs[cc][r - KR] = (ok && n < Nc) ? Zb[(size_t)t * z_tile_stride + (size_t)n * ldz + q] : T(0);
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int cc = 0; cc < CC; ++cc) {
            const T z = zs[cc][tn];
#pragma unroll
            for (int i = 0; i < KR / 4; ++i) acc[i] += xs[cc][tk + 4 * i] * z;
        }
    }
    const int n = n0 + tn;
    if (n >= Nc) return;
    T* out = rows + (size_t)w * ld + off;
    for (int i = 0; i < KR / 4; ++i) {
        const int k = k0 + tk + 4 * i;
        if (k < K) out[(size_t)k * Nc + n] = acc[i];
    }
}

// orbital bias (k_orb_bias_grad per walker): rows[w][off + part * nparam + p] = sum over the spin's electrons of the packed column
// (p, part) of PHIBAR.  grid (walkers), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_jac_orb_bias(const T* __restrict__ PHIBAR, size_t group_stride, int ns, int OC, int nparam,
                                                      long Bc, T* __restrict__ rows, size_t ld, size_t off) {
    const long w = blockIdx.x;
    if (w >= Bc) return;
    const int g = (int)(w / PV), c = (int)(w % PV);
    for (int q = threadIdx.x; q < 2 * nparam; q += blockDim.x) {
        const int p = q % nparam, pt = q / nparam;
        const T* Pg = PHIBAR + (size_t)g * group_stride + (size_t)orb_col<T>(p, pt) * PV + c;
        T v = 0;
        for (int e = 0; e < ns; ++e) v += Pg[(size_t)e * OC * PV];
        rows[(size_t)w * ld + off + q] = v;
    }
}

// envelope parameters (k_env_grad per walker; all envelope types): a thread owns one sigma entry (a, p, j) of the spin channel and
// sums over the channel's electrons of ONE walker.  grid (walkers, spin channels), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_jac_env(SysDev<T> S, const T* __restrict__ x, long Bc, const T* __restrict__ G0,
                                                 const T* __restrict__ QBAR, const T* __restrict__ env_pi0, const T* __restrict__ env_sg0,
                                                 const T* __restrict__ env_pi1, const T* __restrict__ env_sg1, T* __restrict__ rows,
                                                 size_t ld, long off_pi0, long off_sg0, long off_pi1, long off_sg1) {
    const long w = blockIdx.x;
    if (w >= Bc) return;
    const int g = (int)(w / PV), c = (int)(w % PV), sp = blockIdx.y, N = S.N, A = S.A;
    const int i0 = sp == 0 ? 0 : S.n_up, ns = sp == 0 ? S.n_up : S.n_dn, np = S.nparam[sp];
    const int nsig = S.env_type == 0 ? 1 : (S.env_type == 1 ? 3 : 9);
    const T* pi_ = sp == 0 ? env_pi0 : env_pi1;
    const T* sg_ = sp == 0 ? env_sg0 : env_sg1;
    T* dpi = rows + (size_t)w * ld + (sp == 0 ? off_pi0 : off_pi1);
    T* dsg = rows + (size_t)w * ld + (sp == 0 ? off_sg0 : off_sg1);
    for (int idx = threadIdx.x; idx < A * np * nsig; idx += blockDim.x) {
        const int j = idx / (A * np), ap = idx % (A * np), a = ap / np, p = ap % np;
        const int jk = j / 3, jm = j % 3;            // full: sigma[k = jk][m = jm];  diagonal: m = j
        const T pv = pi_[ap];
        T s00 = 0, s01 = 0, s02 = 0, s10 = 0, s11 = 0, s12 = 0, s20 = 0, s21 = 0, s22 = 0;
        if (S.env_type == 0) s00 = sg_[ap];
        else if (S.env_type == 1) { s00 = sg_[(a * 3 + 0) * np + p]; s11 = sg_[(a * 3 + 1) * np + p]; s22 = sg_[(a * 3 + 2) * np + p]; }
        else {
            s00 = sg_[(0 * A + a) * np + p]; s01 = sg_[(1 * A + a) * np + p]; s02 = sg_[(2 * A + a) * np + p];
            s10 = sg_[(3 * A + a) * np + p]; s11 = sg_[(4 * A + a) * np + p]; s12 = sg_[(5 * A + a) * np + p];
            s20 = sg_[(6 * A + a) * np + p]; s21 = sg_[(7 * A + a) * np + p]; s22 = sg_[(8 * A + a) * np + p];
        }
        const T* kv = S.klist[sp] + 3 * (p % S.norb[sp]);
        T gp = 0, gs = 0;
        for (int ii = 0; ii < ns; ++ii) {
            const int i = i0 + ii;
            const T* fp = G0 + ((size_t)(g * N + i) * S.ldk + S.nf * a) * PV;     // rows sd, rel_x, rel_y, rel_z of atom a
            const T* qb = QBAR + ((size_t)(g * N + i) * S.nparam_max + p) * 2 * PV;
            const T* xp = x + (size_t)w * 3 * N + 3 * i;
            T sn, cs;
            ds_sincos(kv[0] * xp[0] + kv[1] * xp[1] + kv[2] * xp[2], &sn, &cs);
            const T ge = qb[c] * cs - qb[PV + c] * sn;
            if (S.env_type == 0) {
                const T sd = fp[c], u = sd * s00, ex = ds_exp(-ds_abs(u));
                gp += ge * ex;
                gs -= ge * pv * ex * sd * ds_sign(u);
            } else {
                const T r0 = fp[(size_t)PV + c], r1 = fp[(size_t)2 * PV + c], r2 = fp[(size_t)3 * PV + c];
                const T u0 = s00 * r0 + s10 * r1 + s20 * r2, u1 = s01 * r0 + s11 * r1 + s21 * r2, u2 = s02 * r0 + s12 * r1 + s22 * r2;
                const T r = ds_sqrt(u0 * u0 + u1 * u1 + u2 * u2), ex = ds_exp(-r);
                gp += ge * ex;
                if (r > T(0)) {
                    const T um = jm == 0 ? u0 : (jm == 1 ? u1 : u2);
                    const int kk = S.env_type == 1 ? jm : jk;
                    const T rk = kk == 0 ? r0 : (kk == 1 ? r1 : r2);
                    gs -= ge * pv * ex * um * rk / r;
                }
            }
        }
        if (j == 0) dpi[ap] = gp;
        if (S.env_type == 0) dsg[ap] = gs;
        else if (S.env_type == 1) dsg[(a * 3 + jm) * np + p] = gs;
        else dsg[(j * A + a) * np + p] = gs;
    }
}

}  // namespace ds
