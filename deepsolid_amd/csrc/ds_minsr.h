// ds_minsr.h -- linear algebra on a per-walker Jacobian J (R x P, row-major, leading dimension ld; R = 2 B rows, P parameters):
// the sample-space form of stochastic reconfiguration (MinSR) and SPRING need  G = J J^T,  J v,  J^T v  and the solution of
// (scale H G H + lambda I) zeta = rhs.  No system handle: any shape.  Operands are float64 or float32 (converted on load);
// every sum is float64 and runs in a fixed order without atomics: two calls give the same bits.
//
// Gram (k_minsr_gram).  The contraction axis is the long one (P ~ 5e5) and contiguous in both operands: a row panel of J is
// both the A and the B operand of v_mfma_f64_16x16x4_f64.  A workgroup of four waves owns a 128 x 128 tile of G on or above the
// diagonal, each wave a 64 x 64 quarter (4 x 4 MFMA tiles, 64 accumulator registers of float64).  Per step of KC = 16 columns the
// workgroup stages the two 128 x 16 panels through LDS (row stride 18 doubles: one 16-byte access of padding) -- the loads of
// the next step are issued into registers before the MFMAs of this one -- and every wave reads 4 + 4 sixteen-row operand slices,
// four consecutive columns per lane, for 64 MFMAs: any assignment of the columns to (k-step, lane group) is a valid contraction
// order as long as both operands use the same one (as in k_outer_gemm).  Per byte fetched from L2 / HBM the 128-wide tile does
// 16 flop in float64 operands; a wave-per-32 x 32 kernel that reads global memory (k_syrk) does 4.
// Small R: the P axis is dealt to `nsplit` workgroups per tile, each writing its partial of the upper triangle; k_minsr_gram_sum
// adds the partials in index order and writes both triangles.  nsplit = 1 writes G directly, the mirrored entry from the same
// accumulator: symmetric to the bit either way.  Rows beyond R and columns beyond P are zeros by index (the slack of ld is
// never read).
#pragma once
#include "ds_kfac.h"

namespace ds {

constexpr int MINSR_TM = 128;      // tile of G per workgroup
constexpr int MINSR_KC = 16;       // columns of J per staging step
constexpr int MINSR_LDS = MINSR_KC + 2;

// grid (upper tiles, nsplit), block 256.  direct: out = G (R x R); else out = partials, split s at out + s * R * R (upper entries only)
template <typename T>
__global__ void __launch_bounds__(256) k_minsr_gram(const T* __restrict__ J, int R, long P, size_t ld, long pchunk, double* __restrict__ out,
                                                    int direct) {
    typedef Acc4<double>::type acc_t;
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int TM = MINSR_TM, KC = MINSR_KC, LD = MINSR_LDS, NL = TM * KC / 256;
    __shared__ __attribute__((aligned(16))) double As[TM * LD];
    __shared__ __attribute__((aligned(16))) double Bs[TM * LD];
    const int nb = (R + TM - 1) / TM;
    int bi = 0, rem = blockIdx.x;
    while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
    const int bj = bi + rem;
    const int split = blockIdx.y;
    const long p_lo = (long)split * pchunk, p_hi = p_lo + pchunk < P ? p_lo + pchunk : P;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4, wr = wave >> 1, wc = wave & 1;
    acc_t acc[4][4];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) acc[a][b] = acc_t{0, 0, 0, 0};
    // staging: element e = tid + 256 i of a panel is (row e / KC, column e % KC): sixteen lanes read one row's 16 columns
    double ra[NL], rb[NL];
    const int sk = threadIdx.x % KC, sr = threadIdx.x / KC;          // rows sr, sr + 16, ...
    auto fetch = [&](long p0) {
        const long p = p0 + sk;
        const bool pok = p < p_hi;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int row = sr + (256 / KC) * i, ga = TM * bi + row, gb = TM * bj + row;
            ra[i] = (pok && ga < R) ? (double)J[(size_t)ga * ld + p] : 0.0;
            rb[i] = (pok && gb < R) ? (double)J[(size_t)gb * ld + p] : 0.0;
        }
    };
    if (p_lo < p_hi) fetch(p_lo);
    for (long p0 = p_lo; p0 < p_hi; p0 += KC) {
        __syncthreads();                       // the MFMAs of the step before have read their operands
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int row = sr + (256 / KC) * i;
            As[row * LD + sk] = ra[i];
            Bs[row * LD + sk] = rb[i];
        }
        __syncthreads();
        if (p0 + KC < p_hi) fetch(p0 + KC);
        d2 av[4][2], bv[4][2];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const d2* pa = reinterpret_cast<const d2*>(&As[(64 * wr + 16 * a + lr) * LD + 4 * lq]);
            const d2* pb = reinterpret_cast<const d2*>(&Bs[(64 * wc + 16 * a + lr) * LD + 4 * lq]);
            av[a][0] = pa[0]; av[a][1] = pa[1];
            bv[a][0] = pb[0]; bv[a][1] = pb[1];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = mfma16(av[a][s >> 1][s & 1], bv[b][s >> 1][s & 1], acc[a][b]);
    }
    double* dst = direct ? out : out + (size_t)split * R * R;
    for (int a = 0; a < 4; ++a)
        for (int r = 0; r < 4; ++r) {
            const int gi = TM * bi + 64 * wr + 16 * a + acc_row<double>(lane, r);
            for (int b = 0; b < 4; ++b) {
                const int gj = TM * bj + 64 * wc + 16 * b + lr;
                if (gi > gj || gj >= R) continue;
                const double v = acc[a][b][r];
                dst[(size_t)gi * R + gj] = v;
                if (direct && gi != gj) dst[(size_t)gj * R + gi] = v;
            }
        }
}

// G[r][c] = sum_s part[s][min(r, c)][max(r, c)], s in index order.  grid (ceil(R^2 / 256)), block 256
__global__ void __launch_bounds__(256) k_minsr_gram_sum(const double* __restrict__ part, int nsplit, int R, double* __restrict__ G) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)R * R;
    if (idx >= n) return;
    int r = (int)(idx / R), c = (int)(idx % R);
    if (r > c) { const int t = r; r = c; c = t; }
    double v = 0;
    for (int s = 0; s < nsplit; ++s) v += part[(size_t)s * n + (size_t)r * R + c];
    G[idx] = v;
}

// out[r] = (add ? add[r] : 0) + alpha * sum_p J[r][p] v[p]: a workgroup per row, a thread sums its columns p = tid, tid + 256, ...
// in order, then an LDS tree.  One pass over J, consecutive lanes read consecutive columns.  grid (R), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_minsr_jv(const T* __restrict__ J, long P, size_t ld, const double* __restrict__ v,
                                                  const double* __restrict__ add, double alpha, double* __restrict__ out) {
    __shared__ double red[256];
    const T* row = J + (size_t)blockIdx.x * ld;
    double s = 0;
    for (long p = threadIdx.x; p < P; p += 256) s += (double)row[p] * v[p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (add ? add[blockIdx.x] : 0.0) + alpha * red[0];
}

// out[p] = sum_r J[r][p] v[r], rows in index order: a thread per column, consecutive lanes read consecutive columns of a row.
// One pass over J.  grid (ceil(P / 256)), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_minsr_jtv(const T* __restrict__ J, int R, long P, size_t ld, const double* __restrict__ v,
                                                   double* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const T* col = J + p;
    double s = 0;
#pragma unroll 8
    for (int r = 0; r < R; ++r) s += (double)col[(size_t)r * ld] * v[r];
    out[p] = s;
}

// ---- the solve: A = scale H G H + lambda I, H centring each consecutive `block` rows and columns (block = 0: H = I).
//   (H G H)_ij = G_ij - m_i[b(j)] - m_j[b(i)] + mm[b(i)][b(j)],  m_i[c] = mean of G[i][block c],  mm[a][c] = mean of m_i[c] over block a
// formed for i <= j only and mirrored, from the upper entries of G: exactly symmetric.

// M1[i][c] = mean over the columns of block c of G[min][max].  grid (R, nblk), block 256
__global__ void __launch_bounds__(256) k_minsr_rowmeans(const double* __restrict__ G, int R, int block, double* __restrict__ M1) {
    __shared__ double red[256];
    const int i = blockIdx.x, c = blockIdx.y, nblk = R / block;
    double s = 0;
    for (int t = threadIdx.x; t < block; t += 256) {
        const int j = c * block + t;
        s += i <= j ? G[(size_t)i * R + j] : G[(size_t)j * R + i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) M1[(size_t)i * nblk + c] = red[0] / (double)block;
}

// MM[a][c] = mean over the rows i of block a of M1[i][c].  grid (nblk, nblk), block 256
__global__ void __launch_bounds__(256) k_minsr_blockmeans(const double* __restrict__ M1, int R, int block, double* __restrict__ MM) {
    __shared__ double red[256];
    const int a = blockIdx.x, c = blockIdx.y, nblk = R / block;
    double s = 0;
    for (int t = threadIdx.x; t < block; t += 256) s += M1[(size_t)(a * block + t) * nblk + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) MM[(size_t)a * nblk + c] = red[0] / (double)block;
}

// the "prepare this matrix" front of the Gauss-Jordan kernels (ds_kfac.h): W = M0 = A (M0 may be null).  grid (ceil(R^2 / 256)), block 256
__global__ void __launch_bounds__(256) k_minsr_prep(const double* __restrict__ G, int R, int block, double scale, double lambda,
                                                    const double* __restrict__ M1, const double* __restrict__ MM, double* __restrict__ W,
                                                    double* __restrict__ M0) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)R * R) return;
    int i = (int)(idx / R), j = (int)(idx % R);
    if (i > j) { const int t = i; i = j; j = t; }
    double v = G[(size_t)i * R + j];
    if (block > 0) {
        const int nblk = R / block, bi = i / block, bj = j / block;
        v = v - M1[(size_t)i * nblk + bj] - M1[(size_t)j * nblk + bi] + MM[(size_t)bi * nblk + bj];
    }
    v = scale * v + (i == j ? lambda : 0.0);
    W[idx] = v;
    if (M0) M0[idx] = v;
}

}  // namespace ds
