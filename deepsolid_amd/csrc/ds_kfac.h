// ds_kfac.h -- Kronecker factors of the KFAC optimizer (reference process.py:209-228: kfac_ferminet_alpha with
// estimation_mode = 'fisher_exact' on the normal predictive distribution train.py:133 registers).
//
// Every linear layer of the network is a `repeated_dense` block (network.py:430-446).  With x the layer's input rows
// (one per walker and repeat: electron, pair, or electron of a spin), x~ = [x | 1] and dy = sqrt2 * d log|psi| / d (layer output),
//   A = x~^T x~ / (B R),   G = dy^T dy / (B R)                      (curvature_blocks.py:158-281)
// Both are symmetric rank-k updates over (repeat, walker).  They run on the buffers of the reverse sweep (ds_grad.h), whose
// contiguous axis carries the walkers (or the pairs) -- so both MFMA operands of  C = sum_t sum_j X[t][r][j] X[t][c][j]  run along
// j, as in k_outer_gemm, and only the 32 x 32 blocks on and above the diagonal are computed (k_syrk).  One partial per group of
// PV walkers; k_kfac_assemble / k_kfac_assemble_g add the partials in index order (no atomics: two calls give the same bits),
// drop the padded rows, put the rows into the reference's order and mirror the upper triangle.
//
// The input of a one-electron layer is [h_e | mean_up h | mean_dn h | pair-mean_up_e | pair-mean_dn_e] (network.py:305-332).  The
// spin means are the same for every electron of a walker, so that row is never formed.  A is assembled from
//   P1 = sum_{b,e} u u^T,  u = [h_e | pair means_e | 1]               contraction over (electron, walker) of the G tiles
//   P2 = sum_b v v^T,      v = [sum_e h_e, sum_e pair means_e | means | 1]   contraction over walkers only (k_kfac_aux builds v)
// as  A[loc, loc] = P1,  A[mean, loc] = P2[mean, esum],  A[mean, mean] = R P2[mean, mean],  A[mean, 1] = R P2[mean, 1].
//
// Masks.  The tail of the last group repeats the last walker (ds_value.h) and the pair axis is padded to NP: the cotangents
// are exact zeros there, the activations are not.  k_syrk therefore zeroes the operand at columns beyond the batch and pairs
// beyond N^2, and k_kfac_aux writes zeros for the columns beyond the batch.
#pragma once
#include "ds_grad.h"

namespace ds {

// cot[b] = (sqrt2, 0): the seed 1 / sqrt(variance) of the normal predictive distribution (loss_functions.py:529-537, variance 0.5)
template <typename T>
__global__ void k_kfac_seed(T* __restrict__ cot, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cot[2 * i] = T(1.41421356237309504880);
    cot[2 * i + 1] = T(0);
}

// part[(g * nsplit + split)][r][c] = sum_t sum_j X[t][r][j] X[t][c][j] mask(t, j)   for the 32 x 32 blocks with block(r) <= block(c).
//   rows r < K come from memory; row K (when `ones`) is a virtual row of ones: its products are the masked row sums (bias column).
//   column j of tile t is (jc, jq) = (j / JP, j % JP); it counts when walker t * tw + jc of the group is inside the batch and
//   jq < (qfix >= 0 ? qfix : walkers of the group inside the batch).
//   walker layout [tile = electron][row][PV]:      J = JP = PV, tw = 0, qfix = -1
//   pair layout   [tile = 5-walker block][row][5][NP]:  J = 5 NP, JP = NP, tw = 5, qfix = N^2
// A lane loads FOUR consecutive j of its row and feeds them to four k-steps (see k_outer_gemm).  A wave owns a 32 x 32 block;
// with nsplit > 1 the tiles are dealt to nsplit waves per block.  grid (ceil(blocks * nsplit / 4), groups), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_syrk(const T* __restrict__ X, size_t x_group_stride, size_t x_tile_stride, int ldx, int n_tiles,
                                              int J, int K, int ones, int JP, int qfix, int tw, long Bc, T* __restrict__ part,
                                              size_t part_stride, int nsplit) {
    typedef typename Acc4<T>::type acc_t;
    typedef T vec4 __attribute__((ext_vector_type(4)));
    const int g = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const int Kt = K + (ones ? 1 : 0), nb = (Kt + 31) / 32, nblk = nb * (nb + 1) / 2, wall = blockIdx.x * 4 + wave;
    const int wt = wall % nblk, split = wall / nblk;
    if (split >= nsplit) return;
    int bi = 0, rem = wt;
    while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
    const int bj = bi + rem;
    const long left = Bc - (long)g * PV;
    const int nv = left < PV ? (int)left : PV, qlim = qfix >= 0 ? qfix : nv;
    const int tps = (n_tiles + nsplit - 1) / nsplit, t_lo = split * tps, t_hi = t_lo + tps < n_tiles ? t_lo + tps : n_tiles;
    const T* Xg = X + (size_t)g * x_group_stride;
    int rr[2], cr[2], rk[2], ck[2];            // row in memory; kind: 0 none, 1 memory, 2 ones
    for (int a = 0; a < 2; ++a) {
        rr[a] = 32 * bi + 16 * a + lr; rk[a] = rr[a] < K ? 1 : (rr[a] < Kt ? 2 : 0); if (rk[a] != 1) rr[a] = 0;
        cr[a] = 32 * bj + 16 * a + lr; ck[a] = cr[a] < K ? 1 : (cr[a] < Kt ? 2 : 0); if (ck[a] != 1) cr[a] = 0;
    }
    acc_t acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = acc_t{0, 0, 0, 0};
    const vec4 zero = {0, 0, 0, 0}, one = {1, 1, 1, 1};
    for (int t = t_lo; t < t_hi; ++t) {
        const T* xa[2]; const T* xb[2];
        for (int a = 0; a < 2; ++a) {
            xa[a] = Xg + (size_t)t * x_tile_stride + (size_t)rr[a] * ldx + 4 * lq;
            xb[a] = Xg + (size_t)t * x_tile_stride + (size_t)cr[a] * ldx + 4 * lq;
        }
        for (int j0 = 0; j0 < J; j0 += 16) {
            const int jj = j0 + 4 * lq, jc = jj / JP, jq = jj - jc * JP;
            const bool wok = t * tw + jc < nv;
            vec4 av[2], bv[2];
            for (int a = 0; a < 2; ++a) {
                av[a] = rk[a] == 1 ? *reinterpret_cast<const vec4*>(xa[a] + j0) : (rk[a] == 2 ? one : zero);
                bv[a] = ck[a] == 1 ? *reinterpret_cast<const vec4*>(xb[a] + j0) : (ck[a] == 2 ? one : zero);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool ok = wok && jq + s < qlim;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    av[a][s] = ok ? av[a][s] : T(0);
                    bv[a][s] = ok ? bv[a][s] : T(0);
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = mfma16(av[a][s], bv[b][s], acc[a][b]);
        }
    }
    T* out = part + ((size_t)g * nsplit + split) * part_stride;
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < 4; ++r) {
            const int k = 32 * bi + 16 * a + acc_row<T>(lane, r);
            if (k >= Kt) continue;
            for (int b = 0; b < 2; ++b) {
                const int n = 32 * bj + 16 * b + lr;
                if (n < Kt) out[(size_t)k * Kt + n] = acc[a][b][r];
            }
        }
}

// AUX[group][row][PV], the walker-only operand of P2:
//   rows [0, Kloc):              sum over the electrons e0 .. e0 + ne - 1 of row k of their G tiles
//   rows Kloc + s * Kh + k:      mean over the electrons of spin s of row k (k < Kh), network.py:327-330
// zero for the columns beyond the batch.  grid (ceil((Kloc + nmean Kh) PV / 256), groups), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_kfac_aux(SysDev<T> S, const T* __restrict__ G, int Kloc, int Kh, int nmean, int e0, int ne,
                                                  long Bc, T* __restrict__ AUX) {
    const int g = blockIdx.y, rows = Kloc + nmean * Kh;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * PV) return;
    const int c = idx % PV, row = idx / PV;
    const T* Gw = G + (size_t)g * S.N * S.ldk * PV;
    T v = 0;
    if ((long)g * PV + c < Bc) {
        if (row < Kloc) {
            for (int e = e0; e < e0 + ne; ++e) v += Gw[((size_t)e * S.ldk + row) * PV + c];
        } else {
            const int s = (row - Kloc) / Kh, k = (row - Kloc) % Kh;
            const int i0 = s == 0 ? 0 : S.n_up, ns = s == 0 ? S.n_up : S.n_dn;
            for (int i = i0; i < i0 + ns; ++i) v += Gw[((size_t)i * S.ldk + k) * PV + c];
            v /= T(ns);
        }
    }
    AUX[(size_t)g * rows * PV + idx] = v;
}

// Shape of a block's input rows: the reference's order [h (kh) | nmean spin means (kh each) | npm pair means (k2 each) | 1 (bias)]
// against the padded rows in memory ([h (Kh) | pair means (K2 each)] per electron; AUX behind them: [means (Kh each)]).
struct KfacRows {
    int kh, Kh, nmean, k2, K2, npm, bias, d_in;
};

// reference row -> (kind, padded row): kind 0 = per-electron row (index into u), 1 = spin mean (index into v), 2 = the ones row
__device__ __forceinline__ void kfac_row(const KfacRows& R, int r, int* kind, int* idx) {
    const int Kloc = R.Kh + R.npm * R.K2;
    if (r < R.kh) { *kind = 0; *idx = r; return; }
    r -= R.kh;
    if (r < R.nmean * R.kh) { *kind = 1; *idx = Kloc + (r / R.kh) * R.Kh + r % R.kh; return; }
    r -= R.nmean * R.kh;
    if (r < R.npm * R.k2) { *kind = 0; *idx = R.Kh + (r / R.k2) * R.K2 + r % R.k2; return; }
    *kind = 2; *idx = 0;
}

// A[r][c] = (first ? 0 : A[r][c]) + scale * (sum of the partials, in index order), both triangles from the entry with r <= c.
//   P1: n1 partials of (Kloc + 1)^2,  P2: n2 partials of (Kloc + nmean Kh + 1)^2 (unused when nmean = 0),  rep = R
template <typename T>
__global__ void __launch_bounds__(256) k_kfac_assemble(KfacRows R, const T* __restrict__ P1, long n1, const T* __restrict__ P2, long n2,
                                                       T rep, T scale, int first, T* __restrict__ A) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)R.d_in * R.d_in) return;
    int r = (int)(idx / R.d_in), c = (int)(idx % R.d_in);
    if (r > c) { const int t = r; r = c; c = t; }
    const int Kloc = R.Kh + R.npm * R.K2, K1 = Kloc + 1, K2t = Kloc + R.nmean * R.Kh + 1;
    int kr, ir, kc, ic;
    kfac_row(R, r, &kr, &ir);
    kfac_row(R, c, &kc, &ic);
    const bool use2 = kr == 1 || kc == 1;
    const T mult = (use2 && kr != 0 && kc != 0) ? rep : T(1);      // (mean, mean) and (mean, 1): the same for every repeat
    int i = kr == 2 ? (use2 ? K2t - 1 : Kloc) : ir, j = kc == 2 ? (use2 ? K2t - 1 : Kloc) : ic;
    if (i > j) { const int t = i; i = j; j = t; }
    const T* P = use2 ? P2 : P1;
    const long n = use2 ? n2 : n1;
    const size_t Kt = use2 ? K2t : K1, stride = Kt * Kt;
    T v = 0;
    for (long p = 0; p < n; ++p) v += P[(size_t)p * stride + (size_t)i * Kt + j];
    A[idx] = (first ? T(0) : A[idx]) + scale * mult * v;
}

// G[r][c] likewise from n partials of Kp^2.  omap = 0: output n of the layer is padded row n; omap = 1: the orbital head, the
// reference's column j = part * nparam + p (Re | Im halves) sits in the packed column orb_col(p, part) (ds_gemm.h)
template <typename T>
__global__ void __launch_bounds__(256) k_kfac_assemble_g(int d_out, int Kp, int omap, int nparam, const T* __restrict__ P, long n, T scale,
                                                         int first, T* __restrict__ G) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)d_out * d_out) return;
    int r = (int)(idx / d_out), c = (int)(idx % d_out);
    if (r > c) { const int t = r; r = c; c = t; }
    int i = omap ? orb_col<T>(r % nparam, r / nparam) : r, j = omap ? orb_col<T>(c % nparam, c / nparam) : c;
    if (i > j) { const int t = i; i = j; j = t; }
    const size_t stride = (size_t)Kp * Kp;
    T v = 0;
    for (long p = 0; p < n; ++p) v += P[(size_t)p * stride + (size_t)i * Kp + j];
    G[idx] = (first ? T(0) : G[idx]) + scale * v;
}

// ------------------------------------------------------------------ KFAC step: damped factor inverses and the preconditioner
// (reference utils.py:130-218 pi_adjusted_inverse / psd_inv_cholesky, curvature_blocks.py:233-281).  Matrix m = 2 b is the A
// (d_in x d_in), m = 2 b + 1 the G (d_out x d_out) of block b; all of them share every launch: a grid dimension runs over the
// matrices and a matrix (a tile) beyond its own size exits at once.  The descriptor travels by value (no table on the device).
#define DS_KFAC_MAX_BLOCKS 18          // DS_MAX_LAYERS one-electron + DS_MAX_LAYERS pair layers + two orbital heads
struct KfacMats {
    int nb;                                 // blocks
    int n[2 * DS_KFAC_MAX_BLOCKS];          // order of matrix m
    long off[2 * DS_KFAC_MAX_BLOCKS];       // its first element in factors / inverses / the float64 work copy
    long rs[2 * DS_KFAC_MAX_BLOCKS];        // rows of the matrices before it (the saved column panel is [rs + row][32])
    int rep[DS_KFAC_MAX_BLOCKS];            // R
    long voff[DS_KFAC_MAX_BLOCKS];          // first element of the block's d_in x d_out matrix in v / out
    int toff[DS_KFAC_MAX_BLOCKS + 1];       // first 32 x 32 output tile of the block among the partials of <out, v>
};

// tr[m] = trace(F_m) / w, summed in a fixed order.  grid (2 nb), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_kinv_trace(KfacMats M, const T* __restrict__ F, double w, double* __restrict__ tr) {
    __shared__ double red[256];
    const int m = blockIdx.x, n = M.n[m];
    const T* A = F + M.off[m];
    double v = 0;
    for (int i = threadIdx.x; i < n; i += 256) v += (double)A[(size_t)i * n + i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) tr[m] = red[0] / w;
}

// the pi-adjusted damping of matrix m (utils.py:193-201): false when the block takes the zero branch (s > 0 fails, NaN included)
__device__ __forceinline__ bool kinv_terms(const KfacMats& M, int m, const double* tr, double damping, double* norm, double* damp,
                                           double* s_out, double* lam_out) {
    const int b = m >> 1;
    const double n0 = tr[2 * b], n1 = tr[2 * b + 1], s = n0 * n1, lam = damping / (double)M.rep[b];
    const double d_in = (double)M.n[2 * b], d_out = (double)M.n[2 * b + 1];
    *s_out = s; *lam_out = lam;
    if (!(s > 0.0)) return false;
    *norm = (m & 1) ? n1 : n0;
    *damp = (m & 1) ? sqrt(lam * d_in / (s * d_out)) : sqrt(lam * d_out / (s * d_in));
    return true;
}

// W_m = M0_m = F_m / w / norm + damp I in float64 (the identity on the zero branch, so the elimination below stays harmless).
// grid (ceil(nmax^2 / 256), 2 nb), block 256
template <typename T>
__global__ void __launch_bounds__(256) k_kinv_prep(KfacMats M, const T* __restrict__ F, double w, double damping,
                                                   const double* __restrict__ tr, double* __restrict__ W, double* __restrict__ M0) {
    const int m = blockIdx.y, n = M.n[m];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n * n) return;
    const int r = (int)(idx / n), c = (int)(idx % n);
    double norm, damp, s, lam;
    const bool reg = kinv_terms(M, m, tr, damping, &norm, &damp, &s, &lam);
    const size_t o = (size_t)M.off[m] + (size_t)idx;
    const double v = reg ? (double)F[o] / w / norm + (r == c ? damp : 0.0) : (r == c ? 1.0 : 0.0);
    W[o] = v;
    M0[o] = v;           // kept for the refinement step (k_kinv_refine)
}

// Block step k of the in-place Gauss-Jordan inverse without pivoting (sound for SPD input), pivot rows K = [32 k, 32 k + kb):
//   k_kinv_diag    P = W[K][K]^-1 in LDS, one workgroup per matrix                                  -> P (32 x 32 per matrix)
//   k_kinv_panel   C[i] = W[i][K] (saved: the update below overwrites it),  W[K][j] = P W[K][j]     for the blocks i, j != k
//   k_kinv_update  W[i][j] -= C[i] W[K][j],  W[i][K] = -C[i] P,  W[K][K] = P                       for i != k
// After the last step W is the inverse.  Edge blocks are handled by index: nothing beyond row / column n is read or written.
// (The kernels that are no templates are `static`: two units include this header, ds_gradpass.hip and ds_minsr.hip.)
// grid (2 nb), block 256
static __global__ void __launch_bounds__(256) k_kinv_diag(KfacMats M, const double* __restrict__ W, double* __restrict__ P, int k) {
    __shared__ double S[32][33];
    const int m = blockIdx.x, n = M.n[m], k0 = 32 * k;
    if (k0 >= n) return;
    const int kb = n - k0 < 32 ? n - k0 : 32;
    const double* A = W + M.off[m];
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const int r = e >> 5, c = e & 31;
        S[r][c] = (r < kb && c < kb) ? A[(size_t)(k0 + r) * n + k0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int p = 0; p < kb; ++p) {
        double nv[4];
        const double piv = 1.0 / S[p][p];
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q, r = e >> 5, c = e & 31;
            const double rp = S[r][p], pc = S[p][c], rc = S[r][c];
            nv[q] = r == p ? (c == p ? piv : pc * piv) : (c == p ? -rp * piv : rc - rp * piv * pc);
        }
        __syncthreads();
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q;
            S[e >> 5][e & 31] = nv[q];
        }
        __syncthreads();
    }
    double* Pm = P + (size_t)m * 1024;
    for (int e = threadIdx.x; e < 1024; e += 256) Pm[e] = S[e >> 5][e & 31];
}

// acc (32 x 32) = A (32 x kb) B (kb x 32) on one wave: A[r][k] = Ap[r * lda + k] for r < ra, B[k][c] = Bp[k * ldb + c] for c < cb
__device__ __forceinline__ void kinv_mma(const double* Ap, size_t lda, int ra, const double* Bp, size_t ldb, int cb, int kb,
                                         Acc4<double>::type acc[2][2]) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = Acc4<double>::type{0, 0, 0, 0};
    for (int k0 = 0; k0 < kb; k0 += 4) {
        const int kk = k0 + lq;
        double av[2], bv[2];
        for (int a = 0; a < 2; ++a) {
            av[a] = (16 * a + lr < ra && kk < kb) ? Ap[(size_t)(16 * a + lr) * lda + kk] : 0.0;
            bv[a] = (16 * a + lr < cb && kk < kb) ? Bp[(size_t)kk * ldb + 16 * a + lr] : 0.0;
        }
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) acc[a][b] = mfma16(av[a], bv[b], acc[a][b]);
    }
}

// grid (ceil(nbmax / 4), 2 nb), block 256: a wave per 32-wide block j of the pivot row panel
static __global__ void __launch_bounds__(256) k_kinv_panel(KfacMats M, double* __restrict__ W, const double* __restrict__ P,
                                                    double* __restrict__ Cs, int k) {
    const int m = blockIdx.y, n = M.n[m], k0 = 32 * k, nbm = (n + 31) / 32;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15;
    if (k0 >= n || j >= nbm || j == k) return;
    const int kb = n - k0 < 32 ? n - k0 : 32, j0 = 32 * j, jb = n - j0 < 32 ? n - j0 : 32;
    double* A = W + M.off[m];
    double* C = Cs + (size_t)M.rs[m] * 32;
    for (int e = lane; e < 1024; e += 64) {
        const int r = e >> 5, c = e & 31;
        if (r < jb) C[(size_t)(j0 + r) * 32 + c] = c < kb ? A[(size_t)(j0 + r) * n + k0 + c] : 0.0;
    }
    Acc4<double>::type acc[2][2];
    kinv_mma(P + (size_t)m * 1024, 32, kb, A + (size_t)k0 * n + j0, (size_t)n, jb, kb, acc);
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * a + acc_row<double>(lane, r);
            if (row >= kb) continue;
            for (int b = 0; b < 2; ++b)
                if (16 * b + lr < jb) A[(size_t)(k0 + row) * n + j0 + 16 * b + lr] = acc[a][b][r];
        }
}

// grid (ceil(nbmax^2 / 4), 2 nb), block 256: a wave per 32 x 32 block (i, j)
static __global__ void __launch_bounds__(256) k_kinv_update(KfacMats M, double* __restrict__ W, const double* __restrict__ P,
                                                     const double* __restrict__ Cs, int k) {
    const int m = blockIdx.y, n = M.n[m], k0 = 32 * k, nbm = (n + 31) / 32;
    const int wt = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15;
    if (k0 >= n || wt >= nbm * nbm) return;
    const int i = wt / nbm, j = wt % nbm;
    const int kb = n - k0 < 32 ? n - k0 : 32, i0 = 32 * i, ib = n - i0 < 32 ? n - i0 : 32, j0 = 32 * j, jb = n - j0 < 32 ? n - j0 : 32;
    double* A = W + M.off[m];
    const double* Pm = P + (size_t)m * 1024;
    if (i == k) {
        if (j == k)
            for (int e = lane; e < 1024; e += 64) {
                const int r = e >> 5, c = e & 31;
                if (r < kb && c < kb) A[(size_t)(k0 + r) * n + k0 + c] = Pm[e];
            }
        return;
    }
    const double* C = Cs + ((size_t)M.rs[m] + i0) * 32;
    Acc4<double>::type acc[2][2];
    if (j == k) kinv_mma(C, 32, ib, Pm, 32, kb, kb, acc);
    else kinv_mma(C, 32, ib, A + (size_t)k0 * n + j0, (size_t)n, jb, kb, acc);
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * a + acc_row<double>(lane, r);
            if (row >= ib) continue;
            for (int b = 0; b < 2; ++b) {
                const int col = 16 * b + lr;
                if (col >= jb) continue;
                double* dst = A + (size_t)(i0 + row) * n + j0 + col;
                *dst = j == k ? -acc[a][b][r] : *dst - acc[a][b][r];
            }
        }
}

// One Newton step on the eliminated inverse X of M0:  STAGE 1: Out = I - M0 X,  STAGE 2: Out = X + X R.
// The elimination keeps A_SS^-1 A_SU in place, whose entries grow with the square root of the condition number, and so loses
// more than a factorisation does (about 1e-9 of the largest entry at condition 1e5); one step of X (2 I - M0 X) brings the
// result to the rounding of the two products.  A wave per 32 x 32 tile, K = n.  grid as k_kinv_update
template <int STAGE>
__global__ void __launch_bounds__(256) k_kinv_refine(KfacMats M, const double* __restrict__ A, const double* __restrict__ B,
                                                     double* __restrict__ Out) {
    const int m = blockIdx.y, n = M.n[m], nbm = (n + 31) / 32;
    const int wt = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15;
    if (wt >= nbm * nbm) return;
    const int i0 = 32 * (wt / nbm), j0 = 32 * (wt % nbm);
    const int ib = n - i0 < 32 ? n - i0 : 32, jb = n - j0 < 32 ? n - j0 : 32;
    const size_t o = (size_t)M.off[m];
    Acc4<double>::type acc[2][2];
    kinv_mma(A + o + (size_t)i0 * n, (size_t)n, ib, B + o + j0, (size_t)n, jb, n, acc);
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * a + acc_row<double>(lane, r);
            if (row >= ib) continue;
            for (int b = 0; b < 2; ++b) {
                const int col = 16 * b + lr;
                if (col >= jb) continue;
                const size_t e = o + (size_t)(i0 + row) * n + j0 + col;
                Out[e] = STAGE == 1 ? (i0 + row == j0 + col ? 1.0 : 0.0) - acc[a][b][r] : A[e] + acc[a][b][r];
            }
        }
}

// out_m = W_m / sqrt(s) (I / sqrt(lambda) on the zero branch), both triangles from the upper one.  grid as k_kinv_prep
template <typename T>
__global__ void __launch_bounds__(256) k_kinv_finish(KfacMats M, const double* __restrict__ W, double damping,
                                                     const double* __restrict__ tr, T* __restrict__ out) {
    const int m = blockIdx.y, n = M.n[m];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n * n) return;
    int r = (int)(idx / n), c = (int)(idx % n);
    if (r > c) { const int t = r; r = c; c = t; }
    double norm, damp, s, lam;
    const bool reg = kinv_terms(M, m, tr, damping, &norm, &damp, &s, &lam);
    const double v = reg ? W[(size_t)M.off[m] + (size_t)r * n + c] / sqrt(s) : (r == c ? 1.0 / sqrt(lam) : 0.0);
    out[(size_t)M.off[m] + (size_t)idx] = (T)v;
}

// One product of the preconditioner P_b = A^-_b V_b G^-_b / R_b, a wave per 32 x 32 output tile of block b = blockIdx.y:
//   STAGE 1: Y_b = A^-_b X_b  (the symmetric A^- is read transposed: sixteen lanes read sixteen consecutive elements)
//   STAGE 2: Y_b = X_b G^-_b / R_b, and part[toff[b] + tile] = sum over the tile of Y o V in float64 (fixed order: registers,
//            then a butterfly over the lanes)
// Both products accumulate in float64 on v_mfma_f64_16x16x4_f64 for either element type, and the intermediate A^- V is kept in
// float64 (XT / YT below): a float32 system loses only the final rounding of `out`, and <out, V> is summed from the unrounded
// entries.  In float32 accumulators that scalar -- the q of the norm constraint -- moved by one to two decades with the order of
// summation (EXPERIMENTS.md, "KFAC on large cells").  For T = double nothing differs from a plain float64 product.
// grid (ceil(max tiles / 4), nb), block 256
template <typename T, int STAGE>
struct KprecTypes {
    typedef T XT;           // STAGE 1 reads V
    typedef double YT;      // and writes A^- V in float64
};
template <typename T>
struct KprecTypes<T, 2> {
    typedef double XT;      // STAGE 2 reads A^- V
    typedef T YT;           // and writes out
};

template <typename T, int STAGE>
__global__ void __launch_bounds__(256) k_kprec_gemm(KfacMats M, const T* __restrict__ inv,
                                                    const typename KprecTypes<T, STAGE>::XT* __restrict__ X,
                                                    typename KprecTypes<T, STAGE>::YT* __restrict__ Y, const T* __restrict__ V,
                                                    double* __restrict__ part) {
    typedef Acc4<double>::type acc_t;
    typedef typename KprecTypes<T, STAGE>::XT XT;
    typedef typename KprecTypes<T, STAGE>::YT YT;
    const int b = blockIdx.y, rows = M.n[2 * b], cols = M.n[2 * b + 1], tn = (cols + 31) / 32, tm = (rows + 31) / 32;
    const int wt = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    if (wt >= tm * tn) return;
    const int i0 = 32 * (wt / tn), j0 = 32 * (wt % tn);
    const int K = STAGE == 1 ? rows : cols;
    const T* Ainv = inv + M.off[2 * b + (STAGE == 1 ? 0 : 1)];
    const XT* Xb = X + M.voff[b];
    const size_t sar = STAGE == 1 ? 1 : (size_t)cols, sak = STAGE == 1 ? (size_t)rows : 1;
    acc_t acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 2; ++c) acc[a][c] = acc_t{0, 0, 0, 0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int kk = k0 + lq;
        double av[2], bv[2];
        for (int a = 0; a < 2; ++a) {
            const int row = i0 + 16 * a + lr, col = j0 + 16 * a + lr;
            const bool aok = row < rows && kk < K, bok = col < cols && kk < K;
            const size_t ai = (size_t)row * sar + (size_t)kk * sak, bi = (size_t)kk * cols + col;
            if (STAGE == 1) {
                av[a] = aok ? (double)Ainv[ai] : 0.0;
                bv[a] = bok ? (double)Xb[bi] : 0.0;
            } else {
                av[a] = aok ? (double)Xb[ai] : 0.0;
                bv[a] = bok ? (double)Ainv[bi] : 0.0;
            }
        }
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 2; ++c) acc[a][c] = mfma16(av[a], bv[c], acc[a][c]);
    }
    YT* Yb = Y + M.voff[b];
    const T* Vb = V + M.voff[b];
    const double rep = (double)M.rep[b];
    double dot = 0;
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + 16 * a + acc_row<double>(lane, r);
            if (row >= rows) continue;
            for (int c = 0; c < 2; ++c) {
                const int col = j0 + 16 * c + lr;
                if (col >= cols) continue;
                const size_t o = (size_t)row * cols + col;
                const double y = STAGE == 1 ? acc[a][c][r] : acc[a][c][r] / rep;
                Yb[o] = (YT)y;
                if (STAGE == 2) dot += y * (double)Vb[o];
            }
        }
    if (STAGE == 2) {
        for (int s = 32; s > 0; s >>= 1) dot += __shfl_xor(dot, s, 64);
        if (lane == 0) part[M.toff[b] + wt] = dot;
    }
}

// sq[b] = the block's tile partials added in index order.  grid (nb), block 64
static __global__ void k_kprec_final(KfacMats M, const double* __restrict__ part, double* __restrict__ sq) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    double v = 0;
    for (int t = M.toff[b]; t < M.toff[b + 1]; ++t) v += part[t];
    sq[b] = v;
}

}  // namespace ds
