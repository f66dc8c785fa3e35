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

}  // namespace ds
