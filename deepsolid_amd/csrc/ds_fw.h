// ds_fw.h -- forward walking for the DMC of ds_dmc.h: ancestor tables carried through the combs, the
// real-space counts of ds_realspace.h with an integer weight per walker and a source row per walker, and weighted sums of
// per-walker values in the fixed order of k_dmc_stats.
//
// The pure estimator of an observable O at lag L is  sum_w w_w(t + L) O(x_anc(w)(t)) / sum_w w_w(t + L): the snapshot taken L
// blocks ago, weighted with what its descendants weigh now.  anc(w) is the walker of the snapshot from which walker w descends;
// -1 means the lineage is lost.
//
// Every index that a kernel here reads from a caller's array (parents, anc as `index`) is range-checked BEFORE it is used as an
// address; one that is out of range is skipped and counted, it never faults.  No floating-point atomics: counts are integer
// atomics (any order of arrival gives the same bits), sums go through the fixed tree of k_dmc_stats.
//
//   k_fw_compose           P[w] = parents[0][parents[1][.. parents[steps-1][w]]], -1 once the chain leaves [0, B)
//   k_fw_apply             anc[s][w] = P[w] < 0 ? -1 : old[s][P[w]]   (old: a copy of anc, so the gather is out of place)
//   k_realspace_counts_w   k_realspace_counts with source row index[w] and integer weight q_w = rint(weight[w] weight_scale)
//   k_fw_sums              one row of partials per FW_GROUP walkers: per column k (sum w v[src, k], sum w)
//   k_fw_sums_final        the rows added in workgroup order
//
// Overflow of the LDS pair bins of k_realspace_counts_w: they are 64-bit.  One workgroup visits at most RS_MAX_LAUNCH_WALKERS /
// RS_MAX_GROUPS = 2^18 walkers of a launch, a walker adds at most N(N-1)/2 <= 8128 < 2^13 counts of at most FW_MAX_Q = 2^24 each:
// below 2^55.  The global int64 buffers are the caller's: a bin grows by at most B N q (density) or B N(N-1)/2 q (pairs) per
// call, so with q <= 2^24 they hold 2^63 / (2^24 x 2^13) = 2^26 calls' worth of walkers of 128 electrons that all fall in one bin.
#pragma once
#include <hip/hip_runtime.h>

#include "ds_realspace.h"

namespace ds {

constexpr long long FW_MAX_Q = 1ll << 24;             // largest integer weight of one walker
static_assert((RS_MAX_LAUNCH_WALKERS / RS_MAX_GROUPS) * (RS_MAX_N * (RS_MAX_N - 1) / 2) < ((1ll << 62) / FW_MAX_Q),
              "64-bit LDS bins would overflow");
constexpr int FW_MAX_K = 64;                          // value columns of ds_dmc_fw_sums
constexpr int FW_GROUP = 256;                         // walkers per row of partials: DMC_GROUP of ds_dmc.h, whose summation order this is

// ------------------------------------------------------------------------------------------------------------ ancestor tables
__global__ void __launch_bounds__(256) k_fw_compose(long long B, int steps, const int* __restrict__ parents, int* __restrict__ P) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B) return;
    long long p = w;
    for (int k = steps - 1; k >= 0; --k) {
        p = parents[(long long)k * B + p];             // p is inside [0, B) here
        if (p < 0 || p >= B) { p = -1; break; }
    }
    P[w] = (int)p;
}

// old (n_slots, B): the tables before the block; anc (n_slots, B): the tables after it.  A value of `old` is copied, never used
// as an address: -1 stays -1.
__global__ void __launch_bounds__(256) k_fw_apply(long long B, int n_slots, const int* __restrict__ P, const int* __restrict__ old,
                                                  int* __restrict__ anc) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B) return;
    const long long p = P[w];                          // written by k_fw_compose: -1 or inside [0, B)
    for (int s = 0; s < n_slots; ++s) anc[(long long)s * B + w] = p < 0 ? -1 : old[(long long)s * B + p];
}

// ------------------------------------------------------------------------------------------------------- the weight of a walker
// src: the source row of walker w, -1 if index[w] is outside [0, B_src)
__device__ __forceinline__ long long fw_source(const int* __restrict__ index, long long w, long long B_src) {
    const long long s = index ? (long long)index[w] : w;
    return (s < 0 || s >= B_src) ? -1 : s;
}

// q = rint(weight scale) as an integer, -1 for a weight that is not finite, negative, or beyond FW_MAX_Q after scaling
__device__ __forceinline__ long long fw_quantise(const double* __restrict__ weight, long long w, double scale) {
    if (!weight) return 1;
    const double wt = weight[w];
    if (!isfinite(wt) || wt < 0.0) return -1;
    const double q = rint(wt * scale);                 // ties to even, as numpy's rint
    if (!(q <= (double)FW_MAX_Q)) return -1;           // (also an infinite or NaN product)
    return (long long)q;
}

// ------------------------------------------------------------------------------------------------------------ weighted counts
// Layout and binning of k_realspace_counts (rs_density_bin / rs_pair_bin are its code).  Walker b of the launch (b0 + b of the
// call) reads row src of x; q_tot[0] += sum q, n_bad[0] += walkers with a bad index, n_bad[1] += walkers with a bad weight (a walker
// with both counts under the index alone).
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void k_realspace_counts_w(RealSpaceArgs A, const T* __restrict__ x, long long B, int N,
                                                                   long long B_src, const int* __restrict__ index,
                                                                   const double* __restrict__ weight, double scale,
                                                                   unsigned long long* __restrict__ dens,
                                                                   unsigned long long* __restrict__ pair,
                                                                   unsigned long long* __restrict__ q_tot,
                                                                   unsigned long long* __restrict__ n_bad) {
    __shared__ double pos[3 * RS_MAX_N];
    __shared__ unsigned long long hist[3 * RS_MAX_NR];
    const int tid = threadIdx.x;
    const int G = gridDim.x;
    const int n_r = A.n_r;
    const int n_pairs = N * (N - 1) / 2;
    unsigned long long q_sum = 0, bad_index = 0, bad_weight = 0;      // (every lane keeps them; lane 0 adds them at the end)
    if (A.do_pair)
        for (int k = tid; k < 3 * n_r; k += RS_THREADS) hist[k] = 0ull;

    for (long long b = blockIdx.x; b < B; b += G) {
        const long long src = fw_source(index, b, B_src);             // uniform over the workgroup
        if (src < 0) { ++bad_index; continue; }
        const long long qs = fw_quantise(weight, b, scale);
        if (qs < 0) { ++bad_weight; continue; }
        if (qs == 0) continue;
        const unsigned long long q = (unsigned long long)qs;
        q_sum += q;
        const T* xb = x + src * 3 * (long long)N;
        __syncthreads();               // the previous walker's readers are done (and, the first time, hist is zero)
        for (int k = tid; k < 3 * N; k += RS_THREADS) pos[k] = (double)xb[k];
        __syncthreads();

        if (A.do_dens && tid < N) {
            const long long bin = rs_density_bin(A, pos[3 * tid], pos[3 * tid + 1], pos[3 * tid + 2]);
            const long long cells = (long long)A.g[0] * A.g[1] * A.g[2];
            atomicAdd(dens + (tid < A.n_up ? 0 : cells) + bin, q);
        }

        if (A.do_pair) {
            for (int p = tid; p < n_pairs; p += RS_THREADS) {
                int lo, hi, ch;
                rs_pair_of(p, lo, hi);
                const int k = rs_pair_bin(A, pos, lo, hi, ch);
                if (k >= 0) atomicAdd(&hist[ch * n_r + k], q);
            }
        }
    }

    if (A.do_pair) {
        __syncthreads();
        for (int k = tid; k < 3 * n_r; k += RS_THREADS) {
            const unsigned long long v = hist[k];
            if (v) atomicAdd(pair + k, v);
        }
    }
    if (tid == 0) {
        if (q_sum) atomicAdd(q_tot, q_sum);
        if (bad_index) atomicAdd(n_bad, bad_index);
        if (bad_weight) atomicAdd(n_bad + 1, bad_weight);
    }
}

// ------------------------------------------------------------------------------------------------------------- weighted sums
// part (n_groups, K, 2): per column k the pair (sum w v[src, k], sum w) over the walkers of the group with a valid src, a finite
// weight > 0 and a finite v[src, k].  Thread t takes walker g0 + t; the tree adds t and t + s: the order of k_dmc_stats.
// bad[0] += walkers with a bad index, bad[1] += walkers with a bad weight + (walker, column) entries whose value is not finite.
__global__ void __launch_bounds__(FW_GROUP) k_fw_sums(long long B, int K, const double* __restrict__ values, long long B_src,
                                                       const int* __restrict__ index, const double* __restrict__ weight,
                                                       double* __restrict__ part, unsigned long long* __restrict__ bad) {
    __shared__ double sh[2][FW_GROUP];
    const long long w = (long long)blockIdx.x * FW_GROUP + threadIdx.x;
    long long src = -1;
    double wt = 0.0;
    unsigned long long n_bad_index = 0, n_bad_value = 0;
    if (w < B) {
        src = fw_source(index, w, B_src);
        if (src < 0) {
            ++n_bad_index;
        } else {
            wt = weight ? weight[w] : 1.0;
            if (!isfinite(wt) || wt < 0.0) { ++n_bad_value; src = -1; }
            else if (wt == 0.0) src = -1;              // contributes nothing, and is not bad
        }
    }
    for (int k = 0; k < K; ++k) {
        double a = 0.0, b = 0.0;
        if (src >= 0) {
            const double v = values[src * (long long)K + k];
            if (isfinite(v)) { a = wt * v; b = wt; }
            else ++n_bad_value;
        }
        __syncthreads();                               // the previous column's readers are done
        sh[0][threadIdx.x] = a;
        sh[1][threadIdx.x] = b;
        __syncthreads();
        for (int s = FW_GROUP / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) {
                sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
                sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
            }
            __syncthreads();
        }
        if (threadIdx.x < 2) part[((long long)blockIdx.x * K + k) * 2 + threadIdx.x] = sh[threadIdx.x][0];
    }
    if (n_bad_index) atomicAdd(bad, n_bad_index);
    if (n_bad_value) atomicAdd(bad + 1, n_bad_value);
}

// out (K, 2): the rows added in workgroup order onto 0
__global__ void __launch_bounds__(2 * FW_MAX_K) k_fw_sums_final(const double* __restrict__ part, long long n_groups, int K,
                                                                double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= 2 * K) return;
    double s = 0.0;
    for (long long g = 0; g < n_groups; ++g) s += part[g * 2 * K + j];
    out[j] = s;
}

}  // namespace ds
