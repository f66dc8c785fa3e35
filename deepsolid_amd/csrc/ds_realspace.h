// ds_realspace.h -- real-space walker observables as integer counts: the spin-resolved electron density on a grid of a folding
// lattice and the spin-resolved radial pair histogram behind g(r).
//
// The reference has no such estimator; the conventions are this project's own.  One launch takes the
// walkers x (B, 3N), float64 or float32 widened to float64 on load, does all arithmetic in float64 and ADDS to two caller-owned
// int64 buffers; it never zeroes them.
//
// Density counts dens[2][g0 g1 g2]: spin of electron e is 0 if e < n_up, else 1.  The electron is folded into the folding
// lattice A_f: f = r . inv(A_f), f -= floor(f), i_j = min(int(f_j g_j), g_j - 1), flat bin (i0 g1 + i1) g2 + i2.
//
// Pair counts pair[3][n_r], channels up-up, up-down, down-down: for each pair i < j the minimum-image distance in the simulation
// cell A: f = (r_i - r_j) . inv(A), f -= floor(f + 1/2), r = the shortest of |(f + s) . A| over s in {-1,0,1}^3;
// bin k = int(r n_r / r_max), counted only if r < r_max.  The caller guarantees r_max <= r_ws (half the shortest non-zero lattice
// vector: at most one image lies inside r_max) and r_max < 1.5 x the smallest plane spacing (an image with some |s_j| >= 2 has
// |f_j + s_j| >= 1.5 and is farther than r_max, so the 27 shifts are enough).
//
// Layout: workgroups of 256 lanes, workgroup g takes the walkers b = g, g + G, ...  A walker's 3N coordinates are staged once in
// LDS (3 KB at N = 128).  Lanes e < N scatter the density with one 64-bit integer atomicAdd on global memory each (B N atomics per
// call).  Lanes stride over the N(N-1)/2 pairs and count into a private 3 x n_r uint32 histogram in LDS (12 KB at n_r = 1024) with
// LDS integer atomics; at the end the workgroup adds its non-zero bins to the global int64 buffer, one atomic each.
//
// Integer addition is associative and commutative: whatever order the atomics arrive in, the buffers end with the same bits, so
// two calls on the same input are bit-identical without slabs or a fixed reduction tree.  No float atomics, no scratch (no
// dynamically indexed private arrays: the 27 shifts are three unrolled loops over kernel-argument constants).
//
// Overflow of the uint32 LDS bins: one workgroup visits at most ceil(B_launch / G) walkers and a walker adds at most
// N(N-1)/2 <= 8128 counts, all bins together.  ds_realspace_counts launches at most RS_MAX_LAUNCH_WALKERS = 2^28 walkers at a
// time (it loops over such pieces of a larger B), and G = 1024 for them, so a bin holds at most 2^18 x 8128 < 2^31.
#pragma once
#include <hip/hip_runtime.h>

namespace ds {

constexpr int RS_MAX_N = 128;                         // electrons per walker
constexpr int RS_MAX_G = 256;                         // grid points per axis
constexpr long long RS_MAX_BINS = 1ll << 22;          // g0 g1 g2
constexpr int RS_MAX_NR = 1024;                       // radial bins
constexpr int RS_MAX_GROUPS = 1024;                   // workgroups of one launch
constexpr long long RS_MAX_LAUNCH_WALKERS = 1ll << 28;
constexpr int RS_THREADS = 256;
static_assert((RS_MAX_LAUNCH_WALKERS / RS_MAX_GROUPS) * (RS_MAX_N * (RS_MAX_N - 1) / 2) < (1ll << 31), "LDS bins would overflow");

struct RealSpaceArgs {
    double fold_inv[9];                // inv(A_f), row-major: f_c = sum_k r_k fold_inv[3 k + c]
    double a[9];                       // simulation cell, rows = lattice vectors
    double a_inv[9];                   // inv(A)
    double r_max;
    int g[3];
    int n_r;
    int n_up;
    int do_dens, do_pair;
};

__host__ __device__ inline int rs_groups(long long B) { return (int)(B < RS_MAX_GROUPS ? B : RS_MAX_GROUPS); }

// pair index p in 0 .. N(N-1)/2 -> (lo, hi), lo < hi, p = hi (hi - 1) / 2 + lo
__device__ inline void rs_pair_of(int p, int& lo, int& hi) {
    int h = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    if (h * (h - 1) / 2 > p) --h;      // the float square root is off by at most one step either way (p < 2^13)
    if ((h + 1) * h / 2 <= p) ++h;
    hi = h;
    lo = p - h * (h - 1) / 2;
}

// The flat density bin of an electron at (r0, r1, r2): the folding rule above.  Shared by every kernel that counts densities
// (k_realspace_counts here, k_realspace_counts_w in ds_fw.h), so that their binning cannot drift apart.
__device__ __forceinline__ long long rs_density_bin(const RealSpaceArgs& A, double r0, double r1, double r2) {
    long long bin = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double f = r0 * A.fold_inv[c] + r1 * A.fold_inv[3 + c] + r2 * A.fold_inv[6 + c];
        f -= floor(f);
        // min(int(f g), g - 1), taken in double so that the conversion is defined for every input (a NaN lands in bin 0)
        const double t = fmin(fmax(f * (double)A.g[c], 0.0), (double)(A.g[c] - 1));
        bin = bin * A.g[c] + (int)t;
    }
    return bin;
}

// The radial bin of the pair (lo, hi), lo < hi, of the staged walker `pos`, or -1 if its minimum-image distance is not below
// r_max; ch receives the channel.  Shared like rs_density_bin.
__device__ __forceinline__ int rs_pair_bin(const RealSpaceArgs& A, const double* pos, int lo, int hi, int& ch) {
    const int n_r = A.n_r;
    const double d0 = pos[3 * lo] - pos[3 * hi], d1 = pos[3 * lo + 1] - pos[3 * hi + 1], d2 = pos[3 * lo + 2] - pos[3 * hi + 2];
    double f0 = d0 * A.a_inv[0] + d1 * A.a_inv[3] + d2 * A.a_inv[6];
    double f1 = d0 * A.a_inv[1] + d1 * A.a_inv[4] + d2 * A.a_inv[7];
    double f2 = d0 * A.a_inv[2] + d1 * A.a_inv[5] + d2 * A.a_inv[8];
    f0 -= floor(f0 + 0.5);
    f1 -= floor(f1 + 0.5);
    f2 -= floor(f2 + 0.5);
    double best = INFINITY;
#pragma unroll
    for (int s0 = -1; s0 <= 1; ++s0) {
#pragma unroll
        for (int s1 = -1; s1 <= 1; ++s1) {
#pragma unroll
            for (int s2 = -1; s2 <= 1; ++s2) {
                const double u0 = f0 + s0, u1 = f1 + s1, u2 = f2 + s2;
                const double v0 = u0 * A.a[0] + u1 * A.a[3] + u2 * A.a[6];
                const double v1 = u0 * A.a[1] + u1 * A.a[4] + u2 * A.a[7];
                const double v2 = u0 * A.a[2] + u1 * A.a[5] + u2 * A.a[8];
                best = fmin(best, v0 * v0 + v1 * v1 + v2 * v2);
            }
        }
    }
    const double r = sqrt(best);
    ch = hi < A.n_up ? 0 : (lo < A.n_up ? 1 : 2);
    if (!(r < A.r_max)) return -1;     // (also for a NaN)
    const int k = (int)(r * (double)n_r / A.r_max);
    return k < n_r ? k : n_r - 1;      // r < r_max, so only a rounding of the quotient could reach n_r
}

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void k_realspace_counts(RealSpaceArgs A, const T* __restrict__ x, long long B, int N,
                                                                 unsigned long long* __restrict__ dens,
                                                                 unsigned long long* __restrict__ pair) {
    __shared__ double pos[3 * RS_MAX_N];
    __shared__ unsigned int hist[3 * RS_MAX_NR];
    const int tid = threadIdx.x;
    const int G = gridDim.x;
    const int n_r = A.n_r;
    const int n_pairs = N * (N - 1) / 2;
    if (A.do_pair)
        for (int k = tid; k < 3 * n_r; k += RS_THREADS) hist[k] = 0u;

    for (long long b = blockIdx.x; b < B; b += G) {
        const T* xb = x + b * 3 * (long long)N;
        __syncthreads();               // the previous walker's readers are done (and, the first time, hist is zero)
        for (int k = tid; k < 3 * N; k += RS_THREADS) pos[k] = (double)xb[k];
        __syncthreads();

        if (A.do_dens && tid < N) {
            const double r0 = pos[3 * tid], r1 = pos[3 * tid + 1], r2 = pos[3 * tid + 2];
            const long long bin = rs_density_bin(A, r0, r1, r2);
            const long long cells = (long long)A.g[0] * A.g[1] * A.g[2];
            atomicAdd(dens + (tid < A.n_up ? 0 : cells) + bin, 1ull);
        }

        if (A.do_pair) {
            for (int p = tid; p < n_pairs; p += RS_THREADS) {
                int lo, hi;
                rs_pair_of(p, lo, hi);
                int ch;
                const int k = rs_pair_bin(A, pos, lo, hi, ch);
                if (k >= 0) {
                    atomicAdd(&hist[ch * n_r + k], 1u);
                }
            }
        }
    }

    if (A.do_pair) {
        __syncthreads();
        for (int k = tid; k < 3 * n_r; k += RS_THREADS) {
            const unsigned int v = hist[k];
            if (v) atomicAdd(pair + k, (unsigned long long)v);
        }
    }
}

}  // namespace ds
