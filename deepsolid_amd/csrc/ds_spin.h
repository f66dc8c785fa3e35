// ds_spin.h -- spin-exchange ratios psi(P_p R) / psi(R) and the per-walker sums the total-spin estimator <S^2> is made of.
//
// The reference has no such estimator: the conventions are this project's own (include/deepsolid_hip.h).
// Electrons 0 .. n_up - 1 are spin up, the rest spin down; P = n_up n_dn pairs, pair p = i n_dn + (j - n_up) with i < n_up <= j.
// P_p R is R with the positions of electrons i and j exchanged; nothing is wrapped or shifted (both positions belong to R).
// Sample g = w * M + m of a call takes pair (first_pair + m) % P of walker w.  There is no random number in the call.
//
//   k_spin_propose   one thread per (sample, electron) of a chunk: the exchanged rows for the value chain
//   (value chain on the chunk: log|psi(P R)|, phase(P R))
//   k_spin_ratio     one thread per sample of the chunk: q = exp(log|psi(P R)| - log|psi(R)|) phase(P R) conj(phase(R)) in float64
//                    into the call's (B, M, 2) float64 buffer (and, on request, into out_ratio in the system's dtype)
//   k_spin_walker    after the last chunk, one wave per walker: lane l adds q of m = l, l + 64, ... in order, lane 0 adds the 64
//                    lane results in lane order -> t_w; a walker with a non-finite q is bad: t_w = NaN
//   k_spin_final     one workgroup: thread t adds (Re t_w, Im t_w, (Re t_w)^2, 1) of the good walkers w = t, t + 256, ... in order,
//                    thread 0 adds the 256 results in thread order and makes ONE addition per entry to the caller's sums
//
// The order of every addition is a function of (B, M) alone, and the chunks only decide which launch computes a q: the sums are
// bit-identical for any workspace size and from run to run.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace ds {

struct SpinArgs {
    long long g0, n;                   // first sample of the chunk, samples in the chunk
    int M, N, n_up, n_dn, first;
};

// the two electrons sample g exchanges
__device__ __forceinline__ void spin_pair_of(const SpinArgs& A, long long g, int* i, int* j) {
    const int p = (int)(((long long)A.first + g % A.M) % ((long long)A.n_up * A.n_dn));
    *i = p / A.n_dn;
    *j = A.n_up + p % A.n_dn;
}

// xd (n, 3N): row r is walker (g0 + r) / M with the positions of the electrons of its pair exchanged
template <typename T>
__global__ void __launch_bounds__(256) k_spin_propose(SpinArgs A, const T* __restrict__ x, T* __restrict__ xd) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n * A.N) return;
    const long long r = t / A.N, g = A.g0 + r, w = g / A.M;
    const int el = (int)(t % A.N);
    int i, j;
    spin_pair_of(A, g, &i, &j);
    const int src = el == i ? j : (el == j ? i : el);
    const T* in = x + (w * A.N + src) * 3;
    T* o = xd + t * 3;
    for (int c = 0; c < 3; ++c) o[c] = in[c];
}

template <typename T>
__global__ void __launch_bounds__(256) k_spin_ratio(SpinArgs A, const T* __restrict__ la0, const T* __restrict__ ph0,
                                                    const T* __restrict__ la, const T* __restrict__ ph, double* __restrict__ q,
                                                    T* __restrict__ out_ratio) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const long long g = A.g0 + r, w = g / A.M;
    const double mag = exp((double)la[r] - (double)la0[w]);
    const double pr = (double)ph[2 * r], pi = (double)ph[2 * r + 1], rr = (double)ph0[2 * w], ri = (double)ph0[2 * w + 1];
    const double qr = mag * (pr * rr + pi * ri), qi = mag * (pi * rr - pr * ri);       // phase(P R) conj(phase(R))
    q[2 * g] = qr; q[2 * g + 1] = qi;
    if (out_ratio) { out_ratio[2 * g] = (T)qr; out_ratio[2 * g + 1] = (T)qi; }
}

// tw (B, 2): t_w = sum_m q_{w,m}, or (NaN, NaN) for a walker with a non-finite q; out_walker gets a copy
constexpr int SPIN_WAVES = 4;          // walkers per workgroup of k_spin_walker
__global__ void __launch_bounds__(64 * SPIN_WAVES) k_spin_walker(const double* __restrict__ q, long long B, int M,
                                                                 double* __restrict__ tw, double* __restrict__ out_walker) {
    __shared__ double l_s[SPIN_WAVES][64][2];
    __shared__ int bad_s[SPIN_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * SPIN_WAVES + wave;
    double ar = 0.0, ai = 0.0;
    int bad = 0;
    if (w < B) {
        const double* qw = q + 2 * w * M;
        for (int m = lane; m < M; m += 64) {
            const double qr = qw[2 * m], qi = qw[2 * m + 1];
            bad |= !(isfinite(qr) && isfinite(qi));
            ar += qr; ai += qi;
        }
    }
    l_s[wave][lane][0] = ar; l_s[wave][lane][1] = ai; bad_s[wave][lane] = bad;
    __syncthreads();
    if (lane == 0 && w < B) {
        double tr = l_s[wave][0][0], ti = l_s[wave][0][1];
        int b = bad_s[wave][0];
        for (int l = 1; l < 64; ++l) { tr += l_s[wave][l][0]; ti += l_s[wave][l][1]; b |= bad_s[wave][l]; }
        if (b) tr = ti = __builtin_nan("");
        tw[2 * w] = tr; tw[2 * w + 1] = ti;
        if (out_walker) { out_walker[2 * w] = tr; out_walker[2 * w + 1] = ti; }
    }
}

// sums[0..3] += [sum Re t_w, sum Im t_w, sum (Re t_w)^2, good walkers], n_bad[0] += bad walkers: ONE addition per call and entry, so
// a second call on the same input doubles a buffer exactly.  A bad walker is one whose t_w is NaN.
__global__ void __launch_bounds__(256) k_spin_final(const double* __restrict__ tw, long long B, double* __restrict__ sums,
                                                    long long* __restrict__ n_bad) {
    __shared__ double p_s[256][4];
    const int t = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long w = t; w < B; w += 256) {
        const double tr = tw[2 * w], ti = tw[2 * w + 1];
        if (isnan(tr) || isnan(ti)) continue;
        a[0] += tr; a[1] += ti; a[2] += tr * tr; a[3] += 1.0;
    }
    for (int c = 0; c < 4; ++c) p_s[t][c] = a[c];
    __syncthreads();
    if (t < 4) {
        double s = p_s[0][t];
        for (int u = 1; u < 256; ++u) s += p_s[u][t];
        if (sums) sums[t] += s;
        if (t == 3 && n_bad) n_bad[0] += B - (long long)s;
    }
}

}  // namespace ds
