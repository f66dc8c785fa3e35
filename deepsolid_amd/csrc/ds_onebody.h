// ds_onebody.h -- one-body ratios psi(R') / psi(R) and the momentum distribution n(k) folded from them.
//
// The reference has no such estimator: the conventions are this project's own (include/deepsolid_hip.h).
// Sample g = w * M + m of a call moves electron e = (first_electron + m) % N of walker w by a shift s that is uniform in the
// simulation cell; every other coordinate is copied and R' is NOT wrapped (the network's Bloch phase reads the unwrapped
// coordinates).  The shift is a pure function of (seed, offset, g): Philox stream 3 (ds_mcmc.h uses 0..2), block A at index 2g,
// block B at index 2g + 1, s = f . a in float64 with f = (u53_co(A0,A1), u53_co(A2,A3), u53_co(B0,B1)).  Test mode replays
// caller-supplied shifts instead.  Both kernels derive s by the same function, so nothing but the displaced rows travels
// through memory between them.
//
//   k_onebody_propose     one thread per (sample, electron) of a chunk: the displaced rows for the value chain
//   (value chain on the chunk: log|psi(R')|, phase(R'))
//   k_onebody_accumulate  one workgroup per OB_GROUP consecutive samples: q = exp(log|psi(R')| - log|psi(R)|) phase(R')
//                         conj(phase(R)) per sample into LDS, then lane l of each of the four waves sums q exp(-i k.s) over its
//                         wave's quarter of the samples IN SAMPLE ORDER for the points k = l, l + 64, ..., and the quarters are
//                         added in order -> one row of partials per group (both spins, then the two bad counts)
//   k_onebody_final       adds the rows in group order to the call's running sums, the last chunk's adds those to the caller's buffer
//
// A chunk starts at a multiple of OB_GROUP samples, so the groups -- and with them every addition and its order -- are the same
// however the workspace cuts the call into chunks: the sums are bit-identical for any workspace size and from run to run.
// No floating-point atomics.
#pragma once
#include "ds_mcmc.h"

namespace ds {

constexpr int OB_MAX_K = 512;          // k points per call
constexpr int OB_GROUP = PV;           // samples per partial row = walkers per value-chain group: chunks start on group borders
constexpr int OB_ROW = 4 * OB_MAX_K + 2;   // doubles of one partial row: [spin][k][re, im], then the bad count of either spin

struct OneBodyArgs {
    double a[9];                       // simulation cell, rows = lattice vectors
    PhiloxKey key;
    long long g0, n;                   // first sample of the chunk, samples in the chunk
    int M, N, n_up, first;
};

// shift of sample g: replayed from `shifts` (B, M, 3) or drawn from the Philox stream 3.  The products and sums of f . a are
// rounded one by one (no contraction into fused multiply-adds), so a host replay is bit-exact.
template <typename T>
__device__ __forceinline__ void onebody_shift(const OneBodyArgs& A, const T* __restrict__ shifts, long long g, double s[3]) {
    if (shifts) {
        for (int c = 0; c < 3; ++c) s[c] = (double)shifts[3 * g + c];
        return;
    }
    const unsigned k0 = (unsigned)A.key.seed, k1 = (unsigned)(A.key.seed >> 32);
    const unsigned c2 = (unsigned)A.key.offset, c3 = ((unsigned)(A.key.offset >> 32) & 0x3fffffffu) | 0xC0000000u;
    const unsigned long long ia = 2ull * (unsigned long long)g, ib = ia + 1;
    const Philox4 pa = philox4x32_10((unsigned)ia, (unsigned)(ia >> 32), c2, c3, k0, k1);
    const Philox4 pb = philox4x32_10((unsigned)ib, (unsigned)(ib >> 32), c2, c3, k0, k1);
    const double f0 = u53_co(pa.v[0], pa.v[1]), f1 = u53_co(pa.v[2], pa.v[3]), f2 = u53_co(pb.v[0], pb.v[1]);
    {
#pragma clang fp contract(off)
        for (int c = 0; c < 3; ++c) s[c] = (f0 * A.a[c] + f1 * A.a[3 + c]) + f2 * A.a[6 + c];
    }
}

// xd (n, 3N): row j is walker (g0 + j) / M with electron (first + (g0 + j) % M) % N moved by the sample's shift
template <typename T>
__global__ void __launch_bounds__(256) k_onebody_propose(OneBodyArgs A, const T* __restrict__ x, const T* __restrict__ shifts,
                                                         T* __restrict__ xd, T* __restrict__ out_shift) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n * A.N) return;
    const long long j = i / A.N, g = A.g0 + j, w = g / A.M;
    const int el = (int)(i % A.N), e = (int)((A.first + g % A.M) % A.N);
    const T* r = x + (w * A.N + el) * 3;
    T* o = xd + i * 3;
    if (el != e) {
        for (int c = 0; c < 3; ++c) o[c] = r[c];
        return;
    }
    double s[3];
    onebody_shift(A, shifts, g, s);
    for (int c = 0; c < 3; ++c) o[c] = (T)((double)r[c] + s[c]);
    if (out_shift)
        for (int c = 0; c < 3; ++c) out_shift[3 * g + c] = (T)s[c];
}

// one workgroup of OB_WAVES waves per group of OB_GROUP samples; part row = blockIdx.x (see the head of the file).  Wave v sums
// the samples [v, v + 1) * OB_GROUP / OB_WAVES of the group in sample order, wave 0 adds the OB_WAVES results in wave order.
constexpr int OB_WAVES = 4;
static_assert(OB_GROUP % OB_WAVES == 0, "every wave takes the same number of samples");
template <typename T>
__global__ void __launch_bounds__(64 * OB_WAVES) k_onebody_accumulate(OneBodyArgs A, const T* __restrict__ shifts,
                                                                      const T* __restrict__ la0, const T* __restrict__ ph0,
                                                                      const T* __restrict__ la, const T* __restrict__ ph,
                                                                      const double* __restrict__ kvec, int n_k,
                                                                      T* __restrict__ out_ratio, double* __restrict__ part) {
    __shared__ double q_s[OB_GROUP][2], s_s[OB_GROUP][3];
    __shared__ int spin_s[OB_GROUP];                    // 0 / 1, or -1 - spin: q is not finite, the sample is left out and counted
    __shared__ double w_s[OB_WAVES][64][4];             // per wave and lane: (spin 0 re, im, spin 1 re, im) of the lane's k point
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long j0 = (long long)blockIdx.x * OB_GROUP;
    const int ns = (int)(A.n - j0 < OB_GROUP ? A.n - j0 : OB_GROUP);
    for (int t = threadIdx.x; t < ns; t += 64 * OB_WAVES) {
        const long long j = j0 + t, g = A.g0 + j, w = g / A.M;
        const int sp = (int)((A.first + g % A.M) % A.N) < A.n_up ? 0 : 1;
        const double mag = exp((double)la[j] - (double)la0[w]);
        const double pr = (double)ph[2 * j], pi = (double)ph[2 * j + 1], rr = (double)ph0[2 * w], ri = (double)ph0[2 * w + 1];
        const double qr = mag * (pr * rr + pi * ri), qi = mag * (pi * rr - pr * ri);       // phase(R') conj(phase(R))
        if (out_ratio) { out_ratio[2 * g] = (T)qr; out_ratio[2 * g + 1] = (T)qi; }
        double s[3];
        onebody_shift(A, shifts, g, s);
        q_s[t][0] = qr; q_s[t][1] = qi;
        for (int c = 0; c < 3; ++c) s_s[t][c] = s[c];
        spin_s[t] = (isfinite(qr) && isfinite(qi)) ? sp : -1 - sp;
    }
    __syncthreads();
    double* P = part + (long long)blockIdx.x * OB_ROW;
    const int t0 = wave * (OB_GROUP / OB_WAVES), t1 = min(ns, t0 + OB_GROUP / OB_WAVES);
    for (int kb = 0; kb < n_k; kb += 64) {              // (uniform over the workgroup: every wave meets both barriers)
        const int k = kb + lane;
        double a0r = 0.0, a0i = 0.0, a1r = 0.0, a1i = 0.0;
        if (k < n_k) {
            const double k0 = kvec[3 * k], k1 = kvec[3 * k + 1], k2 = kvec[3 * k + 2];
            for (int t = t0; t < t1; ++t) {
                const int sp = spin_s[t];
                if (sp < 0) continue;
                double sn, cs;
                sincos(k0 * s_s[t][0] + k1 * s_s[t][1] + k2 * s_s[t][2], &sn, &cs);
                const double qr = q_s[t][0], qi = q_s[t][1];
                const double cr = qr * cs + qi * sn, ci = qi * cs - qr * sn;              // q exp(-i k.s)
                if (sp == 0) { a0r += cr; a0i += ci; } else { a1r += cr; a1i += ci; }
            }
        }
        w_s[wave][lane][0] = a0r; w_s[wave][lane][1] = a0i; w_s[wave][lane][2] = a1r; w_s[wave][lane][3] = a1i;
        __syncthreads();
        if (wave == 0 && k < n_k) {
            double r[4];
            for (int c = 0; c < 4; ++c) {
                r[c] = w_s[0][lane][c];
                for (int v = 1; v < OB_WAVES; ++v) r[c] += w_s[v][lane][c];
            }
            P[k * 2] = r[0]; P[k * 2 + 1] = r[1]; P[(n_k + k) * 2] = r[2]; P[(n_k + k) * 2 + 1] = r[3];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) {
        int bad = 0;
        for (int t = 0; t < ns; ++t) bad += spin_s[t] == -1 - (int)threadIdx.x;
        P[4 * n_k + threadIdx.x] = (double)bad;
    }
}

// acc[i] (i < 4 n_k) = the call's running sum of the part rows in group order, begun at 0 by the call's first chunk; the last
// chunk adds it to the caller's buffer: sums[i] += acc[i], ONE addition per call and entry, so a second call on the same input
// doubles a buffer exactly.  n_bad[sp] += the rows' bad counts (exact small integers).
__global__ void __launch_bounds__(256) k_onebody_final(const double* __restrict__ part, long long n_groups, int n_k, int first,
                                                       int last, double* __restrict__ acc, double* __restrict__ sums,
                                                       long long* __restrict__ n_bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * n_k + 2) return;
    if (i < 4 * n_k) {
        double s = first ? 0.0 : acc[i];
#pragma unroll 8
        for (long long g = 0; g < n_groups; ++g) s += part[g * OB_ROW + i];      // (unrolled: the loads of 8 rows are in flight together)
        if (last) sums[i] += s;
        else acc[i] = s;
    } else if (n_bad) {
        long long b = 0;
        for (long long g = 0; g < n_groups; ++g) b += (long long)part[g * OB_ROW + i];
        n_bad[i - 4 * n_k] += b;
    }
}

}  // namespace ds
