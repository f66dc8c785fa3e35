// ds_obs.h -- the two walker observables of the reference's estimator.py, reduced over the batch.
//
// Reference: DeepSolid/estimator.py:15-42 (complex polarization) and :44-84 (structure factor S(k) on an nq^3 grid of
// simulation-cell reciprocal lattice vectors).  One call turns walkers x (B, 3N) into float64 SUMS over the batch:
//   out[0], out[1]             = sum_b Re P_b, sum_b Im P_b           P_b = exp(i sum_e g_pol . r_be)
//   out[2 + k], out[2 + Q + k] = sum_b Re rho_b(q_k), Im rho_b(q_k)   rho_b(q) = sum_e exp(i q . r_be)
//   out[2 + 2Q + k]            = sum_b |rho_b(q_k)|^2                 k < Q
// The means, the cross-rank pmean and S(k) = (<|rho|^2> - |<rho>|^2) / N are host algebra (deepsolid_amd/estimator.py).
//
// q_k = n1 g_1 + n2 g_2 + n3 g_3 is a lattice vector of the simulation cell, so exp(i q.r) = z1^n1 z2^n2 z3^n3 with
// z_j = exp(i g_j . r): three float64 sincos per electron instead of Q.  The polarization phase g_pol . r is one of the three
// dots; it is summed over the electrons first and then takes one sincos per walker, as the reference does.
//
// Layout: one wave per workgroup, walkers b = blockIdx.x, blockIdx.x + G, ... in turn; lane l owns the points q = l + 64 j.
// Per chunk of 64 electrons each lane computes its electron's z_j and writes the powers z_j^0..z_j^(P-1) to LDS; after the
// barrier every lane walks the chunk's table rows in order and multiplies its points' three powers out of the table.
// An electron's row is not its index but its slot in the chunk's order by coordinate bit patterns (64 integer comparisons per
// lane out of LDS): electrons are identical particles, and with the slots the sums of a walker do not depend on how a chunk's
// electrons are numbered -- permuting them leaves every bit.  (Across chunks the numbering still decides which chunk an
// electron is in, so there only the rounding bound holds.)  The polarization phase goes through LDS by slot as well.
// Reduction order is fixed, so two calls on the same input are bit-identical: the chunks in index order, slots in order inside
// a chunk, the walkers of one workgroup in the order it visits them, then k_obs_final adds the G workgroup partials in
// workgroup order.  No atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace ds {

constexpr int OBS_MAX_N = 128;         // electrons per walker (every cell the library accepts)
constexpr int OBS_MAX_Q = 512;         // nq <= 8
constexpr int OBS_MAX_POW = 8;         // lattice coordinates 0 <= n_j < OBS_MAX_POW
constexpr int OBS_MAX_GROUPS = 1024;   // workgroups of the partial pass (and rows of the workspace)
constexpr int OBS_TAB = 3 * OBS_MAX_POW + 1;   // table row of one electron in double2, +1 against bank conflicts of the writes

struct ObsArgs {
    double g[9];                       // simulation-cell reciprocal vectors, row j = g_j (2 pi inv(a)^T)
    int n_q;                           // number of q points (0: polarization only)
    int n_pow;                         // powers kept per direction: max n_j + 1
    int pol;                           // polarization direction 0..2, -1: none
    signed char qn[OBS_MAX_Q * 3];     // (n1, n2, n3) of every point
};

__host__ __device__ inline int obs_groups(long long B) { return (int)(B < OBS_MAX_GROUPS ? B : OBS_MAX_GROUPS); }

// partial pass: part[blockIdx.x * K + k], K = 2 + 3 n_q, in the order of the packed output
template <typename T, int QJ>
__global__ __launch_bounds__(64) void k_obs_partial(ObsArgs A, const T* __restrict__ x, long long B, int N,
                                                    double* __restrict__ part) {
    __shared__ double2 tab[64][OBS_TAB];
    __shared__ long long key0[64];     // bit patterns of the chunk's coordinates: the first,
    __shared__ long long key[64][3];   // and the other two ([1], [2]) for chunks where two first coordinates are equal
    __shared__ double dps[64];         // polarization phases of the chunk, by slot
    const int lane = threadIdx.x;
    const int G = gridDim.x;
    const int nq = A.n_q;
    int o1[QJ], o2[QJ], o3[QJ];        // table slots of this lane's points
#pragma unroll
    for (int j = 0; j < QJ; ++j) {
        const int q = lane + 64 * j;
        const bool ok = q < nq;
        o1[j] = ok ? A.qn[3 * q] : 0;
        o2[j] = OBS_MAX_POW + (ok ? A.qn[3 * q + 1] : 0);
        o3[j] = 2 * OBS_MAX_POW + (ok ? A.qn[3 * q + 2] : 0);
    }
    double acc_re[QJ], acc_im[QJ], acc_sq[QJ];
#pragma unroll
    for (int j = 0; j < QJ; ++j) acc_re[j] = acc_im[j] = acc_sq[j] = 0.0;
    double pol_re = 0.0, pol_im = 0.0;

    for (long long b = blockIdx.x; b < B; b += G) {
        const T* xb = x + b * 3 * (long long)N;
        double rre[QJ], rim[QJ];
#pragma unroll
        for (int j = 0; j < QJ; ++j) rre[j] = rim[j] = 0.0;
        double dpol = 0.0;
        for (int e0 = 0; e0 < N; e0 += 64) {
            const int ne = N - e0 < 64 ? N - e0 : 64;
            double r0 = 0.0, r1 = 0.0, r2 = 0.0;
            if (lane < ne) {
                const T* r = xb + 3 * (e0 + lane);
                r0 = (double)r[0], r1 = (double)r[1], r2 = (double)r[2];
                key[lane][1] = __double_as_longlong(r1);
                key[lane][2] = __double_as_longlong(r2);
            }
            // slot of this electron in the chunk: the number of electrons before it in the lexicographic order of the
            // coordinates' bit patterns (equal electrons, whose terms are equal too, in lane order): a permutation of 0..ne-1.
            // The first coordinate decides unless two electrons of the chunk share its bits; lanes without an electron hold
            // the largest key and come last.
            const long long k0 = lane < ne ? __double_as_longlong(r0) : 0x7fffffffffffffffLL;
            key0[lane] = k0;
            __syncthreads();
            int slot = 0;
            bool tie = false;
#pragma unroll 16
            for (int m = 0; m < 64; ++m) {
                const long long m0 = key0[m];
                slot += (m0 < k0 || (m0 == k0 && m < lane)) ? 1 : 0;
                tie = tie || (m0 == k0 && m != lane);
            }
            if (__any(tie && lane < ne) && lane < ne) {
                const long long k1 = key[lane][1], k2 = key[lane][2];
                slot = 0;
                for (int m = 0; m < ne; ++m) {
                    const long long m0 = key0[m], m1 = key[m][1], m2 = key[m][2];
                    const bool same = m0 == k0 && m1 == k1 && m2 == k2;
                    const bool less = m0 < k0 || (m0 == k0 && (m1 < k1 || (m1 == k1 && m2 < k2)));
                    slot += (less || (same && m < lane)) ? 1 : 0;
                }
            }
            if (lane < ne) {
                double d[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = A.g[3 * c] * r0 + A.g[3 * c + 1] * r1 + A.g[3 * c + 2] * r2;
                dps[slot] = A.pol == 0 ? d[0] : (A.pol == 1 ? d[1] : (A.pol == 2 ? d[2] : 0.0));
                if (nq > 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double s, co;
                        sincos(d[c], &s, &co);
                        double wr = 1.0, wi = 0.0;
                        for (int p = 0; p < A.n_pow; ++p) {
                            tab[slot][c * OBS_MAX_POW + p] = make_double2(wr, wi);
                            const double tr = wr * co - wi * s;
                            wi = wr * s + wi * co;
                            wr = tr;
                        }
                    }
                }
            }
            __syncthreads();
            if (lane < ne) dpol += dps[lane];
            for (int e = 0; e < ne; ++e) {
#pragma unroll
                for (int j = 0; j < QJ; ++j) {
                    const double2 a = tab[e][o1[j]], u = tab[e][o2[j]], v = tab[e][o3[j]];
                    const double ar = a.x * u.x - a.y * u.y, ai = a.x * u.y + a.y * u.x;
                    rre[j] += ar * v.x - ai * v.y;
                    rim[j] += ar * v.y + ai * v.x;
                }
            }
            __syncthreads();
        }
        // butterfly over the wave: every lane ends with the same bits (each step adds the same two values in either order)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) dpol += __shfl_xor(dpol, m, 64);
        if (A.pol >= 0) {
            double s, co;
            sincos(dpol, &s, &co);
            pol_re += co;
            pol_im += s;
        }
#pragma unroll
        for (int j = 0; j < QJ; ++j) {
            acc_re[j] += rre[j];
            acc_im[j] += rim[j];
            acc_sq[j] += rre[j] * rre[j] + rim[j] * rim[j];
        }
    }
    double* P = part + (long long)blockIdx.x * (2 + 3 * nq);
    if (lane == 0) {
        P[0] = pol_re;
        P[1] = pol_im;
    }
#pragma unroll
    for (int j = 0; j < QJ; ++j) {
        const int q = lane + 64 * j;
        if (q < nq) {
            P[2 + q] = acc_re[j];
            P[2 + nq + q] = acc_im[j];
            P[2 + 2 * nq + q] = acc_sq[j];
        }
    }
}

// final pass: out[k] = sum over the G partials in workgroup order
__global__ void k_obs_final(const double* __restrict__ part, int G, int K, double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(long long)g * K + k];
    out[k] = s;
}

}  // namespace ds
