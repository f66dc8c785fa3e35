// ds_ecp_force.h -- the ionic forces of the semi-local pseudopotential of ds_ecp.h: minus the derivative of E_loc + E_nl in the ion
// positions, per walker and ion of the simulation cell (include/deepsolid_hip.h has the normative text).
//
// Held fixed under the derivative: psi as a function of the electron coordinates, the rotation of the call, the electron positions
// and the image choice.  Per pair p = (w, i, I) inside r_cut_nl, with d the minimum image of r_i - R_I, r = |d|, dhat = d / r,
// U_q = Rot_w u_q, c_q = U_q . dhat, rho_q = psi(R'_q) / psi(R) and g_q = the three complex components of electron i of
// grad log psi at R'_q (d d / d R_I = -1, d r'_a / d R_b = delta_ab - U_qa dhat_b):
//   F^loc_I(w) = sum_i [r_iI < r_cut_loc,I] v'_loc,I(r) dhat
//   F^nl_I(w)  = sum_{i: r_iI < r_cut_nl,I} sum_q (1 / N_q) rho_q { D_q - W_q (g_q - (g_q . U_q) dhat) }
//   D_q = sum_l (2l + 1) [ v'_l(r) P_l(c_q) dhat + v_l(r) P'_l(c_q) (U_q - c_q dhat) / r ],   W_q = sum_l (2l + 1) v_l(r) P_l(c_q)
//   v'(r) = sum_k c_k [ (n_k - 2) r^(n_k - 3) - 2 zeta_k r^(n_k - 1) ] exp(-zeta_k r^2)
// The radial functions are exactly 0 outside their cutoffs; the delta term of the jump at a cutoff is left out.
//
//   (k_ecp_scan, k_ecp_offsets, k_ecp_fill of ds_ecp.h: the rotation, the counts, the offsets and the pair records, unchanged)
//   k_ecp_force_local  one thread per walker: F^loc of every ion, the electrons added in order i = 0 .. N-1 (the (i, I) order of
//                      E_loc restricted to one ion), into the walker's (A, 3) block; a pair at r = 0 inside either cutoff flags
//                      the walker
//   k_ecp_fill_deriv   one thread per pair: v'_l(r) of the pair's record, the second record array (the first one, which T-moves
//                      and DMC read, is not touched)
//   (forward-Laplacian chain with the gradient output on the chunk: log|psi(R')|, phase(R'), grad log psi(R'))
//   k_ecp_force_term   one thread per configuration of a chunk: rho_q as k_ecp_term forms it, the complex 3-vector
//                      (rho_q / N_q) { D_q - W_q (g_q - (g_q . U_q) dhat) } into the call's term buffer: component k of
//                      configuration c at term[k stride + c], k = 2 axis + (0: Re, 1: Im), so that the walker kernel reads runs
//   k_ecp_force_walker after the last chunk, one workgroup of ECPF_WAVES waves per walker; wave v takes the ions v, v + ECPF_WAVES,
//                      ...; for its ion lane l adds the terms of the walker's configurations l, l + 64, ... in order whose pair
//                      belongs to the ion, then the 64 lane results go through the fixed tree (l += l + s, s = 32 .. 1)
//                      -> out_force[w][I][axis] = (F^loc, Re F^nl, Im F^nl) and the rows [w][2][A][3] = (F^pp, F^tot) that
//                      k_force_part (ds_force.h) reads; F^pp = F^loc + Re F^nl, F^tot = F^pp + base
// The order of every addition is a function of the walker's pair list alone and the chunks only decide which launch computes a
// term; the chain is per-walker bit-independent of its batch: the results are bit-identical for any workspace size and from run
// to run.  No floating-point atomics.  Geometry, radial functions and Legendre polynomials are float64 for either element type;
// products and sums are rounded one by one (no contraction), so a host replay is exact up to exp.
#pragma once
#include "ds_ecp.h"

namespace ds {

constexpr int ECPF_WAVES = 4;          // waves per workgroup of k_ecp_force_walker

// v'(r) of table slot `slot`: the terms added in table order
__device__ __forceinline__ double ecp_radial_deriv(const EcpDev& E, int slot, double r) {
    double v = 0.0;
    {
#pragma clang fp contract(off)
        const double r2 = r * r, r3 = r2 * r;
        for (int k = E.term_off[slot]; k < E.term_off[slot + 1]; ++k) {
            const int n = E.term_n[k];
            const double lo = n == 0 ? 1.0 / r3 : n == 1 ? 1.0 / r2 : n == 2 ? 1.0 / r : n == 3 ? 1.0 : r;        // r^(n - 3)
            const double hi = n == 0 ? 1.0 / r : n == 1 ? 1.0 : n == 2 ? r : n == 3 ? r2 : r3;                    // r^(n - 1)
            const double z = E.term_z[k];
            v = v + (E.term_c[k] * ((double)(n - 2) * lo - (2.0 * z) * hi)) * exp(-(z * r2));
        }
    }
    return v;
}

// floc (B, A, 3); badf (B,): bad[w] of k_ecp_scan, or a pair at r = 0 inside a cutoff
template <typename T>
__global__ void __launch_bounds__(64) k_ecp_force_local(EcpDev E, const T* __restrict__ x, long long B, int N, const int* __restrict__ bad,
                                                        double* __restrict__ floc, int* __restrict__ badf) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B) return;
    double* fw = floc + w * 3 * E.n_atoms;
    if (bad[w]) {
        for (int k = 0; k < 3 * E.n_atoms; ++k) fw[k] = __builtin_nan("");
        badf[w] = 1;
        return;
    }
    const T* xw = x + w * 3 * N;
    int zero = 0;
    for (int I = 0; I < E.n_atoms; ++I) {
        const int sp = E.atom_species[I];
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        for (int i = 0; i < N; ++i) {
            const double p[3] = {(double)xw[3 * i], (double)xw[3 * i + 1], (double)xw[3 * i + 2]};
            double dh[3];
            const double r = ecp_min_image(E, p, I, dh);
            const bool loc = r < E.rc_loc[sp];
            zero |= (loc || ecp_nonlocal(E, sp, r)) && !(r > 0.0);
            if (loc) {
#pragma clang fp contract(off)
                const double dv = ecp_radial_deriv(E, sp * ECP_SLOTS, r);
                f0 = f0 + dv * dh[0]; f1 = f1 + dv * dh[1]; f2 = f2 + dv * dh[2];
            }
        }
        fw[3 * I] = f0; fw[3 * I + 1] = f1; fw[3 * I + 2] = f2;
    }
    badf[w] = zero;
}

// pdv (pairs, 3) = (v'_0, v'_1, v'_2)(r) of the pair records, 0 for the channels the species does not have
__global__ void __launch_bounds__(256) k_ecp_fill_deriv(EcpDev E, long long pairs, const int* __restrict__ pi, const double* __restrict__ pr,
                                                        double* __restrict__ pdv) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pairs) return;
    const int sp = E.atom_species[pi[2 * p + 1]];
    const double r = pr[4 * p];
    for (int l = 0; l < ECP_MAX_L; ++l) pdv[3 * p + l] = l < E.n_l[sp] ? ecp_radial_deriv(E, sp * ECP_SLOTS + 1 + l, r) : 0.0;
}

// term (6, stride): the complex 3-vector of configuration c0 + j; grad (n, 3N, 2) of the chunk's rows
template <typename T>
__global__ void __launch_bounds__(256) k_ecp_force_term(EcpDev E, EcpChunk A, const double* __restrict__ rot, const long long* __restrict__ pw,
                                                        const int* __restrict__ pi, const double* __restrict__ pr,
                                                        const double* __restrict__ pv, const double* __restrict__ pdv,
                                                        const T* __restrict__ la0, const T* __restrict__ ph0, const T* __restrict__ la,
                                                        const T* __restrict__ ph, const T* __restrict__ grad, long long stride,
                                                        double* __restrict__ term) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.n) return;
    const long long c = A.c0 + j, p = c / A.n_quad, w = pw[p];
    double U[3];
    ecp_point(E, rot + 9 * w, (int)(c % A.n_quad), U);
    const double r = pr[4 * p], dh[3] = {pr[4 * p + 1], pr[4 * p + 2], pr[4 * p + 3]};
    const T* g = grad + ((size_t)j * A.N + pi[2 * p]) * 6;
    const double mag = exp((double)la[j] - (double)la0[w]);
    const double pr_ = (double)ph[2 * j], pi_ = (double)ph[2 * j + 1], rr = (double)ph0[2 * w], ri = (double)ph0[2 * w + 1];
    const double iq = 1.0 / (double)A.n_quad;
    {
#pragma clang fp contract(off)
        const double qr = (mag * (pr_ * rr + pi_ * ri)) * iq, qi = (mag * (pi_ * rr - pr_ * ri)) * iq;     // rho_q / N_q
        const double t = (U[0] * dh[0] + U[1] * dh[1]) + U[2] * dh[2];
        const double p2 = 0.5 * (3.0 * t * t - 1.0);
        const double v0 = pv[3 * p], v1 = 3.0 * pv[3 * p + 1], v2 = 5.0 * pv[3 * p + 2];
        const double W = (v0 + v1 * t) + v2 * p2;
        const double radial = (pdv[3 * p] + (3.0 * pdv[3 * p + 1]) * t) + (5.0 * pdv[3 * p + 2]) * p2;     // sum (2l+1) v'_l P_l
        const double angular = (v1 + v2 * (3.0 * t)) / r;                                                  // sum (2l+1) v_l P'_l / r
        double gr[3], gi[3];
        for (int k = 0; k < 3; ++k) { gr[k] = (double)g[2 * k]; gi[k] = (double)g[2 * k + 1]; }
        const double gur = (gr[0] * U[0] + gr[1] * U[1]) + gr[2] * U[2], gui = (gi[0] * U[0] + gi[1] * U[1]) + gi[2] * U[2];
        for (int k = 0; k < 3; ++k) {
            const double D = radial * dh[k] + angular * (U[k] - t * dh[k]);
            const double br = D - W * (gr[k] - gur * dh[k]), bi = -(W * (gi[k] - gui * dh[k]));
            term[(2 * k) * stride + c] = qr * br - qi * bi;
            term[(2 * k + 1) * stride + c] = qr * bi + qi * br;
        }
    }
}

// out_force (B, A, 3, 3), rows (B, 2, A, 3), both optional; base (B, A, 3) optional.  A walker that is flagged, or has a non-finite
// result, gets NaN everywhere and is counted
__global__ void __launch_bounds__(64 * ECPF_WAVES) k_ecp_force_walker(const double* __restrict__ term, long long stride,
                                                                      const long long* __restrict__ off, const int* __restrict__ pi,
                                                                      const double* __restrict__ floc, const int* __restrict__ badf,
                                                                      const double* __restrict__ base, int A, int n_quad,
                                                                      double* __restrict__ out_force, double* __restrict__ rows,
                                                                      unsigned long long* __restrict__ n_bad) {
    __shared__ double l_s[ECPF_WAVES][6][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = blockIdx.x;
    const int flagged = badf[w];                       // (uniform over the workgroup)
    const long long c0 = off[w] * n_quad, c1 = flagged ? c0 : off[w + 1] * n_quad;
    double* of = out_force ? out_force + w * 9 * A : nullptr;
    double* rw = rows ? rows + w * 6 * A : nullptr;
    int nonfinite = flagged;
    for (int I0 = 0; I0 < A; I0 += ECPF_WAVES) {
        const int I = I0 + wave;
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (I < A)
            for (long long c = c0 + lane; c < c1; c += 64)
                if (pi[2 * (c / n_quad) + 1] == I)
                    for (int k = 0; k < 6; ++k) acc[k] += term[k * stride + c];
        __syncthreads();                               // the previous round's readers are done
        for (int k = 0; k < 6; ++k) l_s[wave][k][lane] = acc[k];
        for (int s = 32; s > 0; s >>= 1) {
            __syncthreads();
            if (lane < s)
                for (int k = 0; k < 6; ++k) l_s[wave][k][lane] += l_s[wave][k][lane + s];
        }
        __syncthreads();
        if (I < A && lane < 3) {
            const long long e = (w * A + I) * 3 + lane;
            const double fl = floc[e], re = l_s[wave][2 * lane][0], im = l_s[wave][2 * lane + 1][0];
            const double fpp = fl + re, ft = base ? fpp + base[e] : fpp;
            nonfinite |= !isfinite(fl) || !isfinite(re) || !isfinite(im) || !isfinite(ft);
            if (of) { of[9 * I + 3 * lane] = fl; of[9 * I + 3 * lane + 1] = re; of[9 * I + 3 * lane + 2] = im; }
            if (rw) { rw[3 * I + lane] = fpp; rw[3 * A + 3 * I + lane] = ft; }
        }
    }
    if (__syncthreads_or(nonfinite)) {
        const double nan = __builtin_nan("");
        for (int k = threadIdx.x; k < 9 * A; k += 64 * ECPF_WAVES)
            if (of) of[k] = nan;
        for (int k = threadIdx.x; k < 6 * A; k += 64 * ECPF_WAVES)
            if (rw) rw[k] = nan;
        if (threadIdx.x == 0 && n_bad) atomicAdd(n_bad, 1ull);
    }
}

}  // namespace ds
