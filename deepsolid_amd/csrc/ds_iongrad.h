// ds_iongrad.h -- the ion sink of the reverse sweep (ds_grad.h): d log psi_b / d R_a per walker b and atom a of the PRIMITIVE cell,
// behind ds_logpsi_ion_vjp.
//
// psi sees the ions only through the one-electron input features f(o), o = wrap(r_i) - R_a (k_features_val: nf rows per atom in
// every electron's layer-0 input, network.py:249-302), whose rows sd / rel also feed the envelope (network.py:335-364).  The pair
// stream reads neither.  The sweep (sweep_from_seed with the ion sink) has by then left
//   ZBAR [group][electron][n][PV]   cotangent of layer 0's pre-activation      SBAR [group][n][PV]   its sum over the electrons
//   HB   [group][electron][n][PV]   cotangent of layer 0's output (the carry of a first-layer residual)
//   QBAR [group][electron][p][re,im][PV]   cotangent of envelope x phase (dL = Re(QBAR dq))
// and the cotangent of feature row k = nf a + j of electron i is
//   fbar[k] = sum_n Wloc0[k][n] ZBAR[i][n]  +  (1 / n_s) sum_n Wsh0[s Kh + k][n] SBAR[n]   (s = spin of i: its share of the spin mean)
//           + HB[i][k] / sqrt2  (first-layer residual, k < nf A only: the rows beyond are padding and pair means)
//           + the envelope's:  isotropic   sd:    -sum_p ge pi exp(-r) sigma sign(sd sigma)
//                              diag / full rel_k: -sum_p ge pi exp(-r) sum_m u_m sigma[k][m] / r,    ge = Re(QBAR exp(i k.x))
// The nf A x Nout products are formed HERE, not by the sweep's GEMM on two more transposes: they are nf A <= a few dozen rows
// (2 nf A Nout products per electron against Kloc Nout of one hidden layer's W * ZBAR), the GEMM would pad them to 64 rows, need a
// padded output buffer of its own, and round them in the handle's dtype; in this kernel they are float64 and cost no workspace.
//   out[b][a][:] = -sum_i J(o)^T fbar,   J = d f / d o  (d/dR = -d/do)
//
// k_ion_grad: grid (A, groups), block 4 PV: thread (lane, c) = (tid / PV, tid % PV) walks the electrons lane, lane + 4, ... of walker
// c of the group for the workgroup's atom, the four partial 3-vectors meet in LDS and the thread of lane 0 adds them in lane order.
// The order of every addition is a function of (N, Nout, nparam) alone and a chunk of the batch is a whole number of groups: the
// result is bit-identical from run to run and for any workspace size.  No atomics.  All arithmetic is float64 for either handle
// dtype; the handle's tables, the parameters, x and the cotangent buffers (T) are converted on load.
#pragma once
#include "ds_value.h"

namespace ds {

// the features of one (electron, atom) in float64 with what their derivative in o needs: f[0] = sd, f[1..] = rel rows;
// dsd[l] = d sd / d w_l;  'nu': a1[l] = g'(w_l);  'tri': a1[l] = cos w_l, a2[l] = sin w_l          (w_l = o . b_l)
// Loops over the L <= 6 symmetry vectors are unrolled to the bound with a guard: the per-vector arrays are then indexed by
// constants and live in registers (a runtime trip count puts them into scratch memory).
#define DS_ION_FOR(l) _Pragma("unroll") for (int l = 0; l < 6; ++l) if (l < L)
struct IonFeat {
    double f[7], dsd[6], a1[6], a2[6];
};

// NF = 4: nu_distance_val, NF = 7: tri_distance_val (ds_value.h), with first derivatives.  d|w|/dw = sign(w), floor has none.
// The double sums over pairs of vectors are taken through the rel rows, which are linear in the vectors a_l (|a_l|^2 = n2_l):
//   'nu':  s2 = sum_l n2_l f_l^2 + sum_{l != m} (a_l . a_m) g_l g_m = sum_l n2_l (f_l^2 - g_l^2) + |rel|^2,        rel = sum_l a_l g_l
//   'tri': s2 = sum_{l,m} (a_l . a_m) ((1 - c_l)(1 - c_m) + s_l s_m) = |sum_l a_l (1 - c_l)|^2 + |sum_l a_l s_l|^2
// (the same polynomial, L products instead of L^2 and no Gram matrix of the vectors held in registers).
template <typename T, int NF>
__device__ __forceinline__ void ion_features(const double o[3], const T* __restrict__ av, const T* __restrict__ bv, int L, IonFeat& F) {
    const double pi = DS_PI;
    double s2 = 0;
    if (NF == 4) {
        double rel[3] = {0, 0, 0};
        DS_ION_FOR(l) {
            double w = o[0] * (double)bv[3 * l] + o[1] * (double)bv[3 * l + 1] + o[2] * (double)bv[3 * l + 2];
            w = w - floor((w + pi) / (2 * pi)) * 2 * pi;
            const double aw = fabs(w / pi), sg = w > 0 ? 1.0 : (w < 0 ? -1.0 : 0.0);
            const double f0 = fabs(w) * (1 - aw * aw * aw / 4), f1 = sg * (1 - aw * aw * aw);
            const double g0 = w * (1 - 1.5 * aw + 0.5 * aw * aw), g1 = 1 - 3 * aw + 1.5 * aw * aw;
            const double a0 = (double)av[3 * l], a1 = (double)av[3 * l + 1], a2 = (double)av[3 * l + 2], n2 = a0 * a0 + a1 * a1 + a2 * a2;
            s2 += n2 * (f0 * f0 - g0 * g0);
            rel[0] += a0 * g0; rel[1] += a1 * g0; rel[2] += a2 * g0;
            F.a1[l] = g1;
            F.dsd[l] = 2 * n2 * (f0 * f1 - g0 * g1);            // (completed below)
        }
        s2 += rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2];
        DS_ION_FOR(l)
            F.dsd[l] += 2 * F.a1[l] * ((double)av[3 * l] * rel[0] + (double)av[3 * l + 1] * rel[1] + (double)av[3 * l + 2] * rel[2]);
        for (int c = 0; c < 3; ++c) F.f[1 + c] = rel[c];
    } else {
        double P[3] = {0, 0, 0}, Q[3] = {0, 0, 0}, C[3] = {0, 0, 0};
        DS_ION_FOR(l) {
            sincos(o[0] * (double)bv[3 * l] + o[1] * (double)bv[3 * l + 1] + o[2] * (double)bv[3 * l + 2], &F.a2[l], &F.a1[l]);
            for (int c = 0; c < 3; ++c) {
                const double a = (double)av[3 * l + c];
                P[c] += a * (1 - F.a1[l]); Q[c] += a * F.a2[l]; C[c] += a * F.a1[l];
            }
        }
        s2 = P[0] * P[0] + P[1] * P[1] + P[2] * P[2] + Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2];
        DS_ION_FOR(l) {
            const double a0 = (double)av[3 * l], a1 = (double)av[3 * l + 1], a2 = (double)av[3 * l + 2];
            F.dsd[l] = 2 * ((a0 * P[0] + a1 * P[1] + a2 * P[2]) * F.a2[l] + (a0 * Q[0] + a1 * Q[1] + a2 * Q[2]) * F.a1[l]);
        }
        for (int c = 0; c < 3; ++c) { F.f[1 + c] = Q[c]; F.f[4 + c] = C[c]; }
    }
    const double sd = sqrt(s2);
    F.f[0] = sd;
    DS_ION_FOR(l) F.dsd[l] *= 0.5 / sd;
}

// go = J(o)^T fb: the cotangent of o from the cotangent of the NF feature rows
template <typename T, int NF>
__device__ __forceinline__ void ion_features_bwd(const IonFeat& F, const double fb[7], const T* __restrict__ av, const T* __restrict__ bv, int L,
                                                 double go[3]) {
    go[0] = go[1] = go[2] = 0;
    DS_ION_FOR(l) {
        double gw = fb[0] * F.dsd[l];
        for (int c = 0; c < 3; ++c) {
            const double a = (double)av[3 * l + c];
            if (NF == 4) gw += fb[1 + c] * a * F.a1[l];
            else gw += a * (fb[1 + c] * F.a1[l] - fb[4 + c] * F.a2[l]);
        }
        for (int c = 0; c < 3; ++c) go[c] += gw * (double)bv[3 * l + c];
    }
}

// out: (walkers of the chunk, A, 3) float64.  CARRY: HB of layer 0 when the reference adds a residual there, else null.
// Wloc0: (Kloc, Nout), Wsh0: (nch Kh, Nout) row-major as packed.  grid (A, groups), block 4 PV
template <typename T, int NF>
__global__ void __launch_bounds__(4 * PV) k_ion_grad(SysDev<T> S, const T* __restrict__ x, long Bc, const T* __restrict__ ZBAR,
                                                     const T* __restrict__ SBAR, const T* __restrict__ CARRY, int Nout,
                                                     const T* __restrict__ Wloc0, const T* __restrict__ Wsh0, const T* __restrict__ QBAR,
                                                     const T* __restrict__ env_pi0, const T* __restrict__ env_sg0,
                                                     const T* __restrict__ env_pi1, const T* __restrict__ env_sg1, double* __restrict__ out) {
    __shared__ double red[4][3][PV];
    const int a = blockIdx.x, g = blockIdx.y, lane = threadIdx.x / PV, c = threadIdx.x % PV, N = S.N, A = S.A, Kh = S.h1[0];
    const long wi = (long)g * PV + c;
    const long wr = wi < Bc ? wi : Bc - 1;              // (the tail of the last group repeats the last walker, as the value chain does)
    const double rs2 = 0.70710678118654752440;
    // the electron's share of the shared term is the same for every electron of a spin: formed when the thread's walk over the
    // electrons enters a spin (at most twice), the matrix-vector products first and the features behind them (registers)
    double sh[NF], acc[3] = {0, 0, 0};
    int sh_spin = -1;
    for (int i = lane; i < N; i += 4) {
        const int sp = spin_of(i, S.n_up), np = S.nparam[sp], no = S.norb[sp];
        if (sp != sh_spin) {
            sh_spin = sp;
            const double inv = 1.0 / (double)(sp == 0 ? S.n_up : S.n_dn);
            for (int k = 0; k < NF; ++k) sh[k] = 0;
#pragma unroll 2
            for (int n = 0; n < Nout; ++n) {
                const double z = (double)SBAR[((size_t)g * Nout + n) * PV + c];
                for (int k = 0; k < NF; ++k) sh[k] += (double)Wsh0[(size_t)(sp * Kh + NF * a + k) * Nout + n] * z;
            }
            for (int k = 0; k < NF; ++k) sh[k] *= inv;
        }
        double fb[7] = {0, 0, 0, 0, 0, 0, 0};
        const T* zb = ZBAR + ((size_t)(g * N + i) * Nout) * PV + c;
#pragma unroll 2
        for (int n = 0; n < Nout; ++n) {
            const double z = (double)zb[(size_t)n * PV];
            for (int k = 0; k < NF; ++k) fb[k] += (double)Wloc0[(size_t)(NF * a + k) * Nout + n] * z;
        }
        for (int k = 0; k < NF; ++k) fb[k] += sh[k];
        const T* xp = x + (size_t)wr * 3 * N + 3 * i;
        const double r[3] = {(double)xp[0], (double)xp[1], (double)xp[2]};
        // o = wrap(r) - R_a (wrap_point of ds_device.h on the primitive cell, k_features_val)
        double fr[3], o[3];
        for (int k = 0; k < 3; ++k) {
            const double f = r[0] * (double)S.prim_ainv[k] + r[1] * (double)S.prim_ainv[3 + k] + r[2] * (double)S.prim_ainv[6 + k];
            fr[k] = f - floor(f);
        }
        for (int k = 0; k < 3; ++k)
            o[k] = fr[0] * (double)S.prim_a[k] + fr[1] * (double)S.prim_a[3 + k] + fr[2] * (double)S.prim_a[6 + k] - (double)S.atoms[3 * a + k];
        IonFeat F;
        // (the table pointers pass through an empty asm statement in every iteration: the compiler then re-reads the few scalars where it
        //  needs them instead of keeping float64 copies of all of them in vector registers across the loop, which spilled)
        const T *avp = S.prim_AV, *bvp = S.prim_BV;
        asm volatile("" : "+s"(avp), "+s"(bvp));
        ion_features<T, NF>(o, avp, bvp, S.L, F);
        if (CARRY)       // rows n = NF a + k < NF A of HB only: a residual row beyond them meets padding or a pair mean, not a feature
            for (int k = 0; k < NF; ++k) fb[k] += (double)CARRY[((size_t)(g * N + i) * Nout + NF * a + k) * PV + c] * rs2;
        // envelope: e_p = sum_a pi[a,p] exp(-r_ap), cotangent ge = Re(QBAR exp(i k.x)) (k_env_grad)
        const T* pi_ = sp == 0 ? env_pi0 : env_pi1;
        const T* sg_ = sp == 0 ? env_sg0 : env_sg1;
        const T* qb = QBAR + ((size_t)(g * N + i) * S.nparam_max) * 2 * PV + c;
        for (int m = 0; m < no; ++m) {
            const T* kv = S.klist[sp] + 3 * m;
            double sn, cs;
            sincos((double)kv[0] * r[0] + (double)kv[1] * r[1] + (double)kv[2] * r[2], &sn, &cs);
            for (int p = m; p < np; p += no) {
                const double ge = (double)qb[(size_t)(2 * p) * PV] * cs - (double)qb[(size_t)(2 * p + 1) * PV] * sn;
                const double pv = (double)pi_[a * np + p];
                if (S.env_type == 0) {
                    const double sg = (double)sg_[a * np + p], u = F.f[0] * sg;
                    fb[0] -= ge * pv * exp(-fabs(u)) * sg * (u > 0 ? 1.0 : (u < 0 ? -1.0 : 0.0));
                } else {
                    double sk[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};        // sigma[k][m]
                    if (S.env_type == 1)
                        for (int k = 0; k < 3; ++k) sk[k][k] = (double)sg_[(a * 3 + k) * np + p];
                    else
                        for (int k = 0; k < 3; ++k)
                            for (int mm = 0; mm < 3; ++mm) sk[k][mm] = (double)sg_[((k * 3 + mm) * A + a) * np + p];
                    double u[3], r2 = 0;
                    for (int mm = 0; mm < 3; ++mm) {
                        u[mm] = sk[0][mm] * F.f[1] + sk[1][mm] * F.f[2] + sk[2][mm] * F.f[3];
                        r2 += u[mm] * u[mm];
                    }
                    const double rr = sqrt(r2);
                    if (rr > 0) {
                        const double w = ge * pv * exp(-rr) / rr;
                        for (int k = 0; k < 3; ++k) fb[1 + k] -= w * (u[0] * sk[k][0] + u[1] * sk[k][1] + u[2] * sk[k][2]);
                    }
                }
            }
        }
        double go[3];
        ion_features_bwd<T, NF>(F, fb, avp, bvp, S.L, go);
        for (int k = 0; k < 3; ++k) acc[k] -= go[k];
    }
    for (int k = 0; k < 3; ++k) red[lane][k][c] = acc[k];
    __syncthreads();
    if (lane == 0 && wi < Bc)
        for (int k = 0; k < 3; ++k) out[((size_t)wi * A + a) * 3 + k] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
}

#undef DS_ION_FOR

}  // namespace ds
