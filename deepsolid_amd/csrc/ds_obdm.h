// ds_obdm.h -- the one-body reduced density matrix in a basis of crystalline orbitals, folded from one-body ratios.
//
// The reference has no such estimator: the conventions are this project's own (include/deepsolid_hip.h).
// Sample g = w * M + m moves electron e = (first_electron + m) % N of walker w from r_e to r' = r_e + s; its spin is
// sp = e < n_up ? 0 : 1.  With the basis functions phi^sp_i (ds_hf.h; M_sp of them, any columns, not tied to the electrons) it adds
//     dm[sp][i][j] += w_s q conj(phi_i(r')) phi_j(r_e),      ov[sp][i][j] += w_s conj(phi_i(r')) phi_j(r'),
// q = psi(R') / psi(R) and s as ds_one_body_ratios exports them, w_s an optional weight.  A sample whose q or weight is not
// finite adds nothing and is counted; a spin without basis functions adds nothing and counts nothing.
//
//   k_obdm_basis       one wave per (sample of the chunk, r_e or r', group of 8 k points): hf_orbital_row of ds_hf.h -> PHI
//   k_obdm_accumulate  one workgroup of OBDM_WAVES waves per OBDM_GROUP consecutive samples.  Per spin, in stages of OBDM_STAGE
//                      samples through LDS: the planes Re / Im of phi(r') (rows of the left operand AND, times the weight, the
//                      columns of the overlap's right operand) and Re / Im of w_s q phi(r_e); a sample of the other spin, a bad
//                      one and one beyond the end are exact zeros.  A wave owns up to two tiles of 16 x 16 complex entries; per
//                      tile four real products RR, II, RI, IR on v_mfma_f64_16x16x4_f64 (mfma16), samples in index order, and
//                      conj(a) b = (RR + II) + i (RI - IR) lane by lane -> one row of partials per group
//   k_obdm_final       adds the rows in group order to the call's running sums, the last chunk's adds those to the caller's buffers
//
// A chunk starts at a multiple of OBDM_GROUP samples, so the groups -- and every addition and its order -- are the same however
// the workspace cuts the call into chunks: bit-identical sums for any workspace size and from run to run.  No atomics.
#pragma once
#include "ds_hf.h"

namespace ds {

constexpr int OBDM_GROUP = 128;        // samples per partial row
constexpr int OBDM_STAGE = 16;         // samples per LDS stage
constexpr int OBDM_WAVES = 8;
constexpr int OBDM_LD = HF_MAX_ORB + 16;   // plane row stride in doubles: 16 mod 32, so the four sample rows of an operand load
                                           // fall into different banks
static_assert(OBDM_GROUP % OBDM_STAGE == 0 && OBDM_STAGE % 4 == 0, "a group is whole stages, a stage whole MFMA steps");
static_assert(2 * OBDM_WAVES >= (HF_MAX_ORB / 16) * (HF_MAX_ORB / 16), "two tiles per wave cover the largest matrix");

struct ObdmArgs {
    long long g0, n;                   // first sample of the chunk, samples in the chunk
    int M, N, n_up, first;             // samples per walker, electrons, up electrons, first electron
    int Mb;                            // max(M_up, M_dn): the row length of PHI and of the caller's matrices
};

// doubles of one partial row: [spin][dm, ov][i][j][re, im] with i, j < Mb, then the bad count of either spin
__host__ __device__ inline long long obdm_row(int Mb) { return 8LL * Mb * Mb + 2; }

// r' of a sample: the expression of k_onebody_propose, in the walkers' type, then widened
template <typename T> __device__ __forceinline__ double obdm_moved(T r, T s) { return (double)(T)((double)r + (double)s); }

// PHI[which][j][o]: complex128 basis values of sample g0 + j at r_e (which = 0) and at r' (which = 1), o < M_sp of the sample's spin
template <typename T, int NT, int CH>
__global__ __launch_bounds__(64) void k_obdm_basis(HfArgs A, ObdmArgs O, const T* __restrict__ x, const T* __restrict__ shift,
                                                   double* __restrict__ phi) {
    const long long j = blockIdx.x >> 1;
    const int which = blockIdx.x & 1;
    if (j >= O.n) return;
    const long long g = O.g0 + j, w = g / O.M;
    const int e = (int)((O.first + g % O.M) % O.N);
    const int sp = e < O.n_up ? 0 : 1;
    if ((sp ? A.n_dn : A.n_up) == 0) return;             // (uniform over the workgroup)
    const T* xe = x + (w * O.N + e) * 3;
    double r[3];
    for (int c = 0; c < 3; ++c) r[c] = which ? obdm_moved(xe[c], shift[3 * g + c]) : (double)xe[c];
    hf_orbital_row<NT, CH>(A, r, sp, blockIdx.y, phi + 2 * ((which * O.n + j) * (long long)O.Mb));
}

template <typename T>
__global__ void __launch_bounds__(64 * OBDM_WAVES) k_obdm_accumulate(ObdmArgs O, int M_up, int M_dn, const T* __restrict__ ratio,
                                                                     const double* __restrict__ weight,
                                                                     const double* __restrict__ phi, double* __restrict__ part) {
    __shared__ double pl[4][OBDM_STAGE][OBDM_LD];       // planes: Re phi(r'), Im phi(r'), Re w q phi(r_e), Im w q phi(r_e)
    __shared__ double sc[OBDM_GROUP][3];                // per sample: Re w q, Im w q, w  (zeros for a sample left out)
    __shared__ int spin_s[OBDM_GROUP];                  // 0 / 1, -1 - spin: bad, 2: beyond the end or a spin without basis functions
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long j0 = (long long)blockIdx.x * OBDM_GROUP;
    const int ns = (int)(O.n - j0 < OBDM_GROUP ? O.n - j0 : OBDM_GROUP);
    const int Ms[2] = {M_up, M_dn};
    for (int t = tid; t < OBDM_GROUP; t += 64 * OBDM_WAVES) {
        int code = 2;
        double wr = 0.0, wi = 0.0, wv = 0.0;
        if (t < ns) {
            const long long g = O.g0 + j0 + t;
            const int sp = (int)((O.first + g % O.M) % O.N) < O.n_up ? 0 : 1;
            if (Ms[sp] > 0) {
                const double qr = (double)ratio[2 * g], qi = (double)ratio[2 * g + 1];
                const double ww = weight ? weight[g] : 1.0;
                if (isfinite(qr) && isfinite(qi) && isfinite(ww)) {
                    code = sp; wr = ww * qr; wi = ww * qi; wv = ww;
                } else {
                    code = -1 - sp;
                }
            }
        }
        spin_s[t] = code;
        sc[t][0] = wr; sc[t][1] = wi; sc[t][2] = wv;
    }
    __syncthreads();

    typedef Acc4<double>::type acc_t;
    double* P = part + (long long)blockIdx.x * obdm_row(O.Mb);
    const double* phi_e = phi + 2 * j0 * (long long)O.Mb;                    // [t][o][re, im] at r_e
    const double* phi_n = phi + 2 * (O.n + j0) * (long long)O.Mb;            // ... at r'
    const int kk = lane >> 4, col = lane & 15;
    for (int sp = 0; sp < 2; ++sp) {                    // (every bound below is uniform over the workgroup: all waves meet the barriers)
        const int Msp = Ms[sp];
        if (Msp == 0) continue;
        const int nT = (Msp + 15) / 16, Mp = 16 * nT;
        // this wave's tiles u = wave, wave + OBDM_WAVES of the nT x nT complex tiles
        int ci[2], cj[2];
        bool on[2];
        for (int h = 0; h < 2; ++h) {
            const int u = wave + h * OBDM_WAVES;
            on[h] = u < nT * nT;
            ci[h] = on[h] ? u / nT : 0;
            cj[h] = on[h] ? u % nT : 0;
        }
        acc_t acc[2][2][4];                             // [tile][dm, ov][RR, II, RI, IR]
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[h][k][c] = acc_t{0, 0, 0, 0};
        for (int s0 = 0; s0 < OBDM_GROUP; s0 += OBDM_STAGE) {
            if (s0 >= ns) break;
            __syncthreads();                            // the previous stage has been read
            for (int i = tid; i < OBDM_STAGE * Mp; i += 64 * OBDM_WAVES) {
                const int tl = i / Mp, o = i - tl * Mp, t = s0 + tl;
                double nr = 0.0, ni = 0.0, er = 0.0, ei = 0.0;
                if (spin_s[t] == sp && o < Msp) {
                    const long long at = 2 * ((long long)t * O.Mb + o);
                    nr = phi_n[at]; ni = phi_n[at + 1];
                    const double fr = phi_e[at], fi = phi_e[at + 1], wr = sc[t][0], wi = sc[t][1];
                    er = wr * fr - wi * fi;
                    ei = wr * fi + wi * fr;
                }
                pl[0][tl][o] = nr; pl[1][tl][o] = ni; pl[2][tl][o] = er; pl[3][tl][o] = ei;
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!on[h]) continue;                   // (uniform over the wave)
                const int oa = 16 * ci[h] + col, ob = 16 * cj[h] + col;
#pragma unroll
                for (int ks = 0; ks < OBDM_STAGE; ks += 4) {
                    const int tl = ks + kk;
                    const double ar = pl[0][tl][oa], ai = pl[1][tl][oa];
                    const double dr = pl[2][tl][ob], di = pl[3][tl][ob];
                    const double wv = sc[s0 + tl][2];
                    const double vr = wv * pl[0][tl][ob], vi = wv * pl[1][tl][ob];
                    acc[h][0][0] = mfma16(ar, dr, acc[h][0][0]);
                    acc[h][0][1] = mfma16(ai, di, acc[h][0][1]);
                    acc[h][0][2] = mfma16(ar, di, acc[h][0][2]);
                    acc[h][0][3] = mfma16(ai, dr, acc[h][0][3]);
                    acc[h][1][0] = mfma16(ar, vr, acc[h][1][0]);
                    acc[h][1][1] = mfma16(ai, vi, acc[h][1][1]);
                    acc[h][1][2] = mfma16(ar, vi, acc[h][1][2]);
                    acc[h][1][3] = mfma16(ai, vr, acc[h][1][3]);
                }
            }
        }
        // conj(a) b = (RR + II) + i (RI - IR)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!on[h]) continue;
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int i = 16 * ci[h] + acc_row<double>(lane, g), j = 16 * cj[h] + col;
                    if (i < Msp && j < Msp) {
                        double* o = P + 2 * (((long long)(2 * sp + k) * O.Mb + i) * O.Mb + j);
                        o[0] = acc[h][k][0][g] + acc[h][k][1][g];
                        o[1] = acc[h][k][2][g] - acc[h][k][3][g];
                    }
                }
        }
    }
    if (tid < 2) {
        int bad = 0;
        for (int t = 0; t < ns; ++t) bad += spin_s[t] == -1 - tid;
        P[8LL * O.Mb * O.Mb + tid] = (double)bad;
    }
}

// acc[i] = the call's running sum of the part rows in group order, begun at 0 by the call's first chunk; the last chunk adds it to
// the caller's buffer: ONE addition per call and entry, so a second call on the same input doubles a buffer exactly.  Entries
// with a row or a column >= M_sp are neither read nor written.  n_bad[sp] += the rows' bad counts (exact small integers).
__global__ void __launch_bounds__(256) k_obdm_final(const double* __restrict__ part, long long n_groups, int Mb, int M_up, int M_dn,
                                                    int first, int last, double* __restrict__ acc, double* __restrict__ dm,
                                                    double* __restrict__ ov, long long* __restrict__ n_bad) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long body = 8LL * Mb * Mb, row = body + 2;
    if (i >= row) return;
    if (i < body) {
        const int per = 2 * Mb * Mb;
        const int blk = (int)(i / per), rem = (int)(i - (long long)blk * per);     // blk = 2 spin + kind
        const int sp = blk >> 1, kind = blk & 1, r = rem / (2 * Mb), c = (rem / 2) % Mb;
        const int Msp = sp ? M_dn : M_up;
        if (r >= Msp || c >= Msp) return;
        double s = first ? 0.0 : acc[i];
#pragma unroll 8
        for (long long g = 0; g < n_groups; ++g) s += part[g * row + i];
        if (!last) { acc[i] = s; return; }
        double* out = kind ? ov : dm;
        if (out) out[(long long)sp * per + rem] += s;
    } else if (n_bad) {
        long long b = 0;
        for (long long g = 0; g < n_groups; ++g) b += (long long)part[g * row + i];
        n_bad[i - body] += b;
    }
}

}  // namespace ds
