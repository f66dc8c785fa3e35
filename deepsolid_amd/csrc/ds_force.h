// ds_force.h -- ionic forces of a batch of walkers: the Hellmann-Feynman (HF) force of the Ewald electron-ion and ion-ion energy
// and the Assaraf-Caffarel zero-variance (ZV) force F^zv = F^hf + dF.  The reference has no force
// estimator: the conventions are this library's own.
//
// Per walker R and ion a of the simulation cell (charge Z_a, position R_a), with v = mi(r_i - R_a) the minimal-image vector of
// k_ewald (ds_kernels.h: the image choice is held fixed under the derivative) and D_s its 27 lattice displacements:
//   F^hf_a = Z_a sum_i sum_s [erfc(alpha r) / r^2 + (2 alpha / sqrt pi) exp(-alpha^2 r^2) / r] (v + D_s) / r,  r = |v + D_s|
//          - 2 Z_a sum_G w_G G (sin(G.R_a) S_c(G) - cos(G.R_a) S_s(G)),   S_c + i S_s = sum_i exp(i G.r_i)
//          + F^ii_a                                                        (constant of the geometry: the caller's array)
//   dF_a   = sum_{i: r < r_c} [ -1/2 (g'' + 4 g'/r) u - g d_i - (g'/r) (u.d_i) u ],   g(r) = -Z_a c(r) / r,
//            c(r) = (1 - r^2/r_c^2)^3,   d_i = Re grad_i log psi,   r = |u|,   u = the TRUE nearest image of r_i - R_a
// u is not always v.  k_ewald's minimal image of a non-orthogonal cell that takes the fractional wrap (dist_mode 1: the bcc cells)
// is the nearest image only within half the smallest plane spacing, which is less than the Wigner-Seitz radius r_c may reach
// (bcc-Li: 4.58 against 5.61 bohr); that of dist_mode 2 looks one cell around the RAW difference, which a walker outside the cell
// defeats.  Q_a must be a periodic, continuous function of r_i, so the ZV term takes its own image: the fractional wrap of
// r_i - R_a, then the nearest of the 27 images around it.  With r_c below every plane spacing (an entry condition) that is the
// nearest image of the lattice for every r < r_c, wherever the walker is; inside r_c <= r_ws it is unique.  u is then matched
// to the image v + D_s* of F^hf that it equals; if there is none (dist_mode 2, walker cells away), dF is added as it stands.
// -1/2 (g'' + 4 g'/r) u = Z_a [c''/(2r) + c'/r^2] u - Z_a c u / r^3: the last piece cancels the 1/r^2 singularity of the s = s* term
// of F^hf.  F^zv is therefore NOT formed as F^hf + dF: the thread that owns the pair (i, s*) adds to its F^zv sum
//   Z_a v [ ((1 - c) - erf(alpha r)) / r^3 + (2 alpha / sqrt pi) exp(-alpha^2 r^2) / r^2 ]
// with 1 - c = (r^2/r_c^2)(1 + u + u^2), u = 1 - r^2/r_c^2, so that no 1/r^2 number of size Z/r^2 ever enters F^zv.
//
// All arithmetic is float64 for either handle dtype; the handle's tables (T), x and the drift (T) are converted on load.
//
//   k_ion_forces   one workgroup of 256 threads per walker:
//                    1. x and drift to LDS; a non-finite entry makes the walker bad
//                    2. per chunk of FORCE_GC G points: S_c, S_s of the chunk to LDS (phase tables when S.g_len > 0 and they fit,
//                       direct sincos otherwise), then ion by ion the reciprocal force of the chunk: thread t takes
//                       g = t, t + 256, ... in order, the 256 partial 3-vectors go through the LDS tree (t += t + s,
//                       s = 128 .. 1), and thread 0 adds the chunk's result to the ion's entry of an LDS array [A][3]
//                    3. ion by ion: minimal images of the N electrons and s* (thread t: electrons t, t + 256, ...) to LDS, then
//                       thread t takes the pairs
//                       (i, s) = t, t + 256, ... of the N x 27 in order (the pair with s = s* carries the ZV terms of
//                       electron i), the LDS tree over the six sums, and thread 0 writes
//                       F^hf = (real + reciprocal) + F^ii and F^zv likewise
//                  nothing of size A lives in registers.  A bad walker (non-finite input, or a non-finite result) gets NaN
//                  in every output and is counted.
//   k_force_part   one workgroup per FORCE_GROUP walkers of a pass: per (a, c) the four sums over the group's good walkers through
//                  the same LDS tree (thread t = walker t of the group), and the number of good walkers
//   k_force_final  sums[j] = (..((sums[j] + part[0][j]) + part[1][j]) + ..): the groups in order
// The order of every addition is a function of (N, A, NG, B) alone and groups are cut at multiples of FORCE_GROUP walkers of the
// batch, so the results are bit-identical from run to run and for any workspace size.  No floating-point atomics.
//
// LDS (MI355X: 160 KB per CU): 10N + 6 x 256 + 81 + 3A + 2 FORCE_GC doubles = 38.6 KB + 24 A bytes at N = 128, plus the current ion's
// phase table (2 g_len doubles) and the electrons' (2 N g_len doubles).  The handle bounds g_len only through N g_len (a long
// cell with one to three electrons reaches thousands of entries) and A not at all, so force_table_flags keeps what fits into
// FORCE_LDS_MAX = 64 KB (two workgroups, eight waves, per CU at the cap): both tables, else the ion's alone (the structure
// factors then take the direct sincos path), else none (the ion phases too); a cell whose layout without tables exceeds the
// cap (about 1000 ions) is refused before any launch.
#pragma once
#include <hip/hip_runtime.h>

#include "ds_kernels.h"

namespace ds {

constexpr int FORCE_GC = 1024;          // G points per chunk of the structure-factor sums in LDS
constexpr int FORCE_GROUP = 256;        // walkers per row of partial sums
constexpr size_t FORCE_LDS_MAX = 64 * 1024;
static_assert(FORCE_GROUP == 256, "force_tree is written for 256 threads");

// which phase tables a launch keeps in LDS
constexpr int FORCE_ION_TABLE = 1;      // the current ion's (2 g_len doubles)
constexpr int FORCE_EL_TABLES = 2;      // the N electrons' (2 N g_len doubles); only together with the ion's

// doubles of dynamic LDS of k_ion_forces for the tables in `flags`
template <typename T> inline size_t force_lds_doubles(const SysDev<T>& S, int flags) {
    return (size_t)10 * S.N + 6 * 256 + 81 + (size_t)3 * S.As + 2 * (size_t)FORCE_GC +
           ((flags & FORCE_ION_TABLE) ? 2 * (size_t)S.g_len : 0) + ((flags & FORCE_EL_TABLES) ? 2 * (size_t)S.N * S.g_len : 0);
}
// the tables that fit into FORCE_LDS_MAX (the handle bounds g_len only through N g_len, and A not at all); -1: not even the layout
// without tables does (more than about 1000 ions): the call is refused before any launch
template <typename T> inline int force_table_flags(const SysDev<T>& S) {
    int flags = -1;
    for (int f : {0, FORCE_ION_TABLE, FORCE_ION_TABLE | FORCE_EL_TABLES})
        if ((f == 0 || S.g_len > 0) && force_lds_doubles(S, f) * sizeof(double) <= FORCE_LDS_MAX) flags = f;
    return flags;
}

// the fixed tree over the 256 threads on NV arrays red[v][256]; the result is in red[v][0] after the last barrier
template <int NV> __device__ __forceinline__ void force_tree(double* red, int tid) {
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off)
            for (int v = 0; v < NV; ++v) red[256 * v + tid] += red[256 * v + tid + off];
        __syncthreads();
    }
}

// exp(i n theta_j) of one point with fractional coordinates from `p`, table entry t of the handle's layout (k_ewald)
template <typename T>
__device__ __forceinline__ void force_phase_entry(const SysDev<T>& S, const double p[3], int t, double* cs, double* sn) {
    const int j = t >= S.g_off[2] ? 2 : (t >= S.g_off[1] ? 1 : 0);
    const double nn = (double)(S.g_nmin[j] + (t - S.g_off[j]));
    const double frac = p[0] * (double)S.sim_ainv[j] + p[1] * (double)S.sim_ainv[3 + j] + p[2] * (double)S.sim_ainv[6 + j];
    sincos(nn * (6.283185307179586476925286766559 * frac), sn, cs);
}

// rows (optional): [walker of the launch][2][A][3] = (F^hf, F^zv), what k_force_part reads
template <typename T>
__global__ void __launch_bounds__(256) k_ion_forces(SysDev<T> S, const T* __restrict__ x, const T* __restrict__ drift, double r_c, double r_in,
                                                    const double* __restrict__ ion_ion, int tables, double* __restrict__ out_hf,
                                                    double* __restrict__ out_zv, double* __restrict__ rows,
                                                    unsigned long long* __restrict__ n_bad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = S.N, A = S.As, L = S.g_len, NG = S.NG;
    double* xs = reinterpret_cast<double*>(smem_raw);   // [N][3]
    double* ds_ = xs + 3 * N;                           // [N][3] drift
    double* vmi = ds_ + 3 * N;                          // [N][3] minimal images of the current ion
    double* snear = vmi + 3 * N;                        // [N] the displacement s that gives the nearest image of electron i (as a double)
    double* red = snear + N;                            // [6][256]
    double* dsp = red + 6 * 256;                        // [27][3] the lattice displacements D_s (the searches below walk them serially)
    double* frec = dsp + 81;                            // [A][3] reciprocal force
    double* sg = frec + 3 * A;                          // [FORCE_GC][2] = (S_c, S_s) of the chunk
    const bool ion_table = tables & FORCE_ION_TABLE, use_tables = tables & FORCE_EL_TABLES;
    double* tabA = sg + 2 * FORCE_GC;                   // [g_len][2] phase table of the current ion (ion_table)
    double* tab = tabA + (ion_table ? 2 * L : 0);       // [N][g_len][2] electron phase tables (use_tables)
    const size_t w = blockIdx.x;
    const int tid = threadIdx.x;
    const bool want_zv = drift != nullptr;
    int bad_in = 0;
    for (int idx = tid; idx < 3 * N; idx += 256) {
        const double xv = (double)x[w * 3 * N + idx], dv = want_zv ? (double)drift[w * 3 * N + idx] : 0.0;
        bad_in |= !isfinite(xv) || !isfinite(dv);
        xs[idx] = xv; ds_[idx] = dv;
    }
    for (int idx = tid; idx < 3 * A; idx += 256) frec[idx] = 0.0;
    for (int idx = tid; idx < 81; idx += 256) dsp[idx] = (double)S.disp27[idx];
    const int bad_walker = __syncthreads_or(bad_in);
    double* o_hf = out_hf ? out_hf + w * 3 * A : nullptr;
    double* o_zv = out_zv ? out_zv + w * 3 * A : nullptr;
    double* o_rw = rows ? rows + w * 6 * A : nullptr;
    if (bad_walker) {        // (uniform over the workgroup)
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int idx = tid; idx < 3 * A; idx += 256) {
            if (o_hf) o_hf[idx] = nan;
            if (o_zv) o_zv[idx] = nan;
            if (o_rw) { o_rw[idx] = nan; o_rw[3 * A + idx] = nan; }
        }
        if (tid == 0 && n_bad) atomicAdd(n_bad, 1ull);
        return;
    }
    // ---- 2. reciprocal space
    if (use_tables) {
        for (int idx = tid; idx < N * L; idx += 256) {
            const int i = idx / L, t = idx - i * L;
            double cs, sn;
            force_phase_entry(S, xs + 3 * i, t, &cs, &sn);
            tab[2 * idx] = cs; tab[2 * idx + 1] = sn;
        }
    }
    for (int g0 = 0; g0 < NG; g0 += FORCE_GC) {
        const int ng = min(FORCE_GC, NG - g0);
        __syncthreads();         // tables written; the previous chunk's readers of sg are done
        for (int k = tid; k < ng; k += 256) {
            const int g = g0 + k;
            double ss = 0, sc = 0;
            if (use_tables) {
                const int t0 = (int)S.gidx[3 * g], t1 = (int)S.gidx[3 * g + 1], t2 = (int)S.gidx[3 * g + 2];
                for (int i = 0; i < N; ++i) {
                    const double* ti = tab + 2 * (size_t)i * L;
                    const double ar = ti[2 * t0], ai = ti[2 * t0 + 1], br = ti[2 * t1], bi = ti[2 * t1 + 1], cr = ti[2 * t2],
                                 ci = ti[2 * t2 + 1];
                    const double pr = ar * br - ai * bi, pi = ar * bi + ai * br;
                    sc += pr * cr - pi * ci;
                    ss += pr * ci + pi * cr;
                }
            } else {
                const double q0 = (double)S.gpoints[3 * g], q1 = (double)S.gpoints[3 * g + 1], q2 = (double)S.gpoints[3 * g + 2];
                for (int i = 0; i < N; ++i) {
                    double sn, cs;
                    sincos(xs[3 * i] * q0 + xs[3 * i + 1] * q1 + xs[3 * i + 2] * q2, &sn, &cs);
                    ss += sn; sc += cs;
                }
            }
            sg[2 * k] = sc; sg[2 * k + 1] = ss;
        }
        for (int a = 0; a < A; ++a) {
            const double Ra[3] = {(double)S.sim_atoms[3 * a], (double)S.sim_atoms[3 * a + 1], (double)S.sim_atoms[3 * a + 2]};
            __syncthreads();     // sg written; the previous ion's readers of tabA and of red are done
            if (ion_table)
                for (int t = tid; t < L; t += 256) {
                    double cs, sn;
                    force_phase_entry(S, Ra, t, &cs, &sn);
                    tabA[2 * t] = cs; tabA[2 * t + 1] = sn;
                }
            __syncthreads();
            double f[3] = {0, 0, 0};
            for (int k = tid; k < ng; k += 256) {
                const int g = g0 + k;
                const double q0 = (double)S.gpoints[3 * g], q1 = (double)S.gpoints[3 * g + 1], q2 = (double)S.gpoints[3 * g + 2];
                double cs, sn;
                if (ion_table) {
                    const int t0 = (int)S.gidx[3 * g], t1 = (int)S.gidx[3 * g + 1], t2 = (int)S.gidx[3 * g + 2];
                    const double ar = tabA[2 * t0], ai = tabA[2 * t0 + 1], br = tabA[2 * t1], bi = tabA[2 * t1 + 1], cr = tabA[2 * t2],
                                 ci = tabA[2 * t2 + 1];
                    const double pr = ar * br - ai * bi, pi = ar * bi + ai * br;
                    cs = pr * cr - pi * ci;
                    sn = pr * ci + pi * cr;
                } else {
                    sincos(Ra[0] * q0 + Ra[1] * q1 + Ra[2] * q2, &sn, &cs);
                }
                const double m = (double)S.gweight[g] * (sn * sg[2 * k] - cs * sg[2 * k + 1]);
                f[0] += m * q0; f[1] += m * q1; f[2] += m * q2;
            }
            for (int c = 0; c < 3; ++c) red[256 * c + tid] = f[c];
            force_tree<3>(red, tid);
            if (tid < 3) frec[3 * a + tid] += -2.0 * (double)S.sim_charges[a] * red[256 * tid];
        }
    }
    // ---- 3. real space and the zero-variance terms, ion by ion
    const double alpha = (double)S.alpha, kg = 1.1283791670955125738961589031215 * alpha;     // 2 alpha / sqrt(pi)
    const double irc2 = 1.0 / (r_c * r_c);
    int bad_out = 0;             // thread 0..2 only
    for (int a = 0; a < A; ++a) {
        const double Z = (double)S.sim_charges[a];
        __syncthreads();         // frec complete; the previous ion's readers of vmi and red are done
        double hf[3] = {0, 0, 0}, zv[3] = {0, 0, 0};
        for (int i = tid; i < N; i += 256) {
            double d[3], mi[3];
            for (int c = 0; c < 3; ++c) d[c] = xs[3 * i + c] - (double)S.sim_atoms[3 * a + c];
            min_image(S, d, mi);         // (ds_kernels.h, in float64 on the handle's tables)
            for (int c = 0; c < 3; ++c) vmi[3 * i + c] = mi[c];
            if (!want_zv) continue;
            // The image of the ZV term is the true nearest one, u: the fractional wrap of d, then the nearest of the 27 around it
            // (r_c is below every plane spacing, so inside r_c nothing further away can be nearer).  mi itself is not u for the
            // wrapped images of a non-orthogonal cell (dist_mode 1: bcc), nor for a walker outside the cell in dist_mode 2.
            double w[3], fr[3], u[3] = {0, 0, 0};
            for (int c = 0; c < 3; ++c) {
                const double f = d[0] * (double)S.sim_ainv[c] + d[1] * (double)S.sim_ainv[3 + c] + d[2] * (double)S.sim_ainv[6 + c];
                fr[c] = f - rint(f);
            }
            for (int c = 0; c < 3; ++c) w[c] = fr[0] * (double)S.sim_a[c] + fr[1] * (double)S.sim_a[3 + c] + fr[2] * (double)S.sim_a[6 + c];
            // (inside the sphere inscribed in the wrap cell, radius r_in = half the smallest plane spacing, w is the nearest already)
            double best = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
            for (int c = 0; c < 3; ++c) u[c] = w[c];
#pragma unroll 1                 // (unrolled, the 81 table loads cost the kernel a wave per SIMD)
            for (int s = 0; s < 27 && !(best < r_in * r_in); ++s) {
                const double v0 = w[0] + dsp[3 * s], v1 = w[1] + dsp[3 * s + 1], v2 = w[2] + dsp[3 * s + 2];
                const double n2 = v0 * v0 + v1 * v1 + v2 * v2;
                if (n2 < best) { best = n2; u[0] = v0; u[1] = v1; u[2] = v2; }
            }
            int sn = -1;         // the HF image mi + D_s that u is (images differ by at least 2 r_ws >= 2 r_c); -1: no ZV term in the pair loop
            if (best < r_c * r_c) {
                {
                    const double e0 = mi[0] - u[0], e1 = mi[1] - u[1], e2 = mi[2] - u[2];
                    if (e0 * e0 + e1 * e1 + e2 * e2 < 0.25 * r_c * r_c) sn = 13;      // the usual case: u is mi itself
                }
#pragma unroll 1
                for (int s = 0; s < 27 && sn < 0; ++s) {
                    const double e0 = mi[0] + dsp[3 * s] - u[0], e1 = mi[1] + dsp[3 * s + 1] - u[1],
                                 e2 = mi[2] + dsp[3 * s + 2] - u[2];
                    if (e0 * e0 + e1 * e1 + e2 * e2 < 0.25 * r_c * r_c) sn = s;
                }
                if (sn < 0) {
                    // u is none of the 27 images of F^hf (a walker several cells away from the ion in dist_mode 2): F^hf has no
                    // singular term at u to cancel, dF is added as it stands
                    const double r2 = best, r = sqrt(r2), ir = 1.0 / r;
                    const double q = 1.0 - r2 * irc2, q2 = q * q, cq = q2 * q;
                    const double smooth = -9.0 * q2 * irc2 * ir + 12.0 * r * q * irc2 * irc2;
                    const double gp_r = 6.0 * q2 * irc2 * ir + cq * ir * ir * ir;
                    const double* dd = ds_ + 3 * i;
                    const double ud = u[0] * dd[0] + u[1] * dd[1] + u[2] * dd[2];
                    for (int c = 0; c < 3; ++c) zv[c] += Z * ((smooth - cq * ir * ir * ir - gp_r * ud) * u[c] + cq * ir * dd[c]);
                }
            }
            snear[i] = (double)sn;
        }
        __syncthreads();
        for (int it = tid; it < 27 * N; it += 256) {
            const int i = it / 27, s = it - 27 * i;
            const double v[3] = {vmi[3 * i] + dsp[3 * s], vmi[3 * i + 1] + dsp[3 * s + 1],
                                 vmi[3 * i + 2] + dsp[3 * s + 2]};
            const double r2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], r = sqrt(r2), ir = 1.0 / r;
            const double ar = alpha * r, ga = kg * exp(-ar * ar);
            const double h = Z * (erfc(ar) * ir * ir + ga * ir) * ir;
            for (int c = 0; c < 3; ++c) hf[c] += h * v[c];
            if (!want_zv) continue;
            if (s != (int)snear[i] || !(r < r_c)) {
                for (int c = 0; c < 3; ++c) zv[c] += h * v[c];
                continue;
            }
            // the pair's nearest image inside the cutoff: HF and ZV terms together, the Z c v / r^3 pieces cancelled analytically
            const double u = 1.0 - r2 * irc2, u2 = u * u, cu = u2 * u;
            const double one_m_c = r2 * irc2 * (1.0 + u + u2);
            const double comb = ((one_m_c - erf(ar)) * ir * ir + ga * ir) * ir;              // (erfc - c) / r^3 + ga / r^2
            const double smooth = -9.0 * u2 * irc2 * ir + 12.0 * r * u * irc2 * irc2;        // c'' / (2r) + c' / r^2
            const double gp_r = 6.0 * u2 * irc2 * ir + cu * ir * ir * ir;                    // (g' / r) / Z
            const double* d = ds_ + 3 * i;
            const double vd = v[0] * d[0] + v[1] * d[1] + v[2] * d[2];
            for (int c = 0; c < 3; ++c) zv[c] += Z * ((comb + smooth - gp_r * vd) * v[c] + cu * ir * d[c]);
        }
        for (int c = 0; c < 3; ++c) { red[256 * c + tid] = hf[c]; red[256 * (3 + c) + tid] = zv[c]; }
        force_tree<6>(red, tid);
        if (tid < 3) {
            const double fi = ion_ion ? ion_ion[3 * a + tid] : 0.0;
            const double fh = (red[256 * tid] + frec[3 * a + tid]) + fi;
            const double fz = (red[256 * (3 + tid)] + frec[3 * a + tid]) + fi;
            bad_out |= !isfinite(fh) || (want_zv && !isfinite(fz));
            if (o_hf) o_hf[3 * a + tid] = fh;
            if (o_zv) o_zv[3 * a + tid] = fz;
            if (o_rw) { o_rw[3 * a + tid] = fh; o_rw[3 * A + 3 * a + tid] = fz; }
        }
    }
    // a non-finite result (an electron on a nucleus): the whole walker is bad
    if (__syncthreads_or(bad_out)) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int idx = tid; idx < 3 * A; idx += 256) {
            if (o_hf) o_hf[idx] = nan;
            if (o_zv) o_zv[idx] = nan;
            if (o_rw) { o_rw[idx] = nan; o_rw[3 * A + idx] = nan; }
        }
        if (tid == 0 && n_bad) atomicAdd(n_bad, 1ull);
    }
}

// rows: [nw][2][A][3] of one pass (a bad walker's are all NaN: the first entry is tested); part: [groups][12 A + 1], per (a, c)
// (sum F^hf, sum (F^hf)^2, sum F^zv, sum (F^zv)^2) and, last, the number of good walkers of the group
__global__ void __launch_bounds__(FORCE_GROUP) k_force_part(const double* __restrict__ rows, long long nw, int A,
                                                             double* __restrict__ part) {
    __shared__ double sh[4 * FORCE_GROUP];
    const int tid = threadIdx.x;
    const long long wl = (long long)blockIdx.x * FORCE_GROUP + tid;
    const double* rw = rows + wl * 6 * A;
    const bool good = wl < nw && !isnan(rw[0]);
    double* pg = part + (size_t)blockIdx.x * (12 * A + 1);
    for (int j = 0; j < 3 * A; ++j) {
        const double fh = good ? rw[j] : 0.0, fz = good ? rw[3 * A + j] : 0.0;
        __syncthreads();                               // the previous column's readers are done
        sh[tid] = fh; sh[FORCE_GROUP + tid] = fh * fh; sh[2 * FORCE_GROUP + tid] = fz; sh[3 * FORCE_GROUP + tid] = fz * fz;
        force_tree<4>(sh, tid);
        if (tid < 4) pg[4 * j + tid] = sh[FORCE_GROUP * tid];
    }
    __syncthreads();
    sh[tid] = good ? 1.0 : 0.0;
    force_tree<1>(sh, tid);
    if (tid == 0) pg[12 * A] = sh[0];
}

// sums[j] += the rows of part in group order (thread j, any number of workgroups)
__global__ void __launch_bounds__(256) k_force_final(const double* __restrict__ part, long long n_groups, int K, double* __restrict__ sums) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    double s = sums[j];
    for (long long g = 0; g < n_groups; ++g) s += part[g * K + j];
    sums[j] = s;
}

}  // namespace ds
