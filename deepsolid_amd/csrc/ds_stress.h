// ds_stress.h -- strain derivative of the energy of a batch of walkers: the kinetic tensor from the walker gradient and the
// derivative of the Ewald sums of k_ewald with respect to a homogeneous strain of the cell.  The reference
// has no stress estimator: the conventions are this library's own.
//
// Strain eps (symmetric 3 x 3): every electron and ion position and every lattice vector goes v -> v (1 + eps), every reciprocal
// vector G -> G (1 + eps)^-1, the volume V -> V (1 + tr eps).  Held fixed: alpha, the integer list of G points that passed the weight
// cut-off, and the minimal-image choice of every pair (a function of fractional coordinates, which the strain leaves alone).  Per
// walker, as symmetric tensors in the component order xx, yy, zz, yz, xz, xy:
//   kin_ab = - sum_i (Re d_ia Re d_ib + Im d_ia Im d_ib),   d = grad log psi (ds_logpsi_grad)     (= -2 K_ab, <tr K> = <T>)
//   real space, pairs i < j (charge product 1) and (electron, ion a) (charge product -Z_a), 27 displacements each, v = mi + D_s:
//       q f'(r) v_a v_b / r,   f'(r) = -[erfc(alpha r) / r^2 + (2 alpha / sqrt pi) exp(-alpha^2 r^2) / r]
//   reciprocal space: the phases G.r do not change, only w_G = 4 pi exp(-G^2 / 4 alpha^2) / (V G^2) does:
//       dw_ab = w_G [-delta_ab + 2 G_a G_b (1 / G^2 + 1 / (4 alpha^2))]
//       ee: sum_G dw_ab (S_c^2 + S_s^2),   ei: 2 sum_G dw_ab (-Re S_ion S_c - Im S_ion S_s)
//   constants: d(ijconst) / d eps_ab = -ijconst delta_ab, ijconst = -pi / (V alpha^2); the -alpha / sqrt pi of squareconst has none:
//       ee: -(N^2 / 2) ijconst delta_ab,   ei: +N (sum_a Z_a) ijconst delta_ab
//   ion-ion: a constant of the geometry, the caller's array (ewaldsum.ion_ion_stress)
// The outputs are dE / d eps in Hartree; the stress is their sum over V.  All arithmetic is float64 for either handle dtype; the
// handle's tables (T), x and the gradient (T) are converted on load.
//
//   k_stress       one workgroup of 256 threads per walker:
//                    1. x and the gradient to LDS; a non-finite entry makes the walker bad
//                    2. per chunk of FORCE_GC G points: S_c, S_s of the chunk to LDS (phase tables when S.g_len > 0 and they fit,
//                       direct sincos otherwise), then thread t adds its G points t, t + 256, ... of the chunk, in order, into its
//                       twelve sums (ee and ei x 6); the six factors of dw_G come from gpoints, gweight and alpha on the fly
//                    3. real space in the thread-strided order of k_ewald: (electron, ion) items, then pairs i < j, 27 images each,
//                       the minimal image from k_ewald's own min_image (ds_kernels.h) in float64
//                    4. the LDS tree (t += t + s, s = 128 .. 1) over the twelve sums; then the kinetic tensor, thread t taking
//                       electrons t, t + 256, ..., through the same tree
//                    5. thread c < 6 adds the constants and writes kin, ee, ei and total = ((kin + ee) + ei) + ii
//                  nothing of size N or A lives in registers.  A bad walker (non-finite input, or a non-finite result) gets NaN in
//                  every output and is counted.
//   k_stress_part  one workgroup per FORCE_GROUP walkers of a pass: per entry of the 4 x 6 rows the sum and the sum of squares over the
//                  group's good walkers through the LDS tree of ds_force.h (thread t = walker t of the group), and their number
//   k_force_final  (ds_force.h) adds the groups in order onto `sums`
// The order of every addition is a function of (N, A, NG, B) alone and groups are cut at multiples of FORCE_GROUP walkers of the
// batch, so the results are bit-identical from run to run and for any workspace size.  No floating-point atomics.
//
// LDS: 9 N + 12 x 256 + 81 + 2 FORCE_GC doubles = 49.6 KB at N = 128, plus the electrons' phase tables (2 N g_len doubles) when the
// whole stays within FORCE_LDS_MAX = 64 KB (the rule of force_table_flags; the structure factors take the direct sincos path
// otherwise).  The layout without tables is below the cap for every N the handle accepts (N <= 128).
#pragma once
#include <hip/hip_runtime.h>

#include "ds_force.h"

namespace ds {

constexpr int STRESS_ROWS = 4;          // kin, ee, ei, total
constexpr int STRESS_K = 2 * STRESS_ROWS * 6 + 1;       // entries of `sums`

// doubles of dynamic LDS of k_stress, with or without the electrons' phase tables
template <typename T> inline size_t stress_lds_doubles(const SysDev<T>& S, bool tables) {
    return (size_t)9 * S.N + 12 * 256 + 81 + 2 * (size_t)FORCE_GC + (tables ? 2 * (size_t)S.N * S.g_len : 0);
}
// FORCE_EL_TABLES when the tables exist and fit into FORCE_LDS_MAX, 0 when they do not; -1: not even the layout without tables fits
template <typename T> inline int stress_table_flags(const SysDev<T>& S) {
    if (S.g_len > 0 && stress_lds_doubles(S, true) * sizeof(double) <= FORCE_LDS_MAX) return FORCE_EL_TABLES;
    return stress_lds_doubles(S, false) * sizeof(double) <= FORCE_LDS_MAX ? 0 : -1;
}

// acc[0..5] += m (p0 p0, p1 p1, p2 p2, p1 p2, p0 p2, p0 p1)
__device__ __forceinline__ void stress_add_outer(double* acc, double m, double p0, double p1, double p2) {
    acc[0] += m * p0 * p0; acc[1] += m * p1 * p1; acc[2] += m * p2 * p2;
    acc[3] += m * p1 * p2; acc[4] += m * p0 * p2; acc[5] += m * p0 * p1;
}

// out (optional): [walker of the batch][4][6]; rows (optional): the same of the launch, what k_stress_part reads
template <typename T>
__global__ void __launch_bounds__(256) k_stress(SysDev<T> S, const T* __restrict__ x, const T* __restrict__ grad,
                                                const double* __restrict__ ion_ion, int tables, double* __restrict__ out,
                                                double* __restrict__ rows, unsigned long long* __restrict__ n_bad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = S.N, A = S.As, L = S.g_len, NG = S.NG;
    double* xs = reinterpret_cast<double*>(smem_raw);   // [N][3]
    double* gs = xs + 3 * N;                            // [N][3][2] gradient (Re, Im)
    double* red = gs + 6 * N;                           // [12][256]
    double* dsp = red + 12 * 256;                       // [27][3] the lattice displacements D_s
    double* sg = dsp + 81;                              // [FORCE_GC][2] = (S_c, S_s) of the chunk
    double* tab = sg + 2 * FORCE_GC;                    // [N][g_len][2] electron phase tables (use_tables)
    const bool use_tables = tables & FORCE_EL_TABLES;
    const size_t w = blockIdx.x;
    const int tid = threadIdx.x;
    const bool want_kin = grad != nullptr;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* o_w = out ? out + w * 6 * STRESS_ROWS : nullptr;
    double* o_r = rows ? rows + w * 6 * STRESS_ROWS : nullptr;
    int bad_in = 0;
    for (int idx = tid; idx < 3 * N; idx += 256) {
        const double xv = (double)x[w * 3 * N + idx];
        bad_in |= !isfinite(xv);
        xs[idx] = xv;
    }
    for (int idx = tid; idx < 6 * N; idx += 256) {
        const double gv = want_kin ? (double)grad[w * 6 * N + idx] : 0.0;
        bad_in |= !isfinite(gv);
        gs[idx] = gv;
    }
    for (int idx = tid; idx < 81; idx += 256) dsp[idx] = (double)S.disp27[idx];
    if (__syncthreads_or(bad_in)) {        // (uniform over the workgroup)
        if (tid < 6 * STRESS_ROWS) {
            if (o_w) o_w[tid] = nan;
            if (o_r) o_r[tid] = nan;
        }
        if (tid == 0 && n_bad) atomicAdd(n_bad, 1ull);
        return;
    }
    const double alpha = (double)S.alpha, kg = 1.1283791670955125738961589031215 * alpha;     // 2 alpha / sqrt(pi)
    const double i4a2 = 0.25 / (alpha * alpha);
    double acc[12];              // [0..5] ee, [6..11] ei
    for (int c = 0; c < 12; ++c) acc[c] = 0.0;
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
        __syncthreads();
        // (FORCE_GC is a multiple of 256: over the chunks thread t takes g = t, t + 256, ... of all G points in order)
        for (int k = tid; k < ng; k += 256) {
            const int g = g0 + k;
            const double q0 = (double)S.gpoints[3 * g], q1 = (double)S.gpoints[3 * g + 1], q2 = (double)S.gpoints[3 * g + 2];
            const double wg = (double)S.gweight[g];
            const double sc = sg[2 * k], ss = sg[2 * k + 1];
            const double m_ee = wg * (sc * sc + ss * ss);
            const double m_ei = 2.0 * wg * (-(double)S.ion_re[g] * sc - (double)S.ion_im[g] * ss);
            const double f = 2.0 * (1.0 / (q0 * q0 + q1 * q1 + q2 * q2) + i4a2);
            // dw_ab = w (-delta_ab + f G_a G_b)
            for (int c = 0; c < 3; ++c) { acc[c] -= m_ee; acc[6 + c] -= m_ei; }
            stress_add_outer(acc, m_ee * f, q0, q1, q2);
            stress_add_outer(acc + 6, m_ei * f, q0, q1, q2);
        }
    }
    // ---- 3. real space: (electron, ion) items then pairs i < j, 27 images each, in the order of k_ewald
    const int n_ei = N * A, n_ee = N * (N - 1) / 2;
    for (int it = tid; it < n_ei + n_ee; it += 256) {
        double d[3], mi[3], q;
        const bool is_ei = it < n_ei;
        if (is_ei) {
            const int i = it / A, a = it - i * A;
            for (int c = 0; c < 3; ++c) d[c] = xs[3 * i + c] - (double)S.sim_atoms[3 * a + c];
            q = -(double)S.sim_charges[a];
        } else {
            int r = it - n_ei, i = 0;
            while (r >= N - 1 - i) { r -= N - 1 - i; ++i; }
            const int j = i + 1 + r;
            for (int c = 0; c < 3; ++c) d[c] = xs[3 * i + c] - xs[3 * j + c];
            q = 1.0;
        }
        min_image(S, d, mi);
        double p[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
        for (int s = 0; s < 27; ++s) {
            const double v0 = mi[0] + dsp[3 * s], v1 = mi[1] + dsp[3 * s + 1], v2 = mi[2] + dsp[3 * s + 2];
            const double r2 = v0 * v0 + v1 * v1 + v2 * v2, r = sqrt(r2), ir = 1.0 / r;
            const double ar = alpha * r;
            // f'(r) / r
            const double h = -(erfc(ar) * ir * ir + kg * exp(-ar * ar) * ir) * ir;
            stress_add_outer(p, h, v0, v1, v2);
        }
        // (a select, not a pointer into acc: the sums stay in registers)
        for (int c = 0; c < 6; ++c) {
            const double v = q * p[c];
            if (is_ei) acc[6 + c] += v; else acc[c] += v;
        }
    }
    // ---- 4. the trees
    __syncthreads();
    for (int c = 0; c < 12; ++c) red[256 * c + tid] = acc[c];
    force_tree<12>(red, tid);
    double mine_ee = 0, mine_ei = 0;      // thread c < 6: component c
    if (tid < 6) { mine_ee = red[256 * tid]; mine_ei = red[256 * (6 + tid)]; }
    __syncthreads();
    double kin[6] = {0, 0, 0, 0, 0, 0};
    if (want_kin)
        for (int i = tid; i < N; i += 256) {
            const double* gi = gs + 6 * i;
            stress_add_outer(kin, -1.0, gi[0], gi[2], gi[4]);
            stress_add_outer(kin, -1.0, gi[1], gi[3], gi[5]);
        }
    for (int c = 0; c < 6; ++c) red[256 * c + tid] = kin[c];
    force_tree<6>(red, tid);
    // ---- 5. constants and output
    int bad_out = 0;
    double r_kin = 0, r_ee = 0, r_ei = 0, r_tot = 0;
    if (tid < 6) {
        double vol = 0, zsum = 0;
        {
            const double a0 = (double)S.sim_a[0], a1 = (double)S.sim_a[1], a2 = (double)S.sim_a[2], b0 = (double)S.sim_a[3],
                         b1 = (double)S.sim_a[4], b2 = (double)S.sim_a[5], c0 = (double)S.sim_a[6], c1 = (double)S.sim_a[7],
                         c2 = (double)S.sim_a[8];
            vol = a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
        }
        for (int a = 0; a < A; ++a) zsum += (double)S.sim_charges[a];
        const double ijconst = -3.14159265358979323846264338327950288 / (vol * alpha * alpha);
        const double diag = tid < 3 ? 1.0 : 0.0;
        r_kin = red[256 * tid];
        r_ee = mine_ee - diag * (0.5 * (double)N * (double)N * ijconst);
        r_ei = mine_ei + diag * ((double)N * zsum * ijconst);
        r_tot = ((r_kin + r_ee) + r_ei) + (ion_ion ? ion_ion[tid] : 0.0);
        bad_out = !isfinite(r_tot);
    }
    // a non-finite result (two electrons, or an electron and a nucleus, at one point): the whole walker is bad
    const int bad = __syncthreads_or(bad_out);
    if (tid < 6) {
        if (bad) r_kin = r_ee = r_ei = r_tot = nan;
        if (o_w) { o_w[tid] = r_kin; o_w[6 + tid] = r_ee; o_w[12 + tid] = r_ei; o_w[18 + tid] = r_tot; }
        if (o_r) { o_r[tid] = r_kin; o_r[6 + tid] = r_ee; o_r[12 + tid] = r_ei; o_r[18 + tid] = r_tot; }
    }
    if (bad && tid == 0 && n_bad) atomicAdd(n_bad, 1ull);
}

// rows: [nw][4][6] of one pass (a bad walker's are all NaN: the last row's first entry is tested); part: [groups][STRESS_K], per
// entry j of the 24 (sum, sum of squares) at 2 j and, last, the number of good walkers of the group
__global__ void __launch_bounds__(FORCE_GROUP) k_stress_part(const double* __restrict__ rows, long long nw, double* __restrict__ part) {
    __shared__ double sh[2 * FORCE_GROUP];
    const int tid = threadIdx.x;
    const long long wl = (long long)blockIdx.x * FORCE_GROUP + tid;
    const double* rw = rows + wl * 6 * STRESS_ROWS;
    const bool good = wl < nw && !isnan(rw[18]);
    double* pg = part + (size_t)blockIdx.x * STRESS_K;
    for (int j = 0; j < 6 * STRESS_ROWS; ++j) {
        const double v = good ? rw[j] : 0.0;
        __syncthreads();                               // the previous entry's readers are done
        sh[tid] = v; sh[FORCE_GROUP + tid] = v * v;
        force_tree<2>(sh, tid);
        if (tid < 2) pg[2 * j + tid] = sh[FORCE_GROUP * tid];
    }
    __syncthreads();
    sh[tid] = good ? 1.0 : 0.0;
    force_tree<1>(sh, tid);
    if (tid == 0) pg[STRESS_K - 1] = sh[0];
}

}  // namespace ds
