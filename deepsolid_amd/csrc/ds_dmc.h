// ds_dmc.h -- fixed-phase diffusion Monte Carlo: the fused drift-diffusion step and the fixed-population comb.
//
// The reference has no DMC: the conventions are this project's own (include/deepsolid_hip.h states the
// algorithm word for word).  Per step:
//   k_dmc_propose      one thread per electron: limited drift, noise (Philox streams 0 / 1 of ds_mcmc.h or replayed), wrap
//   (energy chain at x' with both outputs, k_ewald)
//   k_dmc_accept       one wave per walker: the two squared norms, the decision, the weight, the selected rows, (p, flags)
//   k_dmc_stats        one workgroup per DMC_GROUP consecutive walkers: one row of float64 partials
//   k_dmc_stats_final  adds the rows in workgroup order: one row of out_stats
// and on a branching step the comb (k_dmc_scan_chunks, k_dmc_scan_offsets, k_dmc_select, k_dmc_gather, k_dmc_copy_back).
// With a pseudopotential (ds_dmc_step_ecp, locality approximation) ds_ecp_energy's launches follow the chain pass at x', the ECP
// instances of k_dmc_init / k_dmc_accept take its float64 triple, k_dmc_col_stats<3> / k_dmc_col_stats_final<3> form the row of
// out_ecp_stats, and k_dmc_gather_epp follows the comb.  With T-moves (ds_dmc_step_tmove) the pseudopotential is evaluated after
// the decision: the kernels at the end of this file.  All three steps take the decision of dmc_decide and set a walker's chain
// scalars with dmc_set_walker; every stats row goes through the one LDS tree of dmc_group_tree.
//
// Prefix sums of the weights, the order the numpy model reproduces bit for bit (DMC_CHUNK = 256):
//   chunk c holds walkers 256 c .. 256 c + 255;  r_0 = w_first, r_i = r_{i-1} + w_i  (sequential inside the chunk);
//   O_0 = 0, O_c = O_{c-1} + r_last(c-1)  (chunk offsets, sequential);  C_j = O_c + r_i;  W = C_{B-1}.
// Every sum is one rounded float64 addition; with weights >= 0 the C_j do not decrease.  No floating-point atomics anywhere.
#pragma once
#include "ds_mcmc.h"

namespace ds {

constexpr int DMC_CHUNK = 256;                         // walkers per scan chunk
constexpr long long DMC_MAX_B = 256ll * 4096;          // the chunk offsets of one call fit one workgroup's LDS: B <= 2^20
constexpr int DMC_GROUP = 256;                         // walkers per row of stats partials
constexpr int DMC_ROW = 9;                             // doubles of one out_stats row
constexpr int DMC_WAVES = 4;                           // walkers per workgroup of the per-walker kernels
// flags of one walker and step
constexpr int DMC_ACCEPTED = 1, DMC_CLIPPED = 2, DMC_NONFINITE = 4, DMC_NODE = 8;

struct DmcArgs {
    double tau, sqrt_tau, tau_eff, e_trial, e_ref, e_cut;
    int node_mode, N;
    long long B;
};

// Umrigar-Nightingale-Runge limiter with a = 1 in the form without cancellation: vbar = v * 2 / (1 + sqrt(1 + 2 |v|^2 tau))
template <typename T> __device__ __forceinline__ T dmc_limiter(const T v[3], T tau) {
    const T v2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    return T(2) / (T(1) + ds_sqrt(T(1) + T(2) * v2 * tau));
}

// sum of the Ewald triple as k_sum3 forms it, then E = Re ke + ewald in float64
template <typename T> __device__ __forceinline__ double dmc_energy(const T* __restrict__ ke, const T* __restrict__ ew3, long long w) {
    const T ew = ew3[3 * w] + ew3[3 * w + 1] + ew3[3 * w + 2];
    return (double)ke[2 * w] + (double)ew;
}

__device__ __forceinline__ double dmc_clip(double e, double e_ref, double e_cut, bool* clipped) {
    *clipped = false;
    if (!(e_cut > 0.0)) return e;
    const double d = e - e_ref;
    if (d > e_cut) { *clipped = true; return e_ref + e_cut; }
    if (d < -e_cut) { *clipped = true; return e_ref - e_cut; }
    return e;
}

// x2 = wrap(x + tau vbar + sqrt(tau) chi); chi is written to `noise_out` in Philox mode so that k_dmc_accept reads what was used
template <typename T>
__global__ void __launch_bounds__(256) k_dmc_propose(const T* __restrict__ a, const T* __restrict__ ainv, const T* __restrict__ x,
                                                     const T* __restrict__ drift, const T* __restrict__ normal, PhiloxKey key,
                                                     unsigned long long step, T tau, T sqrt_tau, size_t n_elec, T* __restrict__ x2,
                                                     T* __restrict__ noise_out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elec) return;
    T v[3], chi[3], r[3], o[3], wr[3];
    for (int c = 0; c < 3; ++c) v[c] = drift[3 * e + c];
    if (normal) {
        for (int c = 0; c < 3; ++c) chi[c] = normal[3 * e + c];
    } else {
        double z[3];
        philox_normal3(key, step, e, z);
        for (int c = 0; c < 3; ++c) { chi[c] = (T)z[c]; noise_out[3 * e + c] = chi[c]; }
    }
    const T f = dmc_limiter(v, tau);
    for (int c = 0; c < 3; ++c) r[c] = x[3 * e + c] + tau * (f * v[c]) + sqrt_tau * chi[c];
    wrap_point(r, a, ainv, o, wr);
    for (int c = 0; c < 3; ++c) x2[3 * e + c] = o[c];
}

// E = ((Re ke + ewald) + E_loc) + Re E_nl with the pseudopotential triple (E_loc, Re E_nl, Im E_nl) of ds_ecp_energy: float64, one
// rounded addition each, in this order (the locality approximation: ds_dmc_step_ecp)
__device__ __forceinline__ double dmc_energy_ecp(double e, const double* __restrict__ epp, long long w) {
#pragma clang fp contract(off)
    return (e + epp[3 * w]) + epp[3 * w + 1];
}

// One wave on walker w after a chain pass (gc, ke, ew3, la: its outputs): drift = Re grad, eloc = Re ke + ewald (ECP: with the triple
// epp2); a walker whose log|psi| or E_L is not finite gets weight 0
template <typename T, bool ECP>
__device__ __forceinline__ void dmc_set_walker(long long w, int lane, int n3, const T* __restrict__ gc, const T* __restrict__ ke,
                                               const T* __restrict__ ew3, const T* __restrict__ la, const double* __restrict__ epp2,
                                               T* __restrict__ drift, double* __restrict__ eloc, double* __restrict__ weight) {
    for (int c = lane; c < n3; c += 64) drift[(size_t)w * n3 + c] = gc[2 * ((size_t)w * n3 + c)];
    if (lane == 0) {
        double e = dmc_energy(ke, ew3, w);
        if constexpr (ECP) e = dmc_energy_ecp(e, epp2, w);
        eloc[w] = e;
        if (!isfinite(e) || !isfinite((double)la[w])) weight[w] = 0.0;
    }
}

// state_valid = 0: dmc_set_walker on the chain pass at x.  ECP: the triple epp2 enters E_L and becomes the walker's epp
template <typename T, bool ECP>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_init(long long B, int n3, const T* __restrict__ gc, const T* __restrict__ ke,
                                                             const T* __restrict__ ew3, const T* __restrict__ logabs,
                                                             T* __restrict__ drift, double* __restrict__ eloc, double* __restrict__ weight,
                                                             const double* __restrict__ epp2, double* __restrict__ epp) {
    const long long w = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= B) return;
    dmc_set_walker<T, ECP>(w, lane, n3, gc, ke, ew3, logabs, epp2, drift, eloc, weight);
    if constexpr (ECP)
        if (lane == 0)
            for (int c = 0; c < 3; ++c) epp[3 * w + c] = epp2[3 * w + c];
}

// The decision of one wave on walker w, the same in the three steps.  Lanes stride the electrons for |chi|^2 and
// |chi + sqrt(tau) (vbar + vbar')|^2 (float64 sums; the butterfly adds them in a fixed order); every lane then holds the same
// decision.  e_prop_of() is the caller's energy at x', whose finiteness the decision asks for: the chain part, to which the locality
// step adds the triple.  It is a callable so that it is evaluated behind the wave sums, where both kernels had it: evaluated in
// front of them, k_dmc_tm_decide<double> takes 66 VGPRs instead of 58 and loses a wave of occupancy.
// flags: DMC_ACCEPTED, DMC_NONFINITE, DMC_NODE (the caller adds DMC_CLIPPED); pacc(): min(1, exp A), 0 for a refused proposal.
struct DmcDecision {
    double a_log, e_prop;
    bool open, acc;                                    // open: the proposal is finite and on the allowed side of the node
    int flags;
    __device__ __forceinline__ double pacc() const { return open ? (a_log < 0.0 ? exp(a_log) : 1.0) : 0.0; }
};
template <typename T, typename F>
__device__ __forceinline__ DmcDecision dmc_decide(const DmcArgs& A, long long w, int lane, const T* __restrict__ logabs,
                                                  const T* __restrict__ phase, const T* __restrict__ drift, const T* __restrict__ la2,
                                                  const T* __restrict__ ph2, const T* __restrict__ gc2, const T* __restrict__ chi,
                                                  const T* __restrict__ uniform, PhiloxKey key, unsigned long long step, const F& e_prop_of) {
    const size_t row = (size_t)w * 3 * A.N;
    double s1 = 0.0, s2 = 0.0;
    for (int e = lane; e < A.N; e += 64) {
        const size_t o = row + 3 * e;
        const T g1[3] = {drift[o], drift[o + 1], drift[o + 2]}, g2[3] = {gc2[2 * o], gc2[2 * (o + 1)], gc2[2 * (o + 2)]};
        const T f1 = dmc_limiter(g1, (T)A.tau), f2 = dmc_limiter(g2, (T)A.tau);
        for (int c = 0; c < 3; ++c) {
            const double ch = (double)chi[o + c];
            const double bk = ch + A.sqrt_tau * ((double)(f1 * g1[c]) + (double)(f2 * g2[c]));
            s1 += ch * ch; s2 += bk * bk;
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    const double la_new = (double)la2[w], la_old = (double)logabs[w];
    const double a_log = 2.0 * (la_new - la_old) + 0.5 * (s1 - s2);
    const double e_prop = e_prop_of();
    const double u = uniform ? (double)uniform[w] : philox_uniform(key, step, (unsigned long long)w);
    const bool finite = isfinite(a_log) && isfinite(e_prop);
    const double overlap = (double)ph2[2 * w] * (double)phase[2 * w] + (double)ph2[2 * w + 1] * (double)phase[2 * w + 1];
    const bool node_ok = A.node_mode == 0 || overlap > 0.0;
    const bool acc = finite && node_ok && a_log > log(u);
    int fl = 0;
    if (acc) fl |= DMC_ACCEPTED;
    if (!finite) fl |= DMC_NONFINITE;
    else if (!node_ok) fl |= DMC_NODE;
    return DmcDecision{a_log, e_prop, finite && node_ok, acc, fl};
}

// One wave per walker: the decision, then lane 0 updates the scalars and the wave copies the rows.
// ECP: the triple epp2 at x' enters E' and is selected into epp with the other rows; epp2 then holds the walker's selected triple
// too (the source of the comb's gather, k_dmc_gather_epp).
template <typename T, bool ECP>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_accept(DmcArgs A, T* __restrict__ x, T* __restrict__ logabs, T* __restrict__ phase,
                                                               T* __restrict__ drift, double* __restrict__ eloc,
                                                               double* __restrict__ weight, const T* __restrict__ x2,
                                                               const T* __restrict__ la2, const T* __restrict__ ph2,
                                                               const T* __restrict__ gc2, const T* __restrict__ ke2,
                                                               const T* __restrict__ ew2, const T* __restrict__ chi,
                                                               const T* __restrict__ uniform, PhiloxKey key, unsigned long long step,
                                                               double* __restrict__ pacc, int* __restrict__ flags,
                                                               double* __restrict__ epp2, double* __restrict__ epp) {
    const long long w = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= A.B) return;
    const int n3 = 3 * A.N;
    const size_t row = (size_t)w * n3;
    const DmcDecision d = dmc_decide(A, w, lane, logabs, phase, drift, la2, ph2, gc2, chi, uniform, key, step, [&] {
        const double e = dmc_energy(ke2, ew2, w);
        if constexpr (ECP) return dmc_energy_ecp(e, epp2, w);
        else return e;
    });
    const bool acc = d.acc;
    const double e_prop = d.e_prop;
    int fl = d.flags;
    const double e_old = eloc[w];
    const double e_new = acc ? e_prop : e_old;
    bool c_new, c_old;
    const double cn = dmc_clip(e_new, A.e_ref, A.e_cut, &c_new), co = dmc_clip(e_old, A.e_ref, A.e_cut, &c_old);
    if (c_new) fl |= DMC_CLIPPED;
    if (acc) {
        for (int c = lane; c < n3; c += 64) { x[row + c] = x2[row + c]; drift[row + c] = gc2[2 * (row + c)]; }
    }
    if (lane == 0) {
        double factor;
        {
#pragma clang fp contract(off)
            factor = exp(-A.tau_eff * (0.5 * (cn + co) - A.e_trial));
        }
        const double wn = weight[w] * factor;
        weight[w] = isfinite(wn) ? wn : 0.0;              // an energy that is not finite kills the walker
        if (acc) { logabs[w] = la2[w]; phase[2 * w] = ph2[2 * w]; phase[2 * w + 1] = ph2[2 * w + 1]; eloc[w] = e_prop; }
        pacc[w] = d.pacc();
        flags[w] = fl;
        if constexpr (ECP) {
            for (int c = 0; c < 3; ++c) {
                if (acc) epp[3 * w + c] = epp2[3 * w + c];
                else epp2[3 * w + c] = epp[3 * w + c];
            }
        }
    }
}

// The column sums of one workgroup of DMC_GROUP threads in LDS: thread t brings v[0..NC), the tree adds t and t + s, and row
// blockIdx.x of `part` takes the NC sums.  Every stats row of this file is formed here, so its order of additions is one.
template <int NC> __device__ __forceinline__ void dmc_group_tree(const double (&v)[NC], double* __restrict__ part) {
    __shared__ double sh[NC][DMC_GROUP];
    for (int j = 0; j < NC; ++j) sh[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int s = DMC_GROUP / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int j = 0; j < NC; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < NC) part[(long long)blockIdx.x * NC + threadIdx.x] = sh[threadIdx.x][0];
}

// out_ecp_stats: one row of partials per DMC_GROUP walkers, [sum w E_loc, sum w Re E_nl, sum w Im E_nl] over the walkers of non-zero
// weight (thread t takes walker g0 + t).  NC = 3: ds_dmc_step_ecp, choice is not read.  NC = 4: ds_dmc_step_tmove, the fourth
// column is the number of walkers that made a T-move (choice >= 0; an exact count) ...
template <int NC>
__global__ void __launch_bounds__(DMC_GROUP) k_dmc_col_stats(long long B, const double* __restrict__ weight, const double* __restrict__ epp,
                                                             const int* __restrict__ choice, double* __restrict__ part) {
    const long long w = (long long)blockIdx.x * DMC_GROUP + threadIdx.x;
    double v[NC] = {};
    if (w < B) {
        const double wt = weight[w];
        if (wt != 0.0)
            for (int j = 0; j < 3; ++j) v[j] = wt * epp[3 * w + j];
        if constexpr (NC > 3) v[3] = choice[w] >= 0 ? 1.0 : 0.0;
    }
    dmc_group_tree<NC>(v, part);
}

// ... and the rows added in workgroup order: one row of out_ecp_stats
template <int NC>
__global__ void __launch_bounds__(64) k_dmc_col_stats_final(const double* __restrict__ part, long long n_groups, double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= NC) return;
    double s = 0.0;
    for (long long g = 0; g < n_groups; ++g) s += part[g * NC + j];
    out[j] = s;
}

// after the comb: epp of walker k = the triple of its parent.  Reads the comb's parents and its run flag (tot[2]); the source is
// epp2, which k_dmc_accept left equal to epp, so no walker reads a row that another one writes.  A skipped comb changes nothing.
__global__ void __launch_bounds__(256) k_dmc_gather_epp(long long B, const double* __restrict__ tot, const int* __restrict__ parent,
                                                        const double* __restrict__ epp2, double* __restrict__ epp) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B || tot[2] == 0.0) return;
    const long long p = parent[k];
    for (int c = 0; c < 3; ++c) epp[3 * k + c] = epp2[3 * p + c];
}

// One row of partials per DMC_GROUP walkers: [sum w, sum w E, sum w E^2, accepted, sum p, clipped, non-finite, sum w^2]; a walker of
// weight 0 adds nothing to the energy sums (its energy may be NaN).  Thread t takes walker g0 + t; the tree adds t and t + s.
__global__ void __launch_bounds__(DMC_GROUP) k_dmc_stats(long long B, const double* __restrict__ weight, const double* __restrict__ eloc,
                                                         const double* __restrict__ pacc, const int* __restrict__ flags,
                                                         double* __restrict__ part) {
    const long long w = (long long)blockIdx.x * DMC_GROUP + threadIdx.x;
    double v[DMC_ROW - 1] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (w < B) {
        const double wt = weight[w], e = eloc[w];
        const int fl = flags[w];
        v[0] = wt; v[7] = wt * wt;
        if (wt != 0.0) { v[1] = wt * e; v[2] = wt * e * e; }
        v[3] = (fl & DMC_ACCEPTED) ? 1.0 : 0.0; v[4] = pacc[w];
        v[5] = (fl & DMC_CLIPPED) ? 1.0 : 0.0; v[6] = (fl & DMC_NONFINITE) ? 1.0 : 0.0;
    }
    dmc_group_tree<DMC_ROW - 1>(v, part);
}

// out[j] = the rows added in workgroup order; out[8] = B (a comb that follows overwrites it)
__global__ void __launch_bounds__(64) k_dmc_stats_final(const double* __restrict__ part, long long n_groups, long long B,
                                                        double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j < DMC_ROW - 1) {
        double s = 0.0;
#pragma unroll 8
        for (long long g = 0; g < n_groups; ++g) s += part[g * (DMC_ROW - 1) + j];
        out[j] = s;
    } else if (j == DMC_ROW - 1) {
        out[j] = (double)B;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the comb
// r (B,): running sums inside each chunk.  One wave per chunk: coalesced load into LDS, lane 0 adds in walker order.
__global__ void __launch_bounds__(64) k_dmc_scan_chunks(long long B, const double* __restrict__ weight, double* __restrict__ r,
                                                        double* __restrict__ chunk_sum) {
    __shared__ double sh[DMC_CHUNK];
    const long long c0 = (long long)blockIdx.x * DMC_CHUNK;
    const int n = (int)(B - c0 < DMC_CHUNK ? B - c0 : DMC_CHUNK);
    for (int i = threadIdx.x; i < n; i += 64) sh[i] = weight[c0 + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = sh[0];
        for (int i = 1; i < n; ++i) { s += sh[i]; sh[i] = s; }
        chunk_sum[blockIdx.x] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 64) r[c0 + i] = sh[i];
}

// off[c] = O_c; tot[0] = W = O_last + r_last, tot[1] = W / B, tot[2] = 1 if W is finite and positive (the comb runs) else 0,
// tot[3] = the number of j with C_j < W: the last walker of positive weight, which the parents are clamped to (a tooth that
// rounding puts on the last edge must not revive the dead walkers behind it)
__global__ void __launch_bounds__(256) k_dmc_scan_offsets(long long B, int n_chunks, const double* __restrict__ chunk_sum,
                                                          const double* __restrict__ r, double* __restrict__ off,
                                                          double* __restrict__ tot) {
    __shared__ double sh[DMC_MAX_B / DMC_CHUNK];
    for (int c = threadIdx.x; c < n_chunks; c += 256) sh[c] = chunk_sum[c];
    __syncthreads();
    if (threadIdx.x == 0) {
        double o = 0.0;
        for (int c = 0; c < n_chunks; ++c) { const double s = sh[c]; sh[c] = o; o += s; }
        tot[0] = o;
        tot[1] = o / (double)B;
        const bool run = isfinite(o) && o > 0.0;
        tot[2] = run ? 1.0 : 0.0;
        long long lo = 0, hi = B - 1;                  // first j with C_j >= W (C_{B-1} = W)
        while (run && lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (sh[mid / DMC_CHUNK] + r[mid] < o) lo = mid + 1;
            else hi = mid;
        }
        tot[3] = (double)lo;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n_chunks; c += 256) off[c] = sh[c];
}

// parent of tooth k = number of j with C_j - k (W/B) <= xi (W/B), clamped to `last` (tot[3]): both products and the difference are rounded on
// their own, so that the model repeats the comparison bit for bit.  The count is found by bisection (the left side does not
// decrease with j).  cnt[block] = teeth of the block whose parent differs from that of the tooth before (tooth 0 counts).
__device__ __forceinline__ long long dmc_parent(long long k, long long B, long long last, double step, double rhs,
                                                const double* __restrict__ r, const double* __restrict__ off) {
#pragma clang fp contract(off)
    const double base = (double)k * step;
    long long lo = 0, hi = B;                          // first j in [lo, hi] whose edge lies above the tooth
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const double cj = off[mid / DMC_CHUNK] + r[mid];
        if (cj - base <= rhs) lo = mid + 1;
        else hi = mid;
    }
    return lo < last ? lo : last;
}

__global__ void __launch_bounds__(256) k_dmc_select(long long B, double xi, const double* __restrict__ xi_dev,
                                                    const double* __restrict__ r, const double* __restrict__ off,
                                                    const double* __restrict__ tot, int* __restrict__ parent, int* __restrict__ cnt,
                                                    int* __restrict__ out_parents) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool run = tot[2] != 0.0;
    int distinct = 0;
    if (k < B) {
        long long p = k;
        if (run) {
            double rhs;
            const double step = tot[1], x = xi_dev ? xi_dev[0] : xi;
            {
#pragma clang fp contract(off)
                rhs = x * step;
            }
            const long long last = (long long)tot[3];
            p = dmc_parent(k, B, last, step, rhs, r, off);
            distinct = (k == 0 || dmc_parent(k - 1, B, last, step, rhs, r, off) != p) ? 1 : 0;
        }
        parent[k] = (int)p;
        if (out_parents) out_parents[k] = (int)p;
    }
    const int n = __syncthreads_count(distinct);
    if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

// What step `step` of a call draws in Philox mode, in the layout of the explicit mode: normals (B,3N) and uniforms (B,) rounded to
// T as the step kernels round them, and the comb's xi (stream 2 at index B) in float64
template <typename T>
__global__ void __launch_bounds__(256) k_dmc_noise(PhiloxKey key, unsigned long long step, size_t n_elec, long long B,
                                                   T* __restrict__ normal, T* __restrict__ uniform, double* __restrict__ xi) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_elec) {
        double z[3];
        philox_normal3(key, step, e, z);
        for (int c = 0; c < 3; ++c) normal[3 * e + c] = (T)z[c];
    }
    if (e < (size_t)B) uniform[e] = (T)philox_uniform(key, step, (unsigned long long)e);
    if (e == (size_t)B) xi[0] = philox_uniform(key, step, (unsigned long long)B);
}

// out_parents of a step without a comb: every walker is its own parent
static __global__ void k_dmc_identity(long long B, int* __restrict__ out_parents) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < B) out_parents[k] = (int)k;
}

// one wave per destination walker: the parent's rows into the second buffer (the state itself is only read)
template <typename T>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_gather(long long B, int n3, const double* __restrict__ tot,
                                                               const int* __restrict__ parent, const T* __restrict__ x,
                                                               const T* __restrict__ logabs, const T* __restrict__ phase,
                                                               const T* __restrict__ drift, const double* __restrict__ eloc,
                                                               T* __restrict__ bx, T* __restrict__ bla, T* __restrict__ bph,
                                                               T* __restrict__ bdr, double* __restrict__ bel) {
    const long long k = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= B || tot[2] == 0.0) return;
    const size_t src = (size_t)parent[k] * n3, dst = (size_t)k * n3;
    for (int c = lane; c < n3; c += 64) { bx[dst + c] = x[src + c]; bdr[dst + c] = drift[src + c]; }
    if (lane == 0) {
        const long long p = parent[k];
        bla[k] = logabs[p]; bph[2 * k] = phase[2 * p]; bph[2 * k + 1] = phase[2 * p + 1]; bel[k] = eloc[p];
    }
}

// ... and back; every weight becomes W / B.  Workgroup 0 adds the distinct-parent counts (exact integers) into the stats row:
// the count, or 0 for a comb that was skipped because W is not finite or not positive.
template <typename T>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_copy_back(long long B, int n3, const double* __restrict__ tot,
                                                                  const int* __restrict__ cnt, int n_cnt, const T* __restrict__ bx,
                                                                  const T* __restrict__ bla, const T* __restrict__ bph,
                                                                  const T* __restrict__ bdr, const double* __restrict__ bel,
                                                                  T* __restrict__ x, T* __restrict__ logabs, T* __restrict__ phase,
                                                                  T* __restrict__ drift, double* __restrict__ eloc,
                                                                  double* __restrict__ weight, double* __restrict__ stat_distinct) {
    const long long k = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool run = tot[2] != 0.0;
    if (blockIdx.x == 0 && threadIdx.x < 64 && stat_distinct) {
        int n = 0;                                     // (at most B <= 2^20)
        for (int i = lane; i < n_cnt; i += 64) n += cnt[i];
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        if (lane == 0) stat_distinct[0] = run ? (double)n : 0.0;
    }
    if (k >= B || !run) return;
    const size_t row = (size_t)k * n3;
    for (int c = lane; c < n3; c += 64) { x[row + c] = bx[row + c]; drift[row + c] = bdr[row + c]; }
    if (lane == 0) {
        logabs[k] = bla[k]; phase[2 * k] = bph[2 * k]; phase[2 * k + 1] = bph[2 * k + 1]; eloc[k] = bel[k];
        weight[k] = tot[1];
    }
}

// ------------------------------------------------------------------------------------------------------------------ T-moves
// ds_dmc_step_tmove evaluates the pseudopotential AFTER the decision, at the position the walker then has, so k_dmc_accept splits:
//   k_dmc_tm_decide    one wave per walker: the decision (dmc_decide) with E_c' = Re ke' + ewald' for E'; (p, flags) and the
//                      selected position x_cur go to the workspace, the state is only read
//   (ds_ecp_energy's launches on x_cur; a pair total above the capacity ends the call here with the state untouched)
//   k_dmc_tm_commit    one wave per walker: selects the rows, E = ((E_c + E_loc) + Re E_nl), the one-point weight, epp, E
//   (k_ecp_tmove of ds_ecp.h: the heat-bath move of one electron; the stats rows)
//   (energy chain at x)
//   k_dmc_tm_refresh   one wave per walker: a walker that made a T-move takes logabs, phase, drift, eloc of that pass
template <typename T>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_tm_decide(DmcArgs A, const T* __restrict__ x, const T* __restrict__ logabs,
                                                                  const T* __restrict__ phase, const T* __restrict__ drift,
                                                                  const T* __restrict__ x2, const T* __restrict__ la2,
                                                                  const T* __restrict__ ph2, const T* __restrict__ gc2,
                                                                  const T* __restrict__ ke2, const T* __restrict__ ew2,
                                                                  const T* __restrict__ chi, const T* __restrict__ uniform, PhiloxKey key,
                                                                  unsigned long long step, double* __restrict__ pacc, int* __restrict__ flags,
                                                                  T* __restrict__ xcur) {
    const long long w = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= A.B) return;
    const int n3 = 3 * A.N;
    const size_t row = (size_t)w * n3;
    const DmcDecision d = dmc_decide(A, w, lane, logabs, phase, drift, la2, ph2, gc2, chi, uniform, key, step,
                                     [&] { return dmc_energy(ke2, ew2, w); });
    const T* src = d.acc ? x2 : x;
    for (int c = lane; c < n3; c += 64) xcur[row + c] = src[row + c];
    if (lane == 0) { pacc[w] = d.pacc(); flags[w] = d.flags; }
}

// epp2: the triple at x_cur; etot: E per walker for the stats row and the T-move (out_energy: a copy for the caller)
template <typename T>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_tm_commit(DmcArgs A, T* __restrict__ x, T* __restrict__ logabs, T* __restrict__ phase,
                                                                  T* __restrict__ drift, double* __restrict__ eloc,
                                                                  double* __restrict__ weight, double* __restrict__ epp,
                                                                  const T* __restrict__ x2, const T* __restrict__ la2,
                                                                  const T* __restrict__ ph2, const T* __restrict__ gc2,
                                                                  const T* __restrict__ ke2, const T* __restrict__ ew2,
                                                                  const double* __restrict__ epp2, int* __restrict__ flags,
                                                                  double* __restrict__ etot, double* __restrict__ out_energy) {
    const long long w = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= A.B) return;
    const int n3 = 3 * A.N;
    const size_t row = (size_t)w * n3;
    const int fl = flags[w];
    const bool acc = (fl & DMC_ACCEPTED) != 0;
    if (acc)
        for (int c = lane; c < n3; c += 64) { x[row + c] = x2[row + c]; drift[row + c] = gc2[2 * (row + c)]; }
    if (lane == 0) {
        const double e_c = acc ? dmc_energy(ke2, ew2, w) : eloc[w];
        const double e = dmc_energy_ecp(e_c, epp2, w);
        bool clipped;
        const double ce = dmc_clip(e, A.e_ref, A.e_cut, &clipped);
        double factor;
        {
#pragma clang fp contract(off)
            factor = exp(-A.tau_eff * (ce - A.e_trial));
        }
        const double wn = weight[w] * factor;
        weight[w] = isfinite(wn) ? wn : 0.0;              // an energy that is not finite kills the walker
        if (acc) { logabs[w] = la2[w]; phase[2 * w] = ph2[2 * w]; phase[2 * w + 1] = ph2[2 * w + 1]; eloc[w] = e_c; }
        for (int c = 0; c < 3; ++c) epp[3 * w + c] = epp2[3 * w + c];
        if (clipped) flags[w] = fl | DMC_CLIPPED;
        etot[w] = e;
        if (out_energy) out_energy[w] = e;
    }
}

// after the chain pass at the positions that follow the T-moves: gc / la2 / ph2 / ke2 / ew2 are that pass's outputs
template <typename T>
__global__ void __launch_bounds__(64 * DMC_WAVES) k_dmc_tm_refresh(long long B, int n3, const int* __restrict__ choice,
                                                                   const T* __restrict__ gc, const T* __restrict__ la2,
                                                                   const T* __restrict__ ph2, const T* __restrict__ ke2,
                                                                   const T* __restrict__ ew2, T* __restrict__ logabs, T* __restrict__ phase,
                                                                   T* __restrict__ drift, double* __restrict__ eloc,
                                                                   double* __restrict__ weight) {
    const long long w = (long long)blockIdx.x * DMC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= B || choice[w] < 0) return;
    dmc_set_walker<T, false>(w, lane, n3, gc, ke2, ew2, la2, nullptr, drift, eloc, weight);
    if (lane == 0) { logabs[w] = la2[w]; phase[2 * w] = ph2[2 * w]; phase[2 * w + 1] = ph2[2 * w + 1]; }
}

}  // namespace ds
