// ds_sample.hip -- the samplers and what shares their kernels (ds_mcmc.h, ds_onebody.h, ds_spin.h, ds_ecp.h, ds_ecp_force.h): the three
// fused Metropolis loops, the one-body ratios and n(k), the spin-exchange ratios and the sums of <S^2>, the pseudopotential energy, its
// forces and its handle, the single proposal / selection steps (ds_mh_*), the batch statistics and the host side of Philox.
#include "ds_host.h"
#include "ds_mcmc.h"
#include "ds_onebody.h"
#include "ds_spin.h"
#include "ds_ecp.h"
#include "ds_ecp_force.h"

struct ds_ecp {
    ds::EcpDev D;
    std::vector<void*> dev;                 // every device allocation, freed by ds_ecp_destroy
};

namespace ds {
namespace host {

// ------------------------------------------------------------------ Metropolis loop (qmc.py:335-362), ds_mcmc.h
// Scratch of the three move loops, in front of the chains' workspace: proposal x2 (B,3N) + log|psi(x2)| (B,); the importance-
// sampled loop adds the complex gradient (B,3N,2), the drifts at x1 / x2, the normal deviates ((B,3N) each), the uniforms (B,) and
// the two batch maxima
template <typename T> struct McmcScratch {
    T *X2, *GC, *G1, *G2, *NZ, *LA2, *UN, *SCR;
    void* wsv; int64_t wsv_bytes;                        // what is left for the value / energy chain
};
template <typename T> McmcScratch<T> carve_mcmc(const ds_system* s, Arena<T>& a, int64_t B) {
    const size_t n3 = (size_t)B * 3 * s->sd.N;
    McmcScratch<T> m{};
    m.X2 = a.take(n3); m.GC = a.take(2 * n3); m.G1 = a.take(n3); m.G2 = a.take(n3); m.NZ = a.take(n3);
    m.LA2 = a.take((size_t)B); m.UN = a.take((size_t)B); m.SCR = a.take(2);
    return m;
}
inline size_t mcmc_scratch_bytes(const ds_system* s, int64_t B) {
    return rup(measure([&](Arena<double>& a) { carve_mcmc<double>(s, a, B); }) * (s->dtype == 0 ? 8 : 4), 256);
}

// What the three loops begin with: the workspace check, the carve, and logprob = 2 f(data) (qmc.py:357) unless lp is valid
template <typename T>
int mcmc_begin(ds_system* s, const char* what, const void* params, const T* x, T* lp, int64_t B, int lp_valid, void* ws,
               int64_t ws_bytes, hipStream_t st, McmcScratch<T>* m) {
    const size_t head = mcmc_scratch_bytes(s, B);
    if ((int64_t)head >= ws_bytes) return fail("workspace too small for %s (see ds_mcmc_workspace_bytes)", what);
    Arena<T> a = arena_of<T>(ws, (int64_t)head);
    *m = carve_mcmc<T>(s, a, B);
    if (!a.ok) return carve_fail(what);
    m->wsv = (char*)ws + head;
    m->wsv_bytes = ws_bytes - (int64_t)head;
    if (!lp_valid) {
        if (int rc = logpsi_forward(s, params, x, B, m->LA2, nullptr, m->wsv, m->wsv_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_scale2<T>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, m->LA2, (long)B, lp);
    }
    return 0;
}

template <typename T>
int mcmc_step_impl(ds_system* s, const void* params, void* x_, void* lp_, int64_t B, int steps, double width, uint64_t seed,
                   uint64_t offset, const void* normals_, const void* uniforms_, int lp_valid, void* n_accept, void* ws,
                   int64_t ws_bytes, hipStream_t st, int first_electron = -1) {
    const ds::SysDev<T>& S = dev<T>(s);
    T* x = (T*)x_; T* lp = (T*)lp_;
    McmcScratch<T> m;
    if (int rc = mcmc_begin<T>(s, "ds_mcmc_step", params, x, lp, B, lp_valid, ws, ws_bytes, st, &m)) return rc;
    const T* normals = (const T*)normals_; const T* uniforms = (const T*)uniforms_;
    const size_t ne = (size_t)B * S.N;
    const ds::PhiloxKey key{seed, offset};
    for (int i = 0; i < steps; ++i) {                                    // lax.fori_loop(0, nsteps, ...)   :358
        // all-electron move, or (first_electron >= 0) move i displaces electron (first_electron + i) % N only  (qmc.py:266)
        const int only = first_electron < 0 ? -1 : (int)(((int64_t)first_electron + i) % S.N);
        const size_t nstride = (size_t)B * 3 * (only < 0 ? S.N : 1);
        hipLaunchKernelGGL((ds::k_mcmc_propose<T>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, S.sim_a, S.sim_ainv, x,
                           normals ? normals + (size_t)i * nstride : (const T*)nullptr, key, (unsigned long long)i, (T)width, ne, m.X2,
                           S.N, only);
        if (int rc = logpsi_forward(s, params, m.X2, B, m.LA2, nullptr, m.wsv, m.wsv_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_mcmc_accept<T>), dim3((unsigned)((B + 63) / 64)), dim3(256), 0, st, x, lp, m.X2, m.LA2,
                           uniforms ? uniforms + (size_t)i * B : (const T*)nullptr, key, (unsigned long long)i, 3 * S.N, 0L, (long)B, (T*)n_accept);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ one-body ratios and n(k), ds_onebody.h
// Workspace of ds_one_body_ratios for B walkers and chunks of ng groups of PV displaced configurations.  Shared by all chunks:
// log|psi(R)| (B,), phase(R) (B,2) and the call's running sums (one row of float64, taken as 2 elements per double: room in
// either element size).  Per chunk: one row of float64 partials per group, the displaced rows, their log|psi| / phase, and the value chain's buffers for ng groups (on a 64-element
// border), which also serve the forward of the undisplaced walkers.
template <typename T> struct OneBodyWs {
    T *LA0, *PH0, *XD, *LA, *PH;
    double *ACC, *PART;
    void* wsv; int64_t wsv_bytes;
};
template <typename T> OneBodyWs<T> carve_onebody(const ds_system* s, Arena<T>& a, int64_t B, int64_t ng) {
    const size_t nc = (size_t)ng * ds::PV;
    OneBodyWs<T> w{};
    w.LA0 = a.take((size_t)B); w.PH0 = a.take(2 * (size_t)B);
    a.align(2);
    w.ACC = (double*)a.take(2 * (size_t)ds::OB_ROW);
    w.PART = (double*)a.take(2 * (size_t)ng * ds::OB_ROW);
    w.XD = a.take(nc * 3 * s->sd.N); w.LA = a.take(nc); w.PH = a.take(2 * nc);
    a.align(64);
    w.wsv = a.take(s->wsv.per_walker * (size_t)ng);
    w.wsv_bytes = (int64_t)(s->wsv.per_walker * (size_t)ng * sizeof(T));
    return w;
}
inline int64_t onebody_bytes(const ds_system* s, int64_t B, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_onebody<double>(s, a, B, ng); }) * (s->dtype == 0 ? 8 : 4);
}

template <typename T>
int one_body_impl(ds_system* s, const void* params, const void* x_, int64_t B, int M, int first, uint64_t seed, uint64_t offset,
                  const void* shifts_, const double* kvec, int n_k, double* nk_sums, void* out_ratio, void* out_shift,
                  int64_t* n_bad, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const T* x = (const T*)x_; const T* shifts = (const T*)shifts_;
    const int64_t total = B * (int64_t)M;
    // the chunk length follows from the workspace: the largest number of groups whose layout fits (the layout is linear in ng up
    // to its two alignment pads, so the estimate is at most a few groups high)
    const int64_t fixed = onebody_bytes(s, B, 0), per = onebody_bytes(s, B, 1) - fixed;
    int64_t ng = std::min<int64_t>({(ws_bytes - fixed) / per + 1, OB_MAX_GROUPS, (total + ds::PV - 1) / ds::PV});
    while (ng >= 1 && onebody_bytes(s, B, ng) > ws_bytes) --ng;
    if (ng < 1) return fail("workspace too small for ds_one_body_ratios: %lld bytes < %lld for one group of %d configurations",
                            (long long)ws_bytes, (long long)onebody_bytes(s, B, 1), ds::PV);
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const OneBodyWs<T> w = carve_onebody<T>(s, a, B, ng);
    if (!a.ok) return carve_fail("one-body ratios");
    const ValI8Call one_path(s, S.N, total);         // (the same value-chain kernels whatever the chunks are)
    if (int rc = logpsi_forward(s, params, x, B, w.LA0, w.PH0, w.wsv, w.wsv_bytes, st)) return rc;
    ds::OneBodyArgs A;
    for (int i = 0; i < 9; ++i) A.a[i] = s->d.sim_a[i];
    A.key = ds::PhiloxKey{seed, offset};
    A.M = M; A.N = S.N; A.n_up = S.n_up; A.first = first;
    const int64_t chunk = ng * ds::PV;
    for (int64_t g0 = 0; g0 < total; g0 += chunk) {
        A.g0 = g0; A.n = std::min(chunk, total - g0);
        const int64_t groups = (A.n + ds::OB_GROUP - 1) / ds::OB_GROUP;
        hipLaunchKernelGGL((ds::k_onebody_propose<T>), dim3((unsigned)((A.n * S.N + 255) / 256)), dim3(256), 0, st, A, x, shifts, w.XD,
                           (T*)out_shift);
        if (int rc = logpsi_forward(s, params, w.XD, A.n, w.LA, w.PH, w.wsv, w.wsv_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_onebody_accumulate<T>), dim3((unsigned)groups), dim3(64 * ds::OB_WAVES), 0, st, A, shifts, (const T*)w.LA0,
                           (const T*)w.PH0, (const T*)w.LA, (const T*)w.PH, kvec, n_k, (T*)out_ratio, w.PART);
        if (n_k > 0 || n_bad)
            hipLaunchKernelGGL(ds::k_onebody_final, dim3((unsigned)((4 * n_k + 2 + 255) / 256)), dim3(256), 0, st, (const double*)w.PART,
                               (long long)groups, n_k, g0 == 0 ? 1 : 0, g0 + chunk >= total ? 1 : 0, w.ACC, nk_sums, (long long*)n_bad);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ spin-exchange ratios and the sums of <S^2>, ds_spin.h
// Workspace of ds_spin_exchange_ratios for B walkers, M samples per walker and chunks of ng groups of PV exchanged configurations.
// Shared by all chunks: log|psi(R)| (B,), phase(R) (B,2), and in float64 (2 elements per double: room in either element size) every
// ratio of the call (B,M,2) and the walker sums (B,2).  Per chunk: the exchanged rows, their log|psi| / phase, and the value chain's
// buffers for ng groups (on a 64-element border), which also serve the forward of the walkers themselves.
template <typename T> struct SpinWs {
    T *LA0, *PH0, *XD, *LA, *PH;
    double *Q, *TW;
    void* wsv; int64_t wsv_bytes;
};
template <typename T> SpinWs<T> carve_spin(const ds_system* s, Arena<T>& a, int64_t B, int64_t M, int64_t ng) {
    const size_t nc = (size_t)ng * ds::PV;
    SpinWs<T> w{};
    w.LA0 = a.take((size_t)B); w.PH0 = a.take(2 * (size_t)B);
    a.align(2);
    w.Q = (double*)a.take(4 * (size_t)B * (size_t)M);
    w.TW = (double*)a.take(4 * (size_t)B);
    w.XD = a.take(nc * 3 * s->sd.N); w.LA = a.take(nc); w.PH = a.take(2 * nc);
    a.align(64);
    w.wsv = a.take(s->wsv.per_walker * (size_t)ng);
    w.wsv_bytes = (int64_t)(s->wsv.per_walker * (size_t)ng * sizeof(T));
    return w;
}
inline int64_t spin_bytes(const ds_system* s, int64_t B, int64_t M, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_spin<double>(s, a, B, M, ng); }) * (s->dtype == 0 ? 8 : 4);
}

template <typename T>
int spin_exchange_impl(ds_system* s, const void* params, const void* x_, int64_t B, int M, int first, double* sums, void* out_ratio,
                       double* out_walker, int64_t* n_bad, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const T* x = (const T*)x_;
    const int64_t total = B * (int64_t)M;
    // the chunk length follows from the workspace, as in one_body_impl
    const int64_t fixed = spin_bytes(s, B, M, 0), per = spin_bytes(s, B, M, 1) - fixed;
    int64_t ng = std::min<int64_t>({(ws_bytes - fixed) / per + 1, OB_MAX_GROUPS, (total + ds::PV - 1) / ds::PV});
    while (ng >= 1 && spin_bytes(s, B, M, ng) > ws_bytes) --ng;
    if (ng < 1) return fail("workspace too small for ds_spin_exchange_ratios: %lld bytes < %lld for one group of %d configurations",
                            (long long)ws_bytes, (long long)spin_bytes(s, B, M, 1), ds::PV);
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const SpinWs<T> w = carve_spin<T>(s, a, B, M, ng);
    if (!a.ok) return carve_fail("spin-exchange ratios");
    const ValI8Call one_path(s, S.N, total);         // (the same value-chain kernels whatever the chunks are)
    if (int rc = logpsi_forward(s, params, x, B, w.LA0, w.PH0, w.wsv, w.wsv_bytes, st)) return rc;
    ds::SpinArgs A;
    A.M = M; A.N = S.N; A.n_up = S.n_up; A.n_dn = S.n_dn; A.first = first;
    const int64_t chunk = ng * ds::PV;
    for (int64_t g0 = 0; g0 < total; g0 += chunk) {
        A.g0 = g0; A.n = std::min(chunk, total - g0);
        hipLaunchKernelGGL((ds::k_spin_propose<T>), dim3((unsigned)((A.n * S.N + 255) / 256)), dim3(256), 0, st, A, x, w.XD);
        if (int rc = logpsi_forward(s, params, w.XD, A.n, w.LA, w.PH, w.wsv, w.wsv_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_spin_ratio<T>), dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, st, A, (const T*)w.LA0, (const T*)w.PH0,
                           (const T*)w.LA, (const T*)w.PH, w.Q, (T*)out_ratio);
    }
    if (sums || out_walker || n_bad) {
        hipLaunchKernelGGL(ds::k_spin_walker, dim3((unsigned)((B + ds::SPIN_WAVES - 1) / ds::SPIN_WAVES)), dim3(64 * ds::SPIN_WAVES), 0, st,
                           (const double*)w.Q, (long long)B, M, w.TW, out_walker);
        if (sums || n_bad)
            hipLaunchKernelGGL(ds::k_spin_final, dim3(1), dim3(256), 0, st, (const double*)w.TW, (long long)B, sums, (long long*)n_bad);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ pseudopotential energy, ds_ecp.h
template <typename T>
int ecp_energy_impl(ds_system* s, const ds_ecp* e, const void* params, const void* x_, int64_t B, uint64_t seed, uint64_t offset,
                    const double* rotations, int64_t cap, double* out_energy, int64_t* out_pairs, void* out_ratio, double* out_rotation,
                    void* ws, int64_t ws_bytes, hipStream_t st, int64_t* pairs_total, int64_t* pairs_total_dev, void* view) {
    const ds::SysDev<T>& S = dev<T>(s);
    const ds::EcpDev& E = e->D;
    const T* x = (const T*)x_;
    const int nq = E.n_quad;
    // the chunk length follows from the workspace, as in one_body_impl; the pair total is not known yet, the capacity bounds it
    const int64_t fixed = ecp_bytes(s, B, cap, nq, 0), per = ecp_bytes(s, B, cap, nq, 1) - fixed;
    int64_t ng = std::min<int64_t>({(ws_bytes - fixed) / per + 1, OB_MAX_GROUPS, (cap * nq + ds::PV - 1) / ds::PV});
    while (ng >= 1 && ecp_bytes(s, B, cap, nq, ng) > ws_bytes) --ng;
    if (ng < 1) return fail("workspace too small for ds_ecp_energy: %lld bytes < %lld for one group of %d configurations",
                            (long long)ws_bytes, (long long)ecp_bytes(s, B, cap, nq, 1), ds::PV);
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const EcpWs<T> w = carve_ecp<T>(s, a, B, cap, nq, ng);
    if (!a.ok) return carve_fail("pseudopotential energy");
    if (view) *(EcpWs<T>*)view = w;
    const dim3 gw((unsigned)((B + 63) / 64)), bw(64);
    hipLaunchKernelGGL((ds::k_ecp_scan<T>), gw, bw, 0, st, E, x, (long long)B, S.N, ds::PhiloxKey{seed, offset}, rotations, w.ROT, w.ELOC,
                       w.CNT, w.BAD, out_rotation);
    hipLaunchKernelGGL(ds::k_ecp_offsets, dim3(1), dim3(1024), 0, st, (const long long*)w.CNT, (long long)B, w.OFF, (long long*)out_pairs);
    hipLaunchKernelGGL((ds::k_ecp_fill<T>), gw, bw, 0, st, E, x, (long long)B, S.N, (const int*)w.BAD, (const long long*)w.OFF,
                       (long long)cap, w.PW, w.PI, w.PR, w.PVL);
    // the one synchronisation of the call: the host needs the pair total to size the chunks
    long long pairs = 0;
    HIP_OK(hipMemcpyAsync(&pairs, w.OFF + B, sizeof(long long), hipMemcpyDeviceToHost, st));
    if (pairs_total_dev) HIP_OK(hipMemcpyAsync(pairs_total_dev, w.OFF + B, sizeof(long long), hipMemcpyDeviceToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    if (pairs_total) *pairs_total = pairs;
    if (pairs > cap)
        return fail("ds_ecp_energy: pair capacity exceeded: the walkers have %lld pairs inside the non-local cutoffs, pair_capacity is %lld",
                    pairs, (long long)cap);
    const int64_t total = pairs * nq;
    const ValI8Call one_path(s, S.N, total);         // (the same value-chain kernels whatever the chunks are)
    if (total > 0)
        if (int rc = logpsi_forward(s, params, x, B, w.LA0, w.PH0, w.wsv, w.wsv_bytes, st)) return rc;
    ds::EcpChunk A;
    A.N = S.N; A.n_quad = nq;
    const int64_t chunk = ng * ds::PV;
    for (int64_t c0 = 0; c0 < total; c0 += chunk) {
        A.c0 = c0; A.n = std::min(chunk, total - c0);
        hipLaunchKernelGGL((ds::k_ecp_propose<T>), dim3((unsigned)((A.n * S.N + 255) / 256)), dim3(256), 0, st, E, A, x, (const double*)w.ROT,
                           (const long long*)w.PW, (const int*)w.PI, (const double*)w.PR, w.XD);
        if (int rc = logpsi_forward(s, params, w.XD, A.n, w.LA, w.PH, w.wsv, w.wsv_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_ecp_term<T>), dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, st, E, A, (const double*)w.ROT,
                           (const long long*)w.PW, (const double*)w.PR, (const double*)w.PVL, (const T*)w.LA0, (const T*)w.PH0,
                           (const T*)w.LA, (const T*)w.PH, w.TERM, (T*)out_ratio);
    }
    hipLaunchKernelGGL(ds::k_ecp_walker, dim3((unsigned)((B + ds::ECP_WAVES - 1) / ds::ECP_WAVES)), dim3(64 * ds::ECP_WAVES), 0, st,
                       (const double*)w.TERM, (const long long*)w.OFF, (const double*)w.ELOC, (const int*)w.BAD, (long long)B, nq, out_energy);
    HIP_OK(hipGetLastError());
    return 0;
}

int ecp_energy_forward(ds_system* s, const ds_ecp* e, const void* params, const void* x, int64_t B, uint64_t seed, uint64_t offset,
                       const double* rotations, int64_t cap, double* out_energy, int64_t* out_pairs, void* out_ratio, double* out_rotation,
                       void* ws, int64_t ws_bytes, hipStream_t st, int64_t* pairs_total, int64_t* pairs_total_dev, void* view) {
    return DS_BY_DTYPE(s->dtype, ecp_energy_impl, s, e, params, x, B, seed, offset, rotations, cap, out_energy, out_pairs, out_ratio,
                       out_rotation, ws, ws_bytes, st, pairs_total, pairs_total_dev, view);
}

template <typename T>
int ecp_tmove_impl(ds_system* s, const ds_ecp* e, const void* view, void* x, int64_t B, double tau, const double* weight,
                   const double* energy, const double* uniforms, uint64_t seed, uint64_t offset, uint64_t step, int* choice, int* out_choice,
                   hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const EcpWs<T>& w = *(const EcpWs<T>*)view;
    hipLaunchKernelGGL((ds::k_ecp_tmove<T>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, e->D, S.sim_a, S.sim_ainv, (T*)x, (long long)B,
                       S.N, tau, (const double*)w.ROT, (const long long*)w.OFF, (const int*)w.PI, (const double*)w.PR, (const double*)w.TERM,
                       weight, energy, uniforms, ds::PhiloxKey{seed, offset}, (unsigned long long)step, choice, out_choice);
    return 0;
}

int ecp_tmove(ds_system* s, const ds_ecp* e, const void* view, void* x, int64_t B, double tau, const double* weight, const double* energy,
              const double* uniforms, uint64_t seed, uint64_t offset, uint64_t step, int* choice, int* out_choice, hipStream_t st) {
    return DS_BY_DTYPE(s->dtype, ecp_tmove_impl, s, e, view, x, B, tau, weight, energy, uniforms, seed, offset, step, choice, out_choice, st);
}

int ecp_n_quad(const ds_ecp* e) { return e->D.n_quad; }

// ------------------------------------------------------------------ pseudopotential forces, ds_ecp_force.h
// Workspace of ds_ecp_forces for B walkers, A ions, at most `cap` pairs, nq points per pair and chunks of ng groups of PV
// configurations.  Shared by all chunks: what carve_ecp shares (log|psi(R)|, phase(R), and in 8-byte elements the rotation, E_loc, the
// pair count, the offsets and the flag per walker, the pair records), then the second flag (a pair at r = 0), the second record array
// v'_l(r), 6 nq terms per pair, F^loc (B, A, 3), the rows (B, 2, A, 3) = (F^pp, F^tot) and one row of partial sums per 256 walkers.
// Per chunk: the displaced rows, their log|psi| / phase / gradient, and the forward-Laplacian chain's buffers for ng PV walkers (on
// a 64-element border), which also serve the pass over the walkers themselves.
template <typename T> struct EcpForceWs {
    T *LA0, *PH0, *XD, *LA, *PH, *GR;
    double *ROT, *ELOC, *PR, *PVL, *PDV, *TERM, *FLOC, *ROWS, *PART;
    long long *CNT, *OFF, *PW;
    int *BAD, *BADF, *PI;
    void* wsc; int64_t wsc_bytes;
};
template <typename T> EcpForceWs<T> carve_ecp_force(const ds_system* s, Arena<T>& a, int64_t B, int A, int64_t cap, int nq, int64_t ng) {
    const size_t nc = (size_t)ng * ds::PV, b = (size_t)B, p = (size_t)cap, groups = (b + FORCE_SUM_GROUP - 1) / FORCE_SUM_GROUP;
    EcpForceWs<T> w{};
    w.LA0 = a.take(b); w.PH0 = a.take(2 * b);
    a.align(2);
    w.ROT = (double*)a.take(2 * 9 * b); w.ELOC = (double*)a.take(2 * b);
    w.CNT = (long long*)a.take(2 * b); w.OFF = (long long*)a.take(2 * (b + 1));
    w.BAD = (int*)a.take(2 * ((b + 1) / 2)); w.BADF = (int*)a.take(2 * ((b + 1) / 2));
    w.PW = (long long*)a.take(2 * p); w.PI = (int*)a.take(2 * p);
    w.PR = (double*)a.take(2 * 4 * p); w.PVL = (double*)a.take(2 * 3 * p); w.PDV = (double*)a.take(2 * 3 * p);
    w.TERM = (double*)a.take(2 * 6 * p * (size_t)nq);
    w.FLOC = (double*)a.take(2 * 3 * (size_t)A * b); w.ROWS = (double*)a.take(2 * 6 * (size_t)A * b);
    w.PART = (double*)a.take(2 * groups * (12 * (size_t)A + 1));
    w.XD = a.take(nc * 3 * s->sd.N); w.LA = a.take(nc); w.PH = a.take(2 * nc); w.GR = a.take(nc * 3 * s->sd.N * 2);
    a.align(64);
    w.wsc = a.take(s->ws.per_walker * nc);
    w.wsc_bytes = (int64_t)(s->ws.per_walker * nc * sizeof(T));
    return w;
}
inline int64_t ecp_force_bytes(const ds_system* s, int64_t B, int A, int64_t cap, int nq, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_ecp_force<double>(s, a, B, A, cap, nq, ng); }) * (s->dtype == 0 ? 8 : 4);
}

template <typename T>
int ecp_forces_impl(ds_system* s, const ds_ecp* e, const void* params, const void* x_, int64_t B, uint64_t seed, uint64_t offset,
                    const double* rotations, int64_t cap, const double* base, double* out_force, double* sums, int64_t* n_bad,
                    int64_t* out_pairs, double* out_rotation, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const ds::EcpDev& E = e->D;
    const T* x = (const T*)x_;
    const int nq = E.n_quad, A = E.n_atoms;
    // the chunk length follows from the workspace, as in ecp_energy_impl, with the forward-Laplacian chain's per-walker layout
    const int64_t fixed = ecp_force_bytes(s, B, A, cap, nq, 0), per = ecp_force_bytes(s, B, A, cap, nq, 1) - fixed;
    int64_t ng = std::min<int64_t>({(ws_bytes - fixed) / per + 1, OB_MAX_GROUPS, (std::max(cap * nq, B) + ds::PV - 1) / ds::PV});
    while (ng >= 1 && ecp_force_bytes(s, B, A, cap, nq, ng) > ws_bytes) --ng;
    if (ng < 1) return fail("workspace too small for ds_ecp_forces: %lld bytes < %lld for one group of %d configurations",
                            (long long)ws_bytes, (long long)ecp_force_bytes(s, B, A, cap, nq, 1), ds::PV);
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const EcpForceWs<T> w = carve_ecp_force<T>(s, a, B, A, cap, nq, ng);
    if (!a.ok) return carve_fail("pseudopotential forces");
    const dim3 gw((unsigned)((B + 63) / 64)), bw(64);
    hipLaunchKernelGGL((ds::k_ecp_scan<T>), gw, bw, 0, st, E, x, (long long)B, S.N, ds::PhiloxKey{seed, offset}, rotations, w.ROT, w.ELOC,
                       w.CNT, w.BAD, out_rotation);
    hipLaunchKernelGGL(ds::k_ecp_offsets, dim3(1), dim3(1024), 0, st, (const long long*)w.CNT, (long long)B, w.OFF, (long long*)out_pairs);
    hipLaunchKernelGGL((ds::k_ecp_fill<T>), gw, bw, 0, st, E, x, (long long)B, S.N, (const int*)w.BAD, (const long long*)w.OFF,
                       (long long)cap, w.PW, w.PI, w.PR, w.PVL);
    // the one synchronisation of the call: the host needs the pair total to size the chunks
    long long pairs = 0;
    HIP_OK(hipMemcpyAsync(&pairs, w.OFF + B, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (pairs > cap)
        return fail("ds_ecp_forces: pair capacity exceeded: the walkers have %lld pairs inside the non-local cutoffs, pair_capacity is %lld",
                    pairs, (long long)cap);
    hipLaunchKernelGGL((ds::k_ecp_force_local<T>), gw, bw, 0, st, E, x, (long long)B, S.N, (const int*)w.BAD, w.FLOC, w.BADF);
    const int64_t total = pairs * nq, chunk = ng * ds::PV, stride = cap * nq;
    if (total > 0) {
        hipLaunchKernelGGL(ds::k_ecp_fill_deriv, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, E, pairs, (const int*)w.PI,
                           (const double*)w.PR, w.PDV);
        // log psi(R) of the ratios: the same chain, one pass over the B walkers (its gradient is not used)
        for (int64_t b0 = 0; b0 < B; b0 += chunk) {
            const int64_t nb = std::min(chunk, B - b0);
            if (int rc = logpsi_grad_forward(s, params, x + b0 * 3 * S.N, nb, w.LA0 + b0, w.PH0 + 2 * b0, w.GR, w.wsc, w.wsc_bytes, st)) return rc;
        }
    }
    ds::EcpChunk C;
    C.N = S.N; C.n_quad = nq;
    for (int64_t c0 = 0; c0 < total; c0 += chunk) {
        C.c0 = c0; C.n = std::min(chunk, total - c0);
        hipLaunchKernelGGL((ds::k_ecp_propose<T>), dim3((unsigned)((C.n * S.N + 255) / 256)), dim3(256), 0, st, E, C, x, (const double*)w.ROT,
                           (const long long*)w.PW, (const int*)w.PI, (const double*)w.PR, w.XD);
        if (int rc = logpsi_grad_forward(s, params, w.XD, C.n, w.LA, w.PH, w.GR, w.wsc, w.wsc_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_ecp_force_term<T>), dim3((unsigned)((C.n + 255) / 256)), dim3(256), 0, st, E, C, (const double*)w.ROT,
                           (const long long*)w.PW, (const int*)w.PI, (const double*)w.PR, (const double*)w.PVL, (const double*)w.PDV,
                           (const T*)w.LA0, (const T*)w.PH0, (const T*)w.LA, (const T*)w.PH, (const T*)w.GR, (long long)stride, w.TERM);
    }
    hipLaunchKernelGGL(ds::k_ecp_force_walker, dim3((unsigned)B), dim3(64 * ds::ECPF_WAVES), 0, st, (const double*)w.TERM, (long long)stride,
                       (const long long*)w.OFF, (const int*)w.PI, (const double*)w.FLOC, (const int*)w.BADF, base, A, nq, out_force,
                       sums ? w.ROWS : (double*)nullptr, (unsigned long long*)n_bad);
    HIP_OK(hipGetLastError());
    if (sums) return force_sums(w.ROWS, B, A, w.PART, sums, st);
    return 0;
}

int64_t ecp_default_groups(const ds_system* s, int64_t B, int64_t pair_capacity, int nq) {
    // as many groups per chunk as ds_workspace_bytes gives the value chain of pair_capacity * n_quad walkers
    const int64_t esz = s->dtype == 0 ? 8 : 4, total = pair_capacity * nq;
    const int64_t fixed = ecp_bytes(s, B, pair_capacity, nq, 0), per = ecp_bytes(s, B, pair_capacity, nq, 1) - fixed;
    return std::min(groups_per_pass(total, esz, PassSize{0, (size_t)(per / esz)}, workspace_budget()), OB_MAX_GROUPS);
}

// what ds_ecp_workspace_bytes and ds_ecp_energy refuse alike
int ecp_check(const ds_system* s, const ds_ecp* e, int64_t B, int64_t pair_capacity) {
    if (!s || !e) return fail("ds_ecp_energy: null system or pseudopotential descriptor");
    if (B < 1) return fail("ds_ecp_energy: B must be >= 1 (got %lld)", (long long)B);
    if (pair_capacity < 1) return fail("ds_ecp_energy: pair_capacity must be >= 1 (got %lld)", (long long)pair_capacity);
    if (e->D.n_atoms != s->d.n_atoms_sim)
        return fail("ds_ecp_energy: the descriptor has %d atoms, the system's simulation cell %d", e->D.n_atoms, s->d.n_atoms_sim);
    double scale = 0.0;
    for (int i = 0; i < 9; ++i) scale = std::max(scale, std::fabs(s->d.sim_a[i]));
    for (int i = 0; i < 9; ++i)
        if (!(std::fabs(e->D.a[i] - s->d.sim_a[i]) <= 1e-12 * scale))
            return fail("ds_ecp_energy: the descriptor's cell differs from the system's simulation cell (entry %d: %.17g against %.17g)", i,
                        e->D.a[i], s->d.sim_a[i]);
    return 0;
}

template <typename V> int ecp_upload(ds_ecp* h, const std::vector<V>& host, const V** out) {
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, (host.empty() ? 1 : host.size()) * sizeof(V)));
    h->dev.push_back(d);
    if (!host.empty()) HIP_OK(hipMemcpy(d, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice));
    *out = (const V*)d;
    return 0;
}

// The descriptor's checks, which need no device: the first violated one as a ds_last_error message
int ecp_validate(const ds_ecp_desc* d) {
    if (!d->atoms || !d->atom_species || !d->n_l || !d->r_cut_loc || !d->r_cut_nl || !d->term_offset)
        return fail("ds_ecp_create: null array in the descriptor");
    if (d->n_atoms < 1 || d->n_species < 1) return fail("ds_ecp_create: no atoms or no species");
    if (d->n_quad != 6 && d->n_quad != 12) return fail("ds_ecp_create: n_quad must be 6 or 12 (got %d)", d->n_quad);
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(d->a[i])) return fail("ds_ecp_create: lattice entry %d is not finite", i);
    double ainv[9], hmin = 1e300;
    inv3(d->a, ainv);
    for (int c = 0; c < 3; ++c) {
        const double n = std::sqrt(ainv[c] * ainv[c] + ainv[3 + c] * ainv[3 + c] + ainv[6 + c] * ainv[6 + c]);
        if (!(n > 0.0) || !std::isfinite(n)) return fail("ds_ecp_create: the simulation cell is singular");
        hmin = std::min(hmin, 1.0 / n);
    }
    const int degree = d->n_quad == 6 ? 3 : 5;
    if (d->term_offset[0] != 0) return fail("ds_ecp_create: term_offset must begin at 0");
    for (int sp = 0; sp < d->n_species; ++sp) {
        const int nl = d->n_l[sp];
        if (nl < 0 || nl > 4) return fail("ds_ecp_create: species %d has n_l = %d; n_l must be in 0..4", sp, nl);
        if (nl == 4) return fail("ds_ecp_create: species %d has n_l = 4: an l = 3 channel needs a quadrature rule of degree >= 6, which is not provided", sp);
        if (2 * (nl - 1) > degree)
            return fail("ds_ecp_create: species %d has n_l = %d: channels up to l = %d need a rule of degree %d, n_quad = %d is exact to degree %d",
                        sp, nl, nl - 1, 2 * (nl - 1), d->n_quad, degree);
        if (!std::isfinite(d->r_cut_loc[sp]) || !std::isfinite(d->r_cut_nl[sp]) || d->r_cut_loc[sp] < 0.0 || d->r_cut_nl[sp] < 0.0)
            return fail("ds_ecp_create: species %d has a cutoff that is negative or not finite", sp);
        for (int j = 0; j < ds::ECP_SLOTS; ++j) {
            const int slot = sp * ds::ECP_SLOTS + j, k0 = d->term_offset[slot], k1 = d->term_offset[slot + 1];
            if (k1 < k0) return fail("ds_ecp_create: term_offset decreases at slot %d", slot);
            if (k1 - k0 > ds::ECP_MAX_TERMS)
                return fail("ds_ecp_create: species %d, function %d has %d terms; at most %d terms are provided", sp, j, k1 - k0, ds::ECP_MAX_TERMS);
            if (k1 > k0 && (!d->term_n || !d->term_zeta || !d->term_c)) return fail("ds_ecp_create: null term table");
            for (int k = k0; k < k1; ++k) {
                if (d->term_n[k] < 0 || d->term_n[k] > 4)
                    return fail("ds_ecp_create: species %d, function %d, term %d has n_k = %d; n_k must be in 0..4", sp, j, k - k0, d->term_n[k]);
                if (!std::isfinite(d->term_zeta[k]) || !std::isfinite(d->term_c[k]))
                    return fail("ds_ecp_create: species %d, function %d, term %d is not finite", sp, j, k - k0);
            }
        }
    }
    for (int I = 0; I < d->n_atoms; ++I) {
        const int sp = d->atom_species[I];
        if (sp < 0 || sp >= d->n_species) return fail("ds_ecp_create: atom %d names species %d of %d", I, sp, d->n_species);
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(d->atoms[3 * I + c])) return fail("ds_ecp_create: atoms[%d][%d] is not finite", I, c);
        const double rc = std::max(d->r_cut_loc[sp], d->n_l[sp] > 0 ? d->r_cut_nl[sp] : 0.0);
        if (rc > 0.5 * hmin)
            return fail("ds_ecp_create: atom %d (species %d) has the cutoff %.6f Bohr; the limit is %.6f Bohr, half the smallest height of the simulation cell",
                        I, sp, rc, 0.5 * hmin);
    }
    return 0;
}

// Drift-biased importance sampling (qmc.importance_update, qmc.py:83-150, as make_mcmc_step drives it): per move the drift
// grad log|psi| at x1, the proposal x2 = wrap(x1 + w N + w^2 limdrift(g1)), (log|psi|, drift) at x2, and the selection with
// the forward / reverse proposal densities -- the kernels of ds_mh_propose_ex / ds_mh_accept_ex (mode 2), enqueued back to back.
template <typename T>
int mcmc_importance_impl(ds_system* s, const void* params, void* x_, void* lp_, int64_t B, int steps, double width, uint64_t seed,
                         uint64_t offset, const void* normals_, const void* uniforms_, int lp_valid, void* n_accept, void* ws,
                         int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const size_t n3 = (size_t)B * 3 * S.N, ne = (size_t)B * S.N;
    T* x = (T*)x_; T* lp = (T*)lp_;
    McmcScratch<T> m;
    if (int rc = mcmc_begin<T>(s, "ds_mcmc_step_importance", params, x, lp, B, lp_valid, ws, ws_bytes, st, &m)) return rc;
    const ds::PhiloxKey key{seed, offset};
    const dim3 ge((unsigned)((n3 + 255) / 256)), gn((unsigned)((std::max<size_t>(ne, (size_t)B) + 255) / 256)), blk(256);
    for (int i = 0; i < steps; ++i) {
        if (int rc = logpsi_grad_forward(s, params, x, B, m.LA2, nullptr, m.GC, m.wsv, m.wsv_bytes, st)) return rc;          // :111
        hipLaunchKernelGGL((ds::k_real_part<T>), ge, blk, 0, st, m.GC, n3, m.G1);
        const T* nz = normals_ ? (const T*)normals_ + (size_t)i * n3 : m.NZ;
        const T* un = uniforms_ ? (const T*)uniforms_ + (size_t)i * B : m.UN;
        if (!normals_) hipLaunchKernelGGL((ds::k_philox_noise<T>), gn, blk, 0, st, key, (unsigned long long)i, ne, (long)B, m.NZ, m.UN);
        hipLaunchKernelGGL((ds::k_max_norm3<T>), dim3(1), dim3(1024), 0, st, m.G1, ne, m.SCR);
        hipLaunchKernelGGL((ds::k_mh_propose_ex<T>), dim3((unsigned)((ne + 255) / 256)), blk, 0, st, S.sim_a, S.sim_ainv, 2, x, nz, (T)width,
                           m.G1, 0, ne, m.X2, m.SCR);                                                                      // :112-115
        if (int rc = logpsi_grad_forward(s, params, m.X2, B, m.LA2, nullptr, m.GC, m.wsv, m.wsv_bytes, st)) return rc;         // :118
        hipLaunchKernelGGL((ds::k_real_part<T>), ge, blk, 0, st, m.GC, n3, m.G2);
        hipLaunchKernelGGL((ds::k_max_norm3<T>), dim3(1), dim3(1024), 0, st, m.G2, ne, m.SCR + 1);
        hipLaunchKernelGGL((ds::k_mh_accept_ex<T>), dim3((unsigned)B), dim3(64), 0, st, 2, x, lp, m.X2, m.LA2, un, nz, (T)width, m.G1, m.G2, 0, S.N,
                           (T*)n_accept, m.SCR);                                                                       // :119-137
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// Asymmetric all-electron proposal (mh_update with atoms=, qmc.py:197-215): step width per electron = width x harmonic mean of its
// nuclear distances, forward / reverse proposal densities in the ratio -- the kernels of ds_mh_propose_ex / ds_mh_accept_ex (mode 1).
template <typename T>
int mcmc_asymmetric_impl(ds_system* s, const void* params, void* x_, void* lp_, int64_t B, int steps, double width, const void* atoms,
                         int n_atoms, uint64_t seed, uint64_t offset, const void* normals_, const void* uniforms_, int lp_valid,
                         void* n_accept, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const size_t n3 = (size_t)B * 3 * S.N, ne = (size_t)B * S.N;
    T* x = (T*)x_; T* lp = (T*)lp_;
    McmcScratch<T> m;
    if (int rc = mcmc_begin<T>(s, "ds_mcmc_step_asymmetric", params, x, lp, B, lp_valid, ws, ws_bytes, st, &m)) return rc;
    const ds::PhiloxKey key{seed, offset};
    const dim3 gn((unsigned)((std::max<size_t>(ne, (size_t)B) + 255) / 256)), blk(256);
    for (int i = 0; i < steps; ++i) {
        const T* nz = normals_ ? (const T*)normals_ + (size_t)i * n3 : m.NZ;
        const T* un = uniforms_ ? (const T*)uniforms_ + (size_t)i * B : m.UN;
        if (!normals_) hipLaunchKernelGGL((ds::k_philox_noise<T>), gn, blk, 0, st, key, (unsigned long long)i, ne, (long)B, m.NZ, m.UN);
        hipLaunchKernelGGL((ds::k_mh_propose_ex<T>), dim3((unsigned)((ne + 255) / 256)), blk, 0, st, S.sim_a, S.sim_ainv, 1, x, nz, (T)width,
                           (const T*)atoms, n_atoms, ne, m.X2, (const T*)nullptr);                                     // :200-204
        if (int rc = logpsi_forward(s, params, m.X2, B, m.LA2, nullptr, m.wsv, m.wsv_bytes, st)) return rc;                  // :205
        hipLaunchKernelGGL((ds::k_mh_accept_ex<T>), dim3((unsigned)B), dim3(64), 0, st, 1, x, lp, m.X2, m.LA2, un, (const T*)nullptr, (T)width,
                           (const T*)atoms, (const T*)nullptr, n_atoms, S.N, (T*)n_accept, (const T*)nullptr);       // :208-222
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ single proposal / selection steps and the batch statistics
template <typename T> void mh_propose(ds_system* s, const void* x1, const void* normal, double width, size_t ne, void* x2, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    hipLaunchKernelGGL((ds::k_mh_propose<T>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, S.sim_a, S.sim_ainv, (const T*)x1, (const T*)normal,
                       (T)width, ne, (T*)x2);
}

template <typename T>
void mh_accept(ds_system* s, void* x1, void* lp1, const void* x2, const void* lp2, const void* uniform, int64_t B, void* n_accept, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_mh_accept<T>), dim3((unsigned)B), dim3(64), 0, st, (T*)x1, (T*)lp1, (const T*)x2, (const T*)lp2, (const T*)uniform,
                       3 * dev<T>(s).N, (T*)n_accept);
}

template <typename T>
void mh_propose_ex(ds_system* s, int mode, const void* x1, const void* normal, double width, const void* aux, int n_aux, size_t ne, void* x2,
                   void* scratch, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    if (mode == 2) hipLaunchKernelGGL((ds::k_max_norm3<T>), dim3(1), dim3(1024), 0, st, (const T*)aux, ne, (T*)scratch);
    hipLaunchKernelGGL((ds::k_mh_propose_ex<T>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, S.sim_a, S.sim_ainv, mode, (const T*)x1,
                       (const T*)normal, (T)width, (const T*)aux, n_aux, ne, (T*)x2, (const T*)scratch);
}

template <typename T>
void mh_accept_ex(ds_system* s, int mode, void* x1, void* lp1, const void* x2, const void* logabs2, const void* uniform, const void* normal,
                  double width, const void* aux1, const void* aux2, int n_aux, size_t ne, int64_t B, void* n_accept, void* scratch,
                  hipStream_t st) {
    if (mode == 2) hipLaunchKernelGGL((ds::k_max_norm3<T>), dim3(1), dim3(1024), 0, st, (const T*)aux2, ne, (T*)scratch + 1);
    hipLaunchKernelGGL((ds::k_mh_accept_ex<T>), dim3((unsigned)B), dim3(64), 0, st, mode, (T*)x1, (T*)lp1, (const T*)x2, (const T*)logabs2,
                       (const T*)uniform, (const T*)normal, (T)width, (const T*)aux1, (const T*)aux2, n_aux, dev<T>(s).N, (T*)n_accept,
                       (const T*)scratch);
}

template <typename T> void energy_stats(const void* ke, const void* ewald, int64_t B, double* out_stats, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_energy_stats<T>), dim3(1), dim3(256), 0, st, (const T*)ke, (const T*)ewald, (long)B, out_stats);
}

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

int ds_mh_propose(ds_system* s, const void* x1, const void* normal, double width, int64_t B, void* x2, void* stream) {
    if (!s || !x1 || !normal || !x2) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t ne = (size_t)B * s->sd.N;
    DS_BY_DTYPE(s->dtype, mh_propose, s, x1, normal, width, ne, x2, st);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_mh_accept(ds_system* s, void* x1, void* lp1, const void* x2, const void* lp2, const void* uniform, int64_t B, void* n_accept,
                 void* stream) {
    if (!s || !x1 || !lp1 || !x2 || !lp2 || !uniform || !n_accept) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    DS_BY_DTYPE(s->dtype, mh_accept, s, x1, lp1, x2, lp2, uniform, B, n_accept, st);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_mh_propose_ex(ds_system* s, int mode, const void* x1, const void* normal, double width, const void* aux, int n_aux, int64_t B,
                     void* x2, void* scratch, void* stream) {
    if (!s || !x1 || !normal || !aux || !x2) return fail("null argument");
    if (mode == 2 && !scratch) return fail("the drift move needs a 2-element device scratch (batch maxima of the drift)");
    if (mode != 1 && mode != 2) return fail("mode must be 1 (asymmetric) or 2 (drift)");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t ne = (size_t)B * s->sd.N;
    DS_BY_DTYPE(s->dtype, mh_propose_ex, s, mode, x1, normal, width, aux, n_aux, ne, x2, scratch, st);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_mh_accept_ex(ds_system* s, int mode, void* x1, void* lp1, const void* x2, const void* logabs2, const void* uniform,
                    const void* normal, double width, const void* aux1, const void* aux2, int n_aux, int64_t B, void* n_accept,
                    void* scratch, void* stream) {
    if (!s || !x1 || !lp1 || !x2 || !logabs2 || !uniform || !aux1 || !n_accept) return fail("null argument");
    if (mode != 1 && mode != 2) return fail("mode must be 1 (asymmetric) or 2 (drift)");
    if (mode == 2 && (!aux2 || !normal || !scratch)) return fail("the drift move needs both gradients, the normal deviates and the scratch of ds_mh_propose_ex");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t ne = (size_t)B * s->sd.N;
    DS_BY_DTYPE(s->dtype, mh_accept_ex, s, mode, x1, lp1, x2, logabs2, uniform, normal, width, aux1, aux2, n_aux, ne, B, n_accept, scratch,
                st);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t ds_mcmc_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s) return -1;
    return ds_workspace_bytes(s, B) + (int64_t)mcmc_scratch_bytes(s, std::max<int64_t>(B, 1));
}

int ds_mcmc_step(ds_system* s, const void* params, void* x, void* lp, int64_t B, int steps, double width, uint64_t philox_seed,
                 uint64_t philox_offset, const void* normals, const void* uniforms, int lp_valid, void* n_accept, void* ws,
                 int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !lp || !n_accept || !ws) return fail("null argument");
    if ((normals == nullptr) != (uniforms == nullptr)) return fail("normals and uniforms must be given together (or both NULL)");
    if (steps < 0) return fail("steps must be >= 0");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, mcmc_step_impl, s, params, x, lp, B, steps, width, philox_seed, philox_offset, normals, uniforms, lp_valid,
                       n_accept, ws, ws_bytes, st);
}

int ds_mcmc_step_one_electron(ds_system* s, const void* params, void* x, void* lp, int64_t B, int moves, int first_electron,
                              double width, uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms,
                              int lp_valid, void* n_accept, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !lp || !n_accept || !ws) return fail("null argument");
    if ((normals == nullptr) != (uniforms == nullptr)) return fail("normals and uniforms must be given together (or both NULL)");
    if (moves < 0 || first_electron < 0) return fail("moves and first_electron must be >= 0");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, mcmc_step_impl, s, params, x, lp, B, moves, width, philox_seed, philox_offset, normals, uniforms, lp_valid,
                       n_accept, ws, ws_bytes, st, first_electron);
}

int ds_mcmc_step_asymmetric(ds_system* s, const void* params, void* x, void* lp, int64_t B, int steps, double width, const void* atoms,
                            int n_atoms, uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms,
                            int lp_valid, void* n_accept, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !lp || !n_accept || !ws || !atoms) return fail("null argument");
    if ((normals == nullptr) != (uniforms == nullptr)) return fail("normals and uniforms must be given together (or both NULL)");
    if (steps < 0 || n_atoms < 1) return fail("steps must be >= 0 and n_atoms >= 1");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, mcmc_asymmetric_impl, s, params, x, lp, B, steps, width, atoms, n_atoms, philox_seed, philox_offset,
                       normals, uniforms, lp_valid, n_accept, ws, ws_bytes, st);
}

int ds_mcmc_step_importance(ds_system* s, const void* params, void* x, void* lp, int64_t B, int steps, double width,
                            uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms, int lp_valid,
                            void* n_accept, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !lp || !n_accept || !ws) return fail("null argument");
    if ((normals == nullptr) != (uniforms == nullptr)) return fail("normals and uniforms must be given together (or both NULL)");
    if (steps < 0) return fail("steps must be >= 0");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, mcmc_importance_impl, s, params, x, lp, B, steps, width, philox_seed, philox_offset, normals, uniforms,
                       lp_valid, n_accept, ws, ws_bytes, st);
}

int64_t ds_one_body_workspace_bytes(const ds_system* s, int64_t B, int n_samples) {
    if (!s || B < 1 || n_samples < 1) return -1;
    // as many groups per chunk as ds_workspace_bytes gives the value chain of B * n_samples walkers
    const int64_t esz = s->dtype == 0 ? 8 : 4, total = B * (int64_t)n_samples;
    const int64_t budget = workspace_budget();
    const int64_t fixed = onebody_bytes(s, B, 0), per = onebody_bytes(s, B, 1) - fixed;
    const int64_t ng = std::min(groups_per_pass(total, esz, PassSize{0, (size_t)(per / esz)}, budget), OB_MAX_GROUPS);
    return onebody_bytes(s, B, ng);
}

int ds_one_body_ratios(ds_system* s, const void* params, const void* x, int64_t B, int n_samples, int first_electron,
                       uint64_t philox_seed, uint64_t philox_offset, const void* shifts, const double* kvec, int n_k, double* nk_sums,
                       void* out_ratio, void* out_shift, int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws) return fail("null argument");
    if (B < 1) return fail("ds_one_body_ratios: B must be >= 1 (got %lld)", (long long)B);
    if (n_samples < 1) return fail("ds_one_body_ratios: n_samples must be >= 1 (got %d)", n_samples);
    if (first_electron < 0 || first_electron >= s->sd.N)
        return fail("ds_one_body_ratios: first_electron must be in 0..%d (got %d)", s->sd.N - 1, first_electron);
    if (n_k < 0 || n_k > ds::OB_MAX_K) return fail("ds_one_body_ratios: n_k must be in 0..%d (got %d)", ds::OB_MAX_K, n_k);
    if (n_k > 0 && (!kvec || !nk_sums)) return fail("ds_one_body_ratios: n_k = %d needs kvec and nk_sums", n_k);
    if (n_k == 0 && !out_ratio) return fail("ds_one_body_ratios: n_k is 0 and out_ratio is null, nothing to write");
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, one_body_impl, s, params, x, B, n_samples, first_electron, philox_seed, philox_offset, shifts, kvec, n_k,
                       nk_sums, out_ratio, out_shift, n_bad, ws, ws_bytes, st);
}

int64_t ds_spin_exchange_workspace_bytes(const ds_system* s, int64_t B, int n_pairs) {
    if (!s || B < 1 || n_pairs < 1) return -1;
    // as many groups per chunk as ds_workspace_bytes gives the value chain of B * n_pairs walkers
    const int64_t esz = s->dtype == 0 ? 8 : 4, total = B * (int64_t)n_pairs;
    const int64_t budget = workspace_budget();
    const int64_t fixed = spin_bytes(s, B, n_pairs, 0), per = spin_bytes(s, B, n_pairs, 1) - fixed;
    const int64_t ng = std::min(groups_per_pass(total, esz, PassSize{0, (size_t)(per / esz)}, budget), OB_MAX_GROUPS);
    return spin_bytes(s, B, n_pairs, ng);
}

int ds_spin_exchange_ratios(ds_system* s, const void* params, const void* x, int64_t B, int n_pairs, int first_pair, double* sums,
                            void* out_ratio, double* out_walker, int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws) return fail("null argument");
    if (B < 1) return fail("ds_spin_exchange_ratios: B must be >= 1 (got %lld)", (long long)B);
    const int64_t P = (int64_t)s->sd.n_up * s->sd.n_dn;
    if (P == 0)
        return fail("ds_spin_exchange_ratios: the cell has no pair of opposite spins (n_up = %d, n_dn = %d): S^2 = S_z (S_z + 1) exactly",
                    s->sd.n_up, s->sd.n_dn);
    if (n_pairs < 1) return fail("ds_spin_exchange_ratios: n_pairs must be >= 1 (got %d)", n_pairs);
    if (first_pair < 0 || first_pair >= P)
        return fail("ds_spin_exchange_ratios: first_pair must be in 0..%lld (got %d)", (long long)P - 1, first_pair);
    if (!sums && !out_ratio && !out_walker)
        return fail("ds_spin_exchange_ratios: sums, out_ratio and out_walker are all null, nothing to write");
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, spin_exchange_impl, s, params, x, B, n_pairs, first_pair, sums, out_ratio, out_walker, n_bad, ws, ws_bytes,
                       st);
}

void ds_ecp_destroy(ds_ecp* e) {
    if (!e) return;
    for (void* d : e->dev) (void)hipFree(d);
    delete e;
}

int ds_ecp_create(const ds_ecp_desc* d, ds_ecp** out) {
    if (!d || !out) return fail("null argument");
    *out = nullptr;
    if (int rc = ecp_validate(d)) return rc;
    ds_ecp* h = new ds_ecp();
    ds::EcpDev& E = h->D;
    for (int i = 0; i < 9; ++i) E.a[i] = d->a[i];
    inv3(d->a, E.ainv);
    E.n_atoms = d->n_atoms; E.n_species = d->n_species; E.n_quad = d->n_quad;
    for (double& v : E.quad) v = 0.0;
    if (d->n_quad == 6) {
        for (int q = 0; q < 6; ++q) E.quad[3 * q + q / 2] = q % 2 ? -1.0 : 1.0;              // +x, -x, +y, -y, +z, -z
    } else {
        const double phi = (1.0 + std::sqrt(5.0)) / 2.0, n = std::sqrt(1.0 + phi * phi);
        const double sg[4][2] = {{1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
        for (int j = 0; j < 4; ++j) {
            const double s1 = sg[j][0], s2 = sg[j][1];
            const double pts[3][3] = {{0.0, s1, s2 * phi}, {s1, s2 * phi, 0.0}, {s2 * phi, 0.0, s1}};
            for (int f = 0; f < 3; ++f)
                for (int c = 0; c < 3; ++c) E.quad[3 * (4 * f + j) + c] = pts[f][c] / n;
        }
    }
    const int n_slots = d->n_species * ds::ECP_SLOTS, n_terms = d->term_offset[n_slots];
    std::vector<double> atoms(d->atoms, d->atoms + 3 * d->n_atoms), rcl(d->r_cut_loc, d->r_cut_loc + d->n_species),
        rcn(d->r_cut_nl, d->r_cut_nl + d->n_species), tz, tc;
    std::vector<int> asp(d->atom_species, d->atom_species + d->n_atoms), nl(d->n_l, d->n_l + d->n_species),
        toff(d->term_offset, d->term_offset + n_slots + 1), tn;
    if (n_terms > 0) {
        tn.assign(d->term_n, d->term_n + n_terms); tz.assign(d->term_zeta, d->term_zeta + n_terms); tc.assign(d->term_c, d->term_c + n_terms);
    }
    const int rc = ecp_upload(h, atoms, &E.atoms) || ecp_upload(h, asp, &E.atom_species) || ecp_upload(h, nl, &E.n_l) ||
                   ecp_upload(h, rcl, &E.rc_loc) || ecp_upload(h, rcn, &E.rc_nl) || ecp_upload(h, toff, &E.term_off) ||
                   ecp_upload(h, tn, &E.term_n) || ecp_upload(h, tz, &E.term_z) || ecp_upload(h, tc, &E.term_c);
    if (rc) { ds_ecp_destroy(h); return 1; }
    *out = h;
    return 0;
}

int64_t ds_ecp_workspace_bytes(const ds_system* s, const ds_ecp* e, int64_t B, int64_t pair_capacity) {
    if (!s || !e) { fail("null argument"); return -1; }
    if (ecp_check(s, e, B, pair_capacity)) return -1;
    const int nq = e->D.n_quad;
    return ecp_bytes(s, B, pair_capacity, nq, ecp_default_groups(s, B, pair_capacity, nq));
}

int ds_ecp_energy(ds_system* s, const ds_ecp* e, const void* params, const void* x, int64_t B, uint64_t philox_seed, uint64_t philox_offset,
                  const double* rotations, int64_t pair_capacity, double* out_energy, int64_t* out_pairs, void* out_ratio,
                  double* out_rotation, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !e || !params || !x || !ws) return fail("null argument");
    if (!out_energy) return fail("ds_ecp_energy: out_energy is null, nothing to write");
    if (int rc = ecp_check(s, e, B, pair_capacity)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ecp_energy_forward(s, e, params, x, B, philox_seed, philox_offset, rotations, pair_capacity, out_energy, out_pairs, out_ratio,
                              out_rotation, ws, ws_bytes, st, nullptr, nullptr);
}

int64_t ds_ecp_forces_workspace_bytes(const ds_system* s, const ds_ecp* e, int64_t B, int64_t pair_capacity) {
    if (!s || !e) { fail("null argument"); return -1; }
    if (ecp_check(s, e, B, pair_capacity)) return -1;
    // as many groups per chunk as ds_workspace_bytes gives the forward-Laplacian chain of pair_capacity * n_quad walkers
    const int nq = e->D.n_quad, A = e->D.n_atoms;
    const int64_t esz = s->dtype == 0 ? 8 : 4, total = std::max(pair_capacity * nq, B);
    const int64_t fixed = ecp_force_bytes(s, B, A, pair_capacity, nq, 0), per = ecp_force_bytes(s, B, A, pair_capacity, nq, 1) - fixed;
    const int64_t ng = std::min(groups_per_pass(total, esz, PassSize{0, (size_t)(per / esz)}, workspace_budget()), OB_MAX_GROUPS);
    return ecp_force_bytes(s, B, A, pair_capacity, nq, ng);
}

int ds_ecp_forces(ds_system* s, const ds_ecp* e, const void* params, const void* x, int64_t B, uint64_t philox_seed, uint64_t philox_offset,
                  const double* rotations, int64_t pair_capacity, const double* base, double* out_force, double* sums, int64_t* n_bad,
                  int64_t* out_pairs, double* out_rotation, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !e || !params || !x || !ws) return fail("null argument");
    if (!out_force && !sums) return fail("ds_ecp_forces: out_force and sums are both null, nothing to write");
    if (int rc = ecp_check(s, e, B, pair_capacity)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, ecp_forces_impl, s, e, params, x, B, philox_seed, philox_offset, rotations, pair_capacity, base, out_force,
                       sums, n_bad, out_pairs, out_rotation, ws, ws_bytes, st);
}

int ds_energy_stats(ds_system* s, const void* ke, const void* ewald, int64_t B, double* out_stats, void* stream) {
    if (!s || !ke || !ewald || !out_stats) return fail("null argument");
    hipStream_t st = (hipStream_t)stream;
    DS_BY_DTYPE(s->dtype, energy_stats, ke, ewald, B, out_stats, st);
    HIP_OK(hipGetLastError());
    return 0;
}

void ds_philox_host(uint64_t seed, uint64_t offset, uint64_t step, uint64_t index, int stream_id, uint32_t out[4]) {
    const uint64_t off = offset + step;
    const ds::Philox4 r = ds::philox4x32_10((unsigned)index, (unsigned)(index >> 32), (unsigned)off,
                                            ((unsigned)(off >> 32) & 0x3fffffffu) | ((unsigned)stream_id << 30), (unsigned)seed,
                                            (unsigned)(seed >> 32));
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}

}  // extern "C"
