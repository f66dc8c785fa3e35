// ds_dmc.hip -- fixed-phase diffusion Monte Carlo (ds_dmc.h): the workspace, the fused block of steps and the comb alone.
#include "ds_host.h"
#include "ds_dmc.h"

namespace ds {
namespace host {

// Workspace of the comb for B walkers of n3 coordinates.  In 8-byte elements (2 elements each: room in either element size): the
// running sums inside the chunks (B,), the chunk sums and offsets, (W, W / B, run), the gathered E_L; as ints the parents and the
// per-workgroup counts of distinct parents.  Then the second buffer of the walker rows.
template <typename T> struct CombWs {
    double *R, *CSUM, *OFF, *TOT, *BEL;
    int *PAR, *CNT;
    T *BX, *BDR, *BLA, *BPH;
};
inline size_t comb_chunks(int64_t B) { return (size_t)((B + ds::DMC_CHUNK - 1) / ds::DMC_CHUNK); }
inline size_t comb_blocks(int64_t B) { return (size_t)((B + 255) / 256); }
template <typename T> CombWs<T> carve_comb(Arena<T>& a, int64_t B, int n3) {
    const size_t b = (size_t)B, nc = comb_chunks(B);
    CombWs<T> w{};
    a.align(2);
    w.R = (double*)a.take(2 * b); w.CSUM = (double*)a.take(2 * nc); w.OFF = (double*)a.take(2 * nc); w.TOT = (double*)a.take(2 * 4);
    w.BEL = (double*)a.take(2 * b);
    w.PAR = (int*)a.take(2 * ((b + 1) / 2)); w.CNT = (int*)a.take(2 * ((comb_blocks(B) + 1) / 2));
    w.BX = a.take(b * n3); w.BDR = a.take(b * n3); w.BLA = a.take(b); w.BPH = a.take(2 * b);
    return w;
}

// Workspace of ds_dmc_step: the comb's, then the proposal x' (B,3N), its complex gradient (B,3N,2), the noise that was used
// (B,3N), log|psi'|, phase', ke', the Ewald triple; in 8-byte elements the acceptance probabilities and the stats partials, as ints
// the flags; behind them, on a 64-element border, the energy chain's buffers for nw walkers.
template <typename T> struct DmcWs {
    CombWs<T> comb;
    T *X2, *GC, *NZ, *LA2, *PH2, *KE2, *EW3;
    double *PACC, *PART;
    int* FLAGS;
    void* wsc; int64_t wsc_bytes;
};
template <typename T> DmcWs<T> carve_dmc(const ds_system* s, Arena<T>& a, int64_t B, int64_t nw) {
    const size_t b = (size_t)B, n3 = 3 * (size_t)s->sd.N;
    DmcWs<T> w{};
    w.comb = carve_comb<T>(a, B, (int)n3);
    a.align(2);
    w.PACC = (double*)a.take(2 * b);
    w.PART = (double*)a.take(2 * (size_t)((B + ds::DMC_GROUP - 1) / ds::DMC_GROUP) * (ds::DMC_ROW - 1));
    w.FLAGS = (int*)a.take(2 * ((b + 1) / 2));
    w.X2 = a.take(b * n3); w.GC = a.take(2 * b * n3); w.NZ = a.take(b * n3);
    w.LA2 = a.take(b); w.PH2 = a.take(2 * b); w.KE2 = a.take(2 * b); w.EW3 = a.take(3 * b);
    a.align(64);
    w.wsc = a.take(s->ws.per_walker * (size_t)nw);
    w.wsc_bytes = (int64_t)(s->ws.per_walker * (size_t)nw * sizeof(T));
    return w;
}
inline int64_t dmc_bytes(const ds_system* s, int64_t B, int64_t nw) {
    return (int64_t)measure([&](Arena<double>& a) { carve_dmc<double>(s, a, B, nw); }) * (s->dtype == 0 ? 8 : 4);
}
inline int64_t comb_bytes(int dtype, int64_t B, int n3) {
    return (int64_t)measure([&](Arena<double>& a) { carve_comb<double>(a, B, n3); }) * (dtype == 0 ? 8 : 4);
}

// the comb on the six state arrays: five launches, no host synchronisation.  xi_dev != nullptr: xi is read from the device.
template <typename T>
void launch_comb(const CombWs<T>& c, int64_t B, int n3, double xi, const double* xi_dev, T* x, T* logabs, T* phase, T* drift, double* eloc,
                 double* weight, int* out_parents, double* stat_distinct, hipStream_t st) {
    const int nc = (int)comb_chunks(B), nb = (int)comb_blocks(B);
    const dim3 gw((unsigned)((B + ds::DMC_WAVES - 1) / ds::DMC_WAVES)), bw(64 * ds::DMC_WAVES);
    hipLaunchKernelGGL(ds::k_dmc_scan_chunks, dim3((unsigned)nc), dim3(64), 0, st, (long long)B, (const double*)weight, c.R, c.CSUM);
    hipLaunchKernelGGL(ds::k_dmc_scan_offsets, dim3(1), dim3(256), 0, st, (long long)B, nc, (const double*)c.CSUM, (const double*)c.R, c.OFF, c.TOT);
    hipLaunchKernelGGL(ds::k_dmc_select, dim3((unsigned)nb), dim3(256), 0, st, (long long)B, xi, xi_dev, (const double*)c.R,
                       (const double*)c.OFF, (const double*)c.TOT, c.PAR, c.CNT, out_parents);
    hipLaunchKernelGGL((ds::k_dmc_gather<T>), gw, bw, 0, st, (long long)B, n3, (const double*)c.TOT, (const int*)c.PAR, (const T*)x,
                       (const T*)logabs, (const T*)phase, (const T*)drift, (const double*)eloc, c.BX, c.BLA, c.BPH, c.BDR, c.BEL);
    hipLaunchKernelGGL((ds::k_dmc_copy_back<T>), gw, bw, 0, st, (long long)B, n3, (const double*)c.TOT, (const int*)c.CNT, nb,
                       (const T*)c.BX, (const T*)c.BLA, (const T*)c.BPH, (const T*)c.BDR, (const double*)c.BEL, x, logabs, phase, drift,
                       eloc, weight, stat_distinct);
}

struct DmcCall {
    int64_t B; int steps; double tau, tau_eff, e_trial, e_ref, e_cut; int node_mode, branch_every;
    uint64_t seed, offset; const void *normals, *uniforms; const double* comb_uniforms; int state_valid;
    double* out_stats; int* out_parents;
};

template <typename T>
int dmc_step_impl(ds_system* s, const void* params, void* x_, void* logabs_, void* phase_, void* drift_, double* eloc, double* weight,
                  const DmcCall& q, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int64_t B = q.B, esz = (int64_t)sizeof(T);
    const int n3 = 3 * S.N;
    T *x = (T*)x_, *logabs = (T*)logabs_, *phase = (T*)phase_, *drift = (T*)drift_;
    // the chain's chunk follows from the workspace (the layout is linear in nw up to its alignment pad)
    const int64_t head = dmc_bytes(s, B, 0);
    int64_t nw = std::min<int64_t>({(ws_bytes - head) / ((int64_t)s->ws.per_walker * esz), 65535, B});
    while (nw >= 1 && dmc_bytes(s, B, nw) > ws_bytes) --nw;
    if (nw < 1)
        return fail("workspace too small for ds_dmc_step: %lld bytes < %lld for one chain chunk of one walker (see ds_dmc_workspace_bytes)",
                    (long long)ws_bytes, (long long)dmc_bytes(s, B, 1));
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const DmcWs<T> w = carve_dmc<T>(s, a, B, nw);
    if (!a.ok) return carve_fail("DMC step");
    const size_t ne = (size_t)B * S.N;
    const dim3 gw((unsigned)((B + ds::DMC_WAVES - 1) / ds::DMC_WAVES)), bw(64 * ds::DMC_WAVES);
    const int64_t ngroups = (B + ds::DMC_GROUP - 1) / ds::DMC_GROUP;
    if (!q.state_valid) {
        if (int rc = energy_grad_forward(s, params, x, B, w.KE2, w.EW3, logabs, phase, w.GC, w.wsc, w.wsc_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_dmc_init<T>), gw, bw, 0, st, (long long)B, n3, (const T*)w.GC, (const T*)w.KE2, (const T*)w.EW3,
                           (const T*)logabs, drift, eloc, weight);
    }
    ds::DmcArgs A{q.tau, std::sqrt(q.tau), q.tau_eff, q.e_trial, q.e_ref, q.e_cut, q.node_mode, S.N, (long long)B};
    const ds::PhiloxKey key{q.seed, q.offset};
    const T* normals = (const T*)q.normals; const T* uniforms = (const T*)q.uniforms;
    for (int i = 0; i < q.steps; ++i) {
        const T* nz = normals ? normals + (size_t)i * B * n3 : (const T*)nullptr;
        hipLaunchKernelGGL((ds::k_dmc_propose<T>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, S.sim_a, S.sim_ainv, (const T*)x,
                           (const T*)drift, nz, key, (unsigned long long)i, (T)q.tau, (T)A.sqrt_tau, ne, w.X2, w.NZ);
        if (int rc = energy_grad_forward(s, params, w.X2, B, w.KE2, w.EW3, w.LA2, w.PH2, w.GC, w.wsc, w.wsc_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_dmc_accept<T>), gw, bw, 0, st, A, x, logabs, phase, drift, eloc, weight, (const T*)w.X2, (const T*)w.LA2,
                           (const T*)w.PH2, (const T*)w.GC, (const T*)w.KE2, (const T*)w.EW3, nz ? nz : (const T*)w.NZ,
                           uniforms ? uniforms + (size_t)i * B : (const T*)nullptr, key, (unsigned long long)i, w.PACC, w.FLAGS);
        double* row = q.out_stats + (size_t)i * ds::DMC_ROW;
        hipLaunchKernelGGL(ds::k_dmc_stats, dim3((unsigned)ngroups), dim3(ds::DMC_GROUP), 0, st, (long long)B, (const double*)weight,
                           (const double*)eloc, (const double*)w.PACC, (const int*)w.FLAGS, w.PART);
        hipLaunchKernelGGL(ds::k_dmc_stats_final, dim3(1), dim3(64), 0, st, (const double*)w.PART, (long long)ngroups, (long long)B, row);
        int* par = q.out_parents ? q.out_parents + (size_t)i * B : nullptr;
        if (q.branch_every > 0 && (i + 1) % q.branch_every == 0) {
            double xi = 0.0;
            if (!q.comb_uniforms) {                       // stream 2 at index B, one past the walkers
                uint32_t r[4];
                ds_philox_host(q.seed, q.offset, (uint64_t)i, (uint64_t)B, 2, r);
                xi = ds::u53_co(r[0], r[1]);
            }
            launch_comb<T>(w.comb, B, n3, xi, q.comb_uniforms ? q.comb_uniforms + i : nullptr, x, logabs, phase, drift, eloc, weight, par,
                           row + ds::DMC_ROW - 1, st);
        } else if (par) {
            hipLaunchKernelGGL(ds::k_dmc_identity, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (long long)B, par);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int dmc_branch_impl(int n_elec, int64_t B, double xi, void* x, void* logabs, void* phase, void* drift, double* eloc, double* weight,
                    int* out_parents, void* ws, int64_t ws_bytes, hipStream_t st) {
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const CombWs<T> c = carve_comb<T>(a, B, 3 * n_elec);
    if (!a.ok) return carve_fail("DMC comb");
    launch_comb<T>(c, B, 3 * n_elec, xi, nullptr, (T*)x, (T*)logabs, (T*)phase, (T*)drift, eloc, weight, out_parents, nullptr, st);
    HIP_OK(hipGetLastError());
    return 0;
}

// the draws of a Philox-mode call as explicit-mode arrays (ds_dmc_noise)
template <typename T>
void dmc_noise(int n_elec, int64_t B, int steps, uint64_t seed, uint64_t offset, void* normals, void* uniforms, double* comb_uniforms,
               hipStream_t st) {
    const size_t ne = (size_t)B * n_elec, n = std::max<size_t>(ne, (size_t)B + 1);
    for (int i = 0; i < steps; ++i)
        hipLaunchKernelGGL((ds::k_dmc_noise<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ds::PhiloxKey{seed, offset},
                           (unsigned long long)i, ne, (long long)B, (T*)normals + (size_t)i * 3 * ne, (T*)uniforms + (size_t)i * B,
                           comb_uniforms + i);
}

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

int64_t ds_dmc_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s || B < 1 || B > ds::DMC_MAX_B) return -1;
    // the chain's share is what ds_workspace_bytes gives the energy chain of B walkers
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    int64_t chunk = std::min<int64_t>(B, s->chunk_cap);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, workspace_budget() / ((int64_t)s->ws.per_walker * esz)));
    return dmc_bytes(s, B, chunk);
}

int ds_dmc_step(ds_system* s, const void* params, void* x, void* logabs, void* phase, void* drift, double* eloc, double* weight, int64_t B,
                int steps, double tau, double tau_eff, double e_trial, double e_ref, double e_cut, int node_mode, int branch_every,
                uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms, const double* comb_uniforms,
                int state_valid, double* out_stats, int32_t* out_parents, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !ws) return fail("ds_dmc_step: null argument");
    if (!x || !logabs || !phase || !drift || !eloc || !weight) return fail("ds_dmc_step: null state pointer");
    if (!out_stats) return fail("ds_dmc_step: out_stats is null");
    if (B < 1 || B > ds::DMC_MAX_B) return fail("ds_dmc_step: B must be in 1..%lld (got %lld)", (long long)ds::DMC_MAX_B, (long long)B);
    if (steps < 1) return fail("ds_dmc_step: steps must be >= 1 (got %d)", steps);
    if (!std::isfinite(tau) || !std::isfinite(tau_eff) || !std::isfinite(e_trial) || !std::isfinite(e_ref) || !std::isfinite(e_cut))
        return fail("ds_dmc_step: tau, tau_eff, e_trial, e_ref and e_cut must be finite");
    if (!(tau > 0.0)) return fail("ds_dmc_step: tau must be > 0 (got %g)", tau);
    if (tau_eff < 0.0) return fail("ds_dmc_step: tau_eff must be >= 0 (got %g)", tau_eff);
    if (node_mode != 0 && node_mode != 1) return fail("ds_dmc_step: node_mode must be 0 (fixed phase) or 1 (fixed node) (got %d)", node_mode);
    if (branch_every < 0) return fail("ds_dmc_step: branch_every must be >= 0 (got %d)", branch_every);
    const int given = (normals ? 1 : 0) + (uniforms ? 1 : 0) + (comb_uniforms ? 1 : 0);
    if (given != 0 && given != 3) return fail("ds_dmc_step: normals, uniforms and comb_uniforms must be given together (or all NULL)");
    const DmcCall q{B, steps, tau, tau_eff, e_trial, e_ref, e_cut, node_mode, branch_every, philox_seed, philox_offset, normals, uniforms,
                    comb_uniforms, state_valid, out_stats, (int*)out_parents};
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, dmc_step_impl, s, params, x, logabs, phase, drift, eloc, weight, q, ws, ws_bytes, st);
}

int ds_dmc_noise(int dtype, int n_elec, int64_t B, int steps, uint64_t philox_seed, uint64_t philox_offset, void* normals, void* uniforms,
                 double* comb_uniforms, void* stream) {
    if (!normals || !uniforms || !comb_uniforms) return fail("ds_dmc_noise: null argument");
    if (n_elec < 1 || B < 1 || B > ds::DMC_MAX_B || steps < 1)
        return fail("ds_dmc_noise: n_elec, B and steps must be >= 1 and B <= %lld", (long long)ds::DMC_MAX_B);
    hipStream_t st = (hipStream_t)stream;
    DS_BY_DTYPE(dtype, dmc_noise, n_elec, B, steps, philox_seed, philox_offset, normals, uniforms, comb_uniforms, st);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t ds_dmc_branch_workspace_bytes(int dtype, int n_elec, int64_t B) {
    if (n_elec < 1 || B < 1 || B > ds::DMC_MAX_B) return -1;
    return comb_bytes(dtype, B, 3 * n_elec);
}

int ds_dmc_branch(int dtype, int n_elec, int64_t B, double xi, void* x, void* logabs, void* phase, void* drift, double* eloc, double* weight,
                  int32_t* out_parents, void* ws, int64_t ws_bytes, void* stream) {
    if (!x || !logabs || !phase || !drift || !eloc || !weight) return fail("ds_dmc_branch: null state pointer");
    if (!ws) return fail("ds_dmc_branch: null workspace");
    if (n_elec < 1) return fail("ds_dmc_branch: n_elec must be >= 1 (got %d)", n_elec);
    if (B < 1 || B > ds::DMC_MAX_B) return fail("ds_dmc_branch: B must be in 1..%lld (got %lld)", (long long)ds::DMC_MAX_B, (long long)B);
    if (!(xi >= 0.0 && xi < 1.0)) return fail("ds_dmc_branch: xi must be in [0, 1) (got %g)", xi);
    const int64_t need = comb_bytes(dtype, B, 3 * n_elec);
    if (ws_bytes < need)
        return fail("workspace too small for ds_dmc_branch: %lld bytes < %lld (see ds_dmc_branch_workspace_bytes)", (long long)ws_bytes,
                    (long long)need);
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(dtype, dmc_branch_impl, n_elec, B, xi, x, logabs, phase, drift, eloc, weight, (int*)out_parents, ws, ws_bytes, st);
}

}  // extern "C"
