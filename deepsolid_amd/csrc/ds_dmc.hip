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

// Workspace of ds_dmc_step_ecp: that of ds_dmc_step, then in 8-byte elements the pseudopotential triple at x' (B,3) and the partials of
// out_ecp_stats, then on a 64-element border the workspace of the pseudopotential energy (carve_ecp) for chunks of ng groups, as
// one block of its own extent: ecp_energy_forward carves it itself.
template <typename T> struct DmcEcpWs {
    DmcWs<T> dmc;
    double *EPP2, *PART3;
    void* wse; int64_t wse_bytes;
};
template <typename T>
DmcEcpWs<T> carve_dmc_ecp(const ds_system* s, Arena<T>& a, int64_t B, int64_t nw, int64_t cap, int nq, int64_t ng) {
    DmcEcpWs<T> w{};
    w.dmc = carve_dmc<T>(s, a, B, nw);
    a.align(2);
    w.EPP2 = (double*)a.take(2 * 3 * (size_t)B);
    w.PART3 = (double*)a.take(2 * 3 * (size_t)((B + ds::DMC_GROUP - 1) / ds::DMC_GROUP));
    a.align(64);
    const size_t n = measure([&](Arena<double>& e) { carve_ecp<double>(s, e, B, cap, nq, ng); });
    w.wse = a.take(n);
    w.wse_bytes = (int64_t)(n * sizeof(T));
    return w;
}
inline int64_t dmc_ecp_bytes(const ds_system* s, int64_t B, int64_t nw, int64_t cap, int nq, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_dmc_ecp<double>(s, a, B, nw, cap, nq, ng); }) * (s->dtype == 0 ? 8 : 4);
}

// Workspace of ds_dmc_step_tmove: that of ds_dmc_step_ecp (EPP2: the triple at x_cur), then x_cur (B,3N), in 8-byte elements E per
// walker and the partials of the four columns of out_ecp_stats, as ints the choice.  (The decision lives in the flags.)
template <typename T> struct DmcTmWs {
    DmcEcpWs<T> ecp;
    T* XCUR;
    double *ETOT, *PART4;
    int* CHOICE;
};
template <typename T>
DmcTmWs<T> carve_dmc_tmove(const ds_system* s, Arena<T>& a, int64_t B, int64_t nw, int64_t cap, int nq, int64_t ng) {
    const size_t b = (size_t)B;
    DmcTmWs<T> w{};
    w.ecp = carve_dmc_ecp<T>(s, a, B, nw, cap, nq, ng);
    w.XCUR = a.take(b * 3 * (size_t)s->sd.N);
    a.align(2);
    w.ETOT = (double*)a.take(2 * b);
    w.PART4 = (double*)a.take(2 * 4 * (size_t)((B + ds::DMC_GROUP - 1) / ds::DMC_GROUP));
    w.CHOICE = (int*)a.take(2 * ((b + 1) / 2));
    return w;
}
inline int64_t dmc_tmove_bytes(const ds_system* s, int64_t B, int64_t nw, int64_t cap, int nq, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_dmc_tmove<double>(s, a, B, nw, cap, nq, ng); }) * (s->dtype == 0 ? 8 : 4);
}

// The split of a workspace between the chain and the pseudopotential (ds_dmc_step_ecp, ds_dmc_step_tmove); bytes(nw, ng) = the
// layout's extent.  One chain walker and one group must fit (false otherwise).  Beside one chain walker the pseudopotential keeps
// room for up to ECP_RESERVE groups (what ds_ecp_workspace_bytes provides at most); then the chain's chunk takes what fits; then
// the groups follow from what is left, as ds_ecp_energy derives them.  (Serving the chain first instead lets a workspace that the
// byte budget cut short run the pseudopotential in chunks of one group: measured 7 x the time of a step.)
template <typename F>
bool split_dmc_ecp(const F& bytes, int64_t ws_bytes, int64_t B, int64_t cap, int nq, int64_t* nw_out, int64_t* ng_out) {
    const int64_t ng_max = std::min<int64_t>(OB_MAX_GROUPS, (cap * nq + ds::PV - 1) / ds::PV);
    const auto fits = [&](int64_t nw_, int64_t ng_) { return bytes(nw_, ng_) <= ws_bytes; };
    const auto largest = [](int64_t hi, const auto& ok) {      // the largest n in 1..hi with ok(n); ok(1) holds and ok is monotone
        int64_t lo = 1;
        while (lo < hi) { const int64_t mid = (lo + hi + 1) / 2; if (ok(mid)) lo = mid; else hi = mid - 1; }
        return lo;
    };
    if (!fits(1, 1)) return false;
    const int64_t ng0 = largest(std::min<int64_t>(ECP_RESERVE, ng_max), [&](int64_t n) { return fits(1, n); });
    const int64_t nw = largest(std::min<int64_t>(B, 65535), [&](int64_t n) { return fits(n, ng0); });
    *nw_out = nw;
    *ng_out = largest(ng_max, [&](int64_t n) { return n <= ng0 || fits(nw, n); });
    return true;
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

// what the three step entries share: the six state arrays, the step, the noise, the outputs
struct DmcCall {
    void *x, *logabs, *phase, *drift; double *eloc, *weight;
    int64_t B; int steps; double tau, tau_eff, e_trial, e_ref, e_cut; int node_mode, branch_every;
    uint64_t seed, offset; const void *normals, *uniforms; const double* comb_uniforms; int state_valid;
    double* out_stats; int* out_parents;
};
// what ds_dmc_step_ecp adds to a call (e == nullptr: ds_dmc_step)
struct DmcEcpCall {
    const ds_ecp* e = nullptr; int64_t cap = 0; const double* rotations = nullptr; double* epp = nullptr; double* out_ecp_stats = nullptr;
    int64_t* out_pairs = nullptr; int* steps_done = nullptr;
};

// What the three step entries refuse, in this order, before anything is launched.  name: the entry; p: what a pseudopotential adds
// (nullptr: ds_dmc_step); given / expected: how many of the entry's explicit noise arrays are not NULL, and how many it takes.
inline int dmc_check(const char* name, ds_system* s, const void* params, const void* ws, const DmcCall& q, const DmcEcpCall* p, int given,
                     int expected) {
    static const char* const noise[] = {"normals, uniforms and comb_uniforms", "normals, uniforms, comb_uniforms and rotations",
                                        "normals, uniforms, comb_uniforms, rotations and tmove_uniforms"};
    if (p && p->steps_done) *p->steps_done = 0;
    if (s) ++s->call_seq;
    if (!s || !params || !ws) return fail("%s: null argument", name);
    if (!q.x || !q.logabs || !q.phase || !q.drift || !q.eloc || !q.weight) return fail("%s: null state pointer", name);
    if (p && !p->epp) return fail("%s: epp is null (the seventh state array)", name);
    if (!q.out_stats) return fail("%s: out_stats is null", name);
    if (q.B < 1 || q.B > ds::DMC_MAX_B) return fail("%s: B must be in 1..%lld (got %lld)", name, (long long)ds::DMC_MAX_B, (long long)q.B);
    if (q.steps < 1) return fail("%s: steps must be >= 1 (got %d)", name, q.steps);
    if (!std::isfinite(q.tau) || !std::isfinite(q.tau_eff) || !std::isfinite(q.e_trial) || !std::isfinite(q.e_ref) || !std::isfinite(q.e_cut))
        return fail("%s: tau, tau_eff, e_trial, e_ref and e_cut must be finite", name);
    if (!(q.tau > 0.0)) return fail("%s: tau must be > 0 (got %g)", name, q.tau);
    if (q.tau_eff < 0.0) return fail("%s: tau_eff must be >= 0 (got %g)", name, q.tau_eff);
    if (q.node_mode != 0 && q.node_mode != 1)
        return fail("%s: node_mode must be 0 (fixed phase) or 1 (fixed node) (got %d)", name, q.node_mode);
    if (q.branch_every < 0) return fail("%s: branch_every must be >= 0 (got %d)", name, q.branch_every);
    if (given != 0 && given != expected) return fail("%s: %s must be given together (or all NULL)", name, noise[expected - 3]);
    if (!p) return 0;
    if (q.offset >= (1ull << 61) || q.offset + (uint64_t)q.steps >= (1ull << 61))
        return fail("%s: philox_offset + steps must be below 2^61 (the rotations' stream 4 lies above)", name);
    return ecp_check(s, p->e, q.B, p->cap);
}

// the chain's chunk that the *_workspace_bytes entries provide: what ds_workspace_bytes gives the energy chain of B walkers
inline int64_t dmc_default_chunk(const ds_system* s, int64_t B) {
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    const int64_t chunk = std::min<int64_t>(B, s->chunk_cap);
    return std::max<int64_t>(1, std::min<int64_t>(chunk, workspace_budget() / ((int64_t)s->ws.per_walker * esz)));
}

// What both step loops work with, built once per call behind the workspace: the typed state, the geometry of the per-walker kernels
// and of the stats rows, the kernels' arguments, the explicit noise of step i (nullptr in Philox mode), and the launches they share.
template <typename T> struct DmcCtx {
    ds_system* s; const void* params; const DmcCall& q; const DmcWs<T>& w; hipStream_t st;
    const ds::SysDev<T>& S = dev<T>(s);
    const int64_t B = q.B, ngroups = (B + ds::DMC_GROUP - 1) / ds::DMC_GROUP;
    const int n3 = 3 * S.N;
    const size_t ne = (size_t)B * S.N;
    T *x = (T*)q.x, *logabs = (T*)q.logabs, *phase = (T*)q.phase, *drift = (T*)q.drift;
    double *eloc = q.eloc, *weight = q.weight;
    const dim3 gw = dim3((unsigned)((B + ds::DMC_WAVES - 1) / ds::DMC_WAVES)), bw = dim3(64 * ds::DMC_WAVES);
    const ds::DmcArgs A{q.tau, std::sqrt(q.tau), q.tau_eff, q.e_trial, q.e_ref, q.e_cut, q.node_mode, S.N, (long long)B};
    const ds::PhiloxKey key{q.seed, q.offset};
    const T* nz(int i) const { return q.normals ? (const T*)q.normals + (size_t)i * B * n3 : nullptr; }
    const T* un(int i) const { return q.uniforms ? (const T*)q.uniforms + (size_t)i * B : nullptr; }

    // the energy chain with both outputs at xe: KE2, EW3 and GC, log|psi| and the phase into la and ph
    int chain(const T* xe, T* la, T* ph) const {
        return energy_grad_forward(s, params, xe, B, w.KE2, w.EW3, la, ph, w.GC, w.wsc, w.wsc_bytes, st);
    }
    // state_valid = 0: the chain at x, then k_dmc_init; with epp its ECP instance, which takes the triple epp2
    int init(const double* epp2, double* epp) const {
        if (int rc = chain(x, logabs, phase)) return rc;
        const auto k = epp ? ds::k_dmc_init<T, true> : ds::k_dmc_init<T, false>;
        hipLaunchKernelGGL(k, gw, bw, 0, st, (long long)B, n3, (const T*)w.GC, (const T*)w.KE2, (const T*)w.EW3, (const T*)logabs, drift, eloc,
                           weight, epp2, epp);
        return 0;
    }
    // step i: the proposal x' into X2 (the noise that was used into NZ), then the chain at x'
    int propose(int i) const {
        hipLaunchKernelGGL((ds::k_dmc_propose<T>), dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, S.sim_a, S.sim_ainv, (const T*)x,
                           (const T*)drift, nz(i), key, (unsigned long long)i, (T)q.tau, (T)A.sqrt_tau, ne, w.X2, w.NZ);
        return chain(w.X2, w.LA2, w.PH2);
    }
    // row i of out_stats from the weights, the energies e and the (p, flags) of the decision -> the row
    double* stats_row(int i, const double* e) const {
        double* row = q.out_stats + (size_t)i * ds::DMC_ROW;
        hipLaunchKernelGGL(ds::k_dmc_stats, dim3((unsigned)ngroups), dim3(ds::DMC_GROUP), 0, st, (long long)B, (const double*)weight, e,
                           (const double*)w.PACC, (const int*)w.FLAGS, w.PART);
        hipLaunchKernelGGL(ds::k_dmc_stats_final, dim3(1), dim3(64), 0, st, (const double*)w.PART, (long long)ngroups, (long long)B, row);
        return row;
    }
    // one row of out_ecp_stats: NC = 3 columns from epp, with NC = 4 the count of choice >= 0
    template <int NC> void ecp_row(const double* epp, const int* choice, double* part, double* out) const {
        hipLaunchKernelGGL(ds::k_dmc_col_stats<NC>, dim3((unsigned)ngroups), dim3(ds::DMC_GROUP), 0, st, (long long)B, (const double*)weight,
                           epp, choice, part);
        hipLaunchKernelGGL(ds::k_dmc_col_stats_final<NC>, dim3(1), dim3(64), 0, st, (const double*)part, (long long)ngroups, out);
    }
    // The end of step i.  On a branching step the comb, which puts the distinct parents into the row (xi: comb_uniforms or stream 2
    // at index B, one past the walkers), and with a pseudopotential the gather of epp from epp2, which the step left equal to it.
    // Otherwise every walker is its own parent.
    void branch(int i, double* row, const double* epp2, double* epp, int* steps_done) const {
        int* par = q.out_parents ? q.out_parents + (size_t)i * B : nullptr;
        if (q.branch_every > 0 && (i + 1) % q.branch_every == 0) {
            double xi = 0.0;
            if (!q.comb_uniforms) {
                uint32_t r[4];
                ds_philox_host(q.seed, q.offset, (uint64_t)i, (uint64_t)B, 2, r);
                xi = ds::u53_co(r[0], r[1]);
            }
            launch_comb<T>(w.comb, B, n3, xi, q.comb_uniforms ? q.comb_uniforms + i : nullptr, x, logabs, phase, drift, eloc, weight, par,
                           row + ds::DMC_ROW - 1, st);
            if (epp)
                hipLaunchKernelGGL(ds::k_dmc_gather_epp, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (long long)B,
                                   (const double*)w.comb.TOT, (const int*)w.comb.PAR, epp2, epp);
        } else if (par) {
            hipLaunchKernelGGL(ds::k_dmc_identity, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (long long)B, par);
        }
        if (steps_done) *steps_done = i + 1;
    }
};

// The pseudopotential triple of the walkers at xe into EPP2, exactly as ds_ecp_energy(xe, seed, counter) forms it (one host
// synchronisation: the pair total, which above the capacity fails the call); slot: its entry of `rotations` and of out_pairs;
// view: the term buffer that the evaluation leaves in the workspace (ecp_tmove)
template <typename T>
int dmc_ecp_eval(const DmcCtx<T>& c, const DmcEcpCall& p, const DmcEcpWs<T>& we, const T* xe, uint64_t counter, int slot, void* view = nullptr) {
    return ecp_energy_forward(c.s, p.e, c.params, xe, c.B, c.q.seed, counter, p.rotations ? p.rotations + (size_t)slot * 9 * c.B : nullptr,
                              p.cap, we.EPP2, nullptr, nullptr, nullptr, we.wse, we.wse_bytes, c.st, nullptr,
                              p.out_pairs ? p.out_pairs + slot : nullptr, view);
}

// ds_dmc_step and ds_dmc_step_ecp (the locality approximation: the pseudopotential at x' enters the decision's E')
template <typename T>
int dmc_step_impl(ds_system* s, const void* params, const DmcCall& q, const DmcEcpCall& p, void* ws, int64_t ws_bytes, hipStream_t st) {
    const int64_t B = q.B, esz = (int64_t)sizeof(T);
    DmcEcpWs<T> we{};
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    if (!p.e) {
        // the chain's chunk follows from the workspace (the layout is linear in nw up to its alignment pad)
        const int64_t head = dmc_bytes(s, B, 0);
        int64_t nw = std::min<int64_t>({(ws_bytes - head) / ((int64_t)s->ws.per_walker * esz), 65535, B});
        while (nw >= 1 && dmc_bytes(s, B, nw) > ws_bytes) --nw;
        if (nw < 1)
            return fail("workspace too small for ds_dmc_step: %lld bytes < %lld for one chain chunk of one walker (see ds_dmc_workspace_bytes)",
                        (long long)ws_bytes, (long long)dmc_bytes(s, B, 1));
        we.dmc = carve_dmc<T>(s, a, B, nw);
    } else {
        const int nq = ecp_n_quad(p.e);
        int64_t nw, ng;
        if (!split_dmc_ecp([&](int64_t nw_, int64_t ng_) { return dmc_ecp_bytes(s, B, nw_, p.cap, nq, ng_); }, ws_bytes, B, p.cap, nq, &nw, &ng))
            return fail("workspace too small for ds_dmc_step_ecp: %lld bytes < %lld for one chain chunk of one walker and one group of %d "
                        "configurations (see ds_dmc_ecp_workspace_bytes)", (long long)ws_bytes,
                        (long long)dmc_ecp_bytes(s, B, 1, p.cap, nq, 1), ds::PV);
        we = carve_dmc_ecp<T>(s, a, B, nw, p.cap, nq, ng);
    }
    if (!a.ok) return carve_fail("DMC step");
    const DmcWs<T>& w = we.dmc;
    const DmcCtx<T> c{s, params, q, w, st};
    if (!q.state_valid) {
        // (the pseudopotential first: a pair total above the capacity then fails the call with the state untouched)
        if (p.e)
            if (int rc = dmc_ecp_eval(c, p, we, (const T*)c.x, q.offset, 0)) return rc;
        if (int rc = c.init(we.EPP2, p.epp)) return rc;
    }
    const auto accept = p.e ? ds::k_dmc_accept<T, true> : ds::k_dmc_accept<T, false>;
    for (int i = 0; i < q.steps; ++i) {
        if (int rc = c.propose(i)) return rc;
        // (a pair total above the capacity fails the call here: the state is that after i steps)
        if (p.e)
            if (int rc = dmc_ecp_eval(c, p, we, (const T*)w.X2, q.offset + 1 + (uint64_t)i, i + 1)) return rc;
        const T* nz = c.nz(i);
        hipLaunchKernelGGL(accept, c.gw, c.bw, 0, st, c.A, c.x, c.logabs, c.phase, c.drift, c.eloc, c.weight, (const T*)w.X2, (const T*)w.LA2,
                           (const T*)w.PH2, (const T*)w.GC, (const T*)w.KE2, (const T*)w.EW3, nz ? nz : (const T*)w.NZ, c.un(i), c.key,
                           (unsigned long long)i, w.PACC, w.FLAGS, we.EPP2, p.epp);
        double* row = c.stats_row(i, c.eloc);
        if (p.e && p.out_ecp_stats) c.template ecp_row<3>(p.epp, nullptr, we.PART3, p.out_ecp_stats + (size_t)i * 3);
        c.branch(i, row, we.EPP2, p.epp, p.steps_done);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// what ds_dmc_step_tmove adds to a ds_dmc_step_ecp call
struct DmcTmCall {
    const double* tmove_uniforms; int* out_tmove; double* out_energy;
};

// ds_dmc_step_tmove: the pseudopotential is evaluated after the decision, at the position the walker then has
template <typename T>
int dmc_tmove_impl(ds_system* s, const void* params, const DmcCall& q, const DmcEcpCall& p, const DmcTmCall& m, void* ws, int64_t ws_bytes,
                   hipStream_t st) {
    const int64_t B = q.B;
    const int nq = ecp_n_quad(p.e);
    int64_t nw, ng;
    if (!split_dmc_ecp([&](int64_t nw_, int64_t ng_) { return dmc_tmove_bytes(s, B, nw_, p.cap, nq, ng_); }, ws_bytes, B, p.cap, nq, &nw, &ng))
        return fail("workspace too small for ds_dmc_step_tmove: %lld bytes < %lld for one chain chunk of one walker and one group of %d "
                    "configurations (see ds_dmc_tmove_workspace_bytes)", (long long)ws_bytes,
                    (long long)dmc_tmove_bytes(s, B, 1, p.cap, nq, 1), ds::PV);
    Arena<T> a = arena_of<T>(ws, ws_bytes);
    const DmcTmWs<T> wt = carve_dmc_tmove<T>(s, a, B, nw, p.cap, nq, ng);
    if (!a.ok) return carve_fail("DMC step with T-moves");
    const DmcEcpWs<T>& we = wt.ecp;
    const DmcWs<T>& w = we.dmc;
    const DmcCtx<T> c{s, params, q, w, st};
    if (!q.state_valid) {
        // (what ds_dmc_step's initialisation does: no pseudopotential is evaluated, eloc is the chain part)
        if (int rc = c.init(nullptr, nullptr)) return rc;
        HIP_OK(hipMemsetAsync(p.epp, 0, sizeof(double) * 3 * (size_t)B, st));
    }
    for (int i = 0; i < q.steps; ++i) {
        if (int rc = c.propose(i)) return rc;
        const T* nz = c.nz(i);
        hipLaunchKernelGGL((ds::k_dmc_tm_decide<T>), c.gw, c.bw, 0, st, c.A, (const T*)c.x, (const T*)c.logabs, (const T*)c.phase,
                           (const T*)c.drift, (const T*)w.X2, (const T*)w.LA2, (const T*)w.PH2, (const T*)w.GC, (const T*)w.KE2,
                           (const T*)w.EW3, nz ? nz : (const T*)w.NZ, c.un(i), c.key, (unsigned long long)i, w.PACC, w.FLAGS, wt.XCUR);
        // the pseudopotential at x_cur.  A pair total above the capacity fails the call here: nothing of step i is committed, the
        // state is that after i steps
        EcpWs<T> view{};
        if (int rc = dmc_ecp_eval(c, p, we, (const T*)wt.XCUR, q.offset + 1 + (uint64_t)i, i, &view)) return rc;
        hipLaunchKernelGGL((ds::k_dmc_tm_commit<T>), c.gw, c.bw, 0, st, c.A, c.x, c.logabs, c.phase, c.drift, c.eloc, c.weight, p.epp,
                           (const T*)w.X2, (const T*)w.LA2, (const T*)w.PH2, (const T*)w.GC, (const T*)w.KE2, (const T*)w.EW3,
                           (const double*)we.EPP2, w.FLAGS, wt.ETOT, m.out_energy ? m.out_energy + (size_t)i * B : nullptr);
        if (int rc = ecp_tmove(s, p.e, &view, c.x, B, q.tau, c.weight, wt.ETOT, m.tmove_uniforms ? m.tmove_uniforms + (size_t)i * B : nullptr,
                               q.seed, q.offset, (uint64_t)i, wt.CHOICE, m.out_tmove ? m.out_tmove + (size_t)i * B : nullptr, st))
            return rc;
        // the rows: the weights and E of the commit (the second chain pass may still zero a weight)
        double* row = c.stats_row(i, wt.ETOT);
        if (p.out_ecp_stats) c.template ecp_row<4>(p.epp, wt.CHOICE, wt.PART4, p.out_ecp_stats + (size_t)i * 4);
        // the chain at x (all B walkers); only the walkers that moved take its outputs
        if (int rc = c.chain(c.x, w.LA2, w.PH2)) return rc;
        hipLaunchKernelGGL((ds::k_dmc_tm_refresh<T>), c.gw, c.bw, 0, st, (long long)B, c.n3, (const int*)wt.CHOICE, (const T*)w.GC,
                           (const T*)w.LA2, (const T*)w.PH2, (const T*)w.KE2, (const T*)w.EW3, c.logabs, c.phase, c.drift, c.eloc, c.weight);
        // (the commit left epp equal to EPP2, the source of the gather)
        c.branch(i, row, we.EPP2, p.epp, p.steps_done);
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
    return dmc_bytes(s, B, dmc_default_chunk(s, B));
}

int ds_dmc_step(ds_system* s, const void* params, void* x, void* logabs, void* phase, void* drift, double* eloc, double* weight, int64_t B,
                int steps, double tau, double tau_eff, double e_trial, double e_ref, double e_cut, int node_mode, int branch_every,
                uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms, const double* comb_uniforms,
                int state_valid, double* out_stats, int32_t* out_parents, void* ws, int64_t ws_bytes, void* stream) {
    const DmcCall q{x, logabs, phase, drift, eloc, weight, B, steps, tau, tau_eff, e_trial, e_ref, e_cut, node_mode, branch_every, philox_seed,
                    philox_offset, normals, uniforms, comb_uniforms, state_valid, out_stats, (int*)out_parents};
    const int given = (normals ? 1 : 0) + (uniforms ? 1 : 0) + (comb_uniforms ? 1 : 0);
    if (int rc = dmc_check("ds_dmc_step", s, params, ws, q, nullptr, given, 3)) return rc;
    return DS_BY_DTYPE(s->dtype, dmc_step_impl, s, params, q, DmcEcpCall{}, ws, ws_bytes, (hipStream_t)stream);
}

// the chain's share as in ds_dmc_workspace_bytes, the pseudopotential's as in ds_ecp_workspace_bytes
int64_t ds_dmc_ecp_workspace_bytes(const ds_system* s, const ds_ecp* e, int64_t B, int64_t pair_capacity) {
    if (!s || !e) { fail("null argument"); return -1; }
    if (B > ds::DMC_MAX_B || ecp_check(s, e, B, pair_capacity)) return -1;
    const int nq = ecp_n_quad(e);
    return dmc_ecp_bytes(s, B, dmc_default_chunk(s, B), pair_capacity, nq, ecp_default_groups(s, B, pair_capacity, nq));
}

int ds_dmc_step_ecp(ds_system* s, const ds_ecp* ecp, const void* params, void* x, void* logabs, void* phase, void* drift, double* eloc,
                    double* weight, double* epp, int64_t B, int steps, double tau, double tau_eff, double e_trial, double e_ref, double e_cut,
                    int node_mode, int branch_every, uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms,
                    const double* comb_uniforms, const double* rotations, int64_t pair_capacity, int state_valid, double* out_stats,
                    double* out_ecp_stats, int32_t* out_parents, int64_t* out_pairs, int* steps_done, void* ws, int64_t ws_bytes,
                    void* stream) {
    const DmcCall q{x, logabs, phase, drift, eloc, weight, B, steps, tau, tau_eff, e_trial, e_ref, e_cut, node_mode, branch_every, philox_seed,
                    philox_offset, normals, uniforms, comb_uniforms, state_valid, out_stats, (int*)out_parents};
    const DmcEcpCall p{ecp, pair_capacity, rotations, epp, out_ecp_stats, out_pairs, steps_done};
    const int given = (normals ? 1 : 0) + (uniforms ? 1 : 0) + (comb_uniforms ? 1 : 0) + (rotations ? 1 : 0);
    if (int rc = dmc_check("ds_dmc_step_ecp", s, params, ws, q, &p, given, 4)) return rc;
    return DS_BY_DTYPE(s->dtype, dmc_step_impl, s, params, q, p, ws, ws_bytes, (hipStream_t)stream);
}

// the shares of ds_dmc_ecp_workspace_bytes
int64_t ds_dmc_tmove_workspace_bytes(const ds_system* s, const ds_ecp* e, int64_t B, int64_t pair_capacity) {
    if (!s || !e) { fail("null argument"); return -1; }
    if (B > ds::DMC_MAX_B || ecp_check(s, e, B, pair_capacity)) return -1;
    const int nq = ecp_n_quad(e);
    return dmc_tmove_bytes(s, B, dmc_default_chunk(s, B), pair_capacity, nq, ecp_default_groups(s, B, pair_capacity, nq));
}

int ds_dmc_step_tmove(ds_system* s, const ds_ecp* ecp, const void* params, void* x, void* logabs, void* phase, void* drift, double* eloc,
                      double* weight, double* epp, int64_t B, int steps, double tau, double tau_eff, double e_trial, double e_ref,
                      double e_cut, int node_mode, int branch_every, uint64_t philox_seed, uint64_t philox_offset, const void* normals,
                      const void* uniforms, const double* comb_uniforms, const double* rotations, const double* tmove_uniforms,
                      int64_t pair_capacity, int state_valid, double* out_stats, double* out_ecp_stats, int32_t* out_parents,
                      int64_t* out_pairs, int32_t* out_tmove, double* out_energy, int* steps_done, void* ws, int64_t ws_bytes,
                      void* stream) {
    const DmcCall q{x, logabs, phase, drift, eloc, weight, B, steps, tau, tau_eff, e_trial, e_ref, e_cut, node_mode, branch_every, philox_seed,
                    philox_offset, normals, uniforms, comb_uniforms, state_valid, out_stats, (int*)out_parents};
    const DmcEcpCall p{ecp, pair_capacity, rotations, epp, out_ecp_stats, out_pairs, steps_done};
    const DmcTmCall m{tmove_uniforms, (int*)out_tmove, out_energy};
    const int given = (normals ? 1 : 0) + (uniforms ? 1 : 0) + (comb_uniforms ? 1 : 0) + (rotations ? 1 : 0) + (tmove_uniforms ? 1 : 0);
    if (int rc = dmc_check("ds_dmc_step_tmove", s, params, ws, q, &p, given, 5)) return rc;
    return DS_BY_DTYPE(s->dtype, dmc_tmove_impl, s, params, q, p, m, ws, ws_bytes, (hipStream_t)stream);
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
