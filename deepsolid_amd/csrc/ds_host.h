// ds_host.h -- what the host units of libdeepsolid_hip.so share (ds_api.hip, ds_chain.hip, ds_det.hip, ds_value.hip,
// ds_gradpass.hip, ds_minsr.hip, ds_sample.hip, ds_dmc.hip, ds_observe.hip) on top of ds_base.h (error slot, workspace arena): the handle, the workspace layouts of the
// two chains and the few functions that one unit calls in another.  Internal to the library.
#pragma once
#include "ds_base.h"
#include "ds_value.h"

namespace ds {
namespace host {

// A pass over groups of PV walkers: elements shared by all groups and elements per group (measured from the pass's layout function)
struct PassSize { size_t fixed, per_group; };
// The groups per pass a *_workspace_bytes entry point provides for a batch of B walkers: all of them, at most 64, within a byte budget ...
inline int64_t groups_per_pass(int64_t B, int64_t esz, const PassSize& z, int64_t budget) {
    const int64_t groups = std::min<int64_t>((std::max<int64_t>(B, 1) + ds::PV - 1) / ds::PV, 64);
    return std::max<int64_t>(1, std::min<int64_t>(groups, budget / ((int64_t)z.per_group * esz)));
}
// ... and its inverse: the groups a workspace of ws_bytes has room for (< 1: too small)
inline int64_t groups_that_fit(int64_t ws_bytes, int64_t esz, const PassSize& z) {
    return (ws_bytes / esz - (int64_t)z.fixed) / (int64_t)z.per_group;
}

// per-walker workspace carve, in elements
struct WsLayout {
    size_t G, MEAN, ZB, H2, Q, MOUT, MINV, DETS, TR;      // sizes of one buffer per walker
    size_t PARTM = 0;                                      // value chain: per-tile segment sums of the pair layer (k_two_layer)
    size_t XL = 0;                                         // layer-0 input tiles [N][h1[0] + nch h2[0]][P] (low-rank first hidden layer)
    size_t YO = 0;                                         // (y, oL) of the layer-0 output per electron and feature [N][h1[1]][2]
    size_t mout_off[2], minv_off[2], dets_off[2], tr_off[2];
    size_t per_walker;                                     // measured extent of carve() / carve_value() at one walker / one group
};

}  // namespace host
}  // namespace ds

struct ds_system {
    ds_system_desc d;                 // scalar fields only (pointers invalid after create)
    int dtype;
    ds::SysDev<double> sd;
    ds::SysDev<float> sf;
    void* blob64 = nullptr;
    void* blob32 = nullptr;
    std::vector<ds_param_block> blocks;
    int64_t nparams = 0;
    ds::host::WsLayout ws;                      // forward-Laplacian chain, per walker
    ds::host::WsLayout wsv;                     // value chain, per group of PV walkers
    // block indices
    std::vector<int> i_wloc, i_wsh, i_b, i_w2, i_b2, i_worb, i_wsh_orb, i_borb, i_pi, i_sg;
    bool use_last = false;
    // the reference's widths (network.py:111-132) as given to ds_system_create; `d` holds the widths the kernels run (zero-padded:
    // plan_widths) and res1 / res2 say where the reference adds a residual (network.py:525-528: in == out of the REFERENCE widths)
    int32_t ref_single[DS_MAX_LAYERS] = {0}, ref_double[DS_MAX_LAYERS] = {0};
    bool res1[DS_MAX_LAYERS] = {false}, res2[DS_MAX_LAYERS] = {false};
    bool no_lu_wave = false;          // DS_NO_LU_WAVE: log det of 16 < n <= 64 by the Gauss-Jordan inverse kernel (as before round 3)
    int val_nb = 0;                   // DS_VAL_NB = 1 / 2 / 4: one wave-tile width for the value chain's GEMMs (default: by workgroup count)
    bool det_valu = false;            // DS_DET_VALU (read once in ds_system_create): VALU determinant-trace kernel
    int64_t chunk_cap = 4096;         // DS_CHUNK_WALKERS: walkers per chunk of the local-energy chain (workspace sizing)
    bool use_g4 = true;               // DS_NO_G4 unset: the dense float64 layer of the 24-electron cells multiplies its last slot tile as 4-column groups
    bool use_pair_expand = true;      // DS_NO_PAIR_EXPAND unset: a pair layer writes the pair-mean rows of the next one-electron layer itself (k_two_layer_expand)
    bool use_pair_recompute = true;   // DS_NO_PAIR_RECOMPUTE unset: a float64 residual pair layer runs the layer in front of it in registers; that layer's output is not written (k_two_layer_expand<.., PREV>)
    bool use_pm_skip = true;         // DS_NO_PM_SKIP unset: the dense float64 hidden layer skips the structurally zero slot tiles of its pair-mean rows
    bool use_lr = true;               // DS_NO_LOWRANK unset: the first hidden layer runs on the low-rank form of its input (k_layer1_lr)
    void* lr_w0t = nullptr;           // transposed / padded layer-0 weights of that kernel, refilled from the parameters at every call
    int64_t val_i8_min_tiles = 512;   // (group, electron) tiles from which they do: two per CU (DS_I8_VAL_MIN_TILES overrides: measurements)
    bool use_i8_val = true;           // DS_NO_I8_VAL unset: the value chain's residual hidden layers run as the int8 split too (large batches)
    int val_i8_call = 0;              // 0: a launch of the value chain decides by its own tiles; +1 / -1: the call has decided for all of its launches (ValI8Call)
    bool use_pair_fuse = true;        // DS_NO_PAIR_FUSE unset: a log-psi forward runs all pair layers in one launch (k_pair_stream_val, ds_value.h)
    bool use_ldsb = true;             // DS_NO_LDSB unset: float32 cells with more than 10 slot tiles run the orbital head with LDS-staged jet rows (ds_ldsb.h)
    bool use_i8 = false;              // DS_I8=1: dense hidden layers of the 5-slot-tile float64 cells run their per-electron contraction as a 47-bit int8 split (ds_i8.h); default since round 6: float64 MFMA (the split measured 17.0-17.7 ms against 19.6 at 13 x the energy error)
    void* i8_wp = nullptr;            // per layer: digit planes of its weights + (behind them) the 256 column scales; filled once per C-ABI call
    uint64_t call_seq = 0;            // counts the C-ABI calls that take `params` (the planes of layer l are current when i8_prepped[l] == call_seq)
    uint64_t i8_prepped[DS_MAX_LAYERS];   // (set to ~0 at creation: never equal to a call count)
    int n_cu = 256;                   // compute units of the device (grid of the persistent int8 layer kernel)
    bool use_wide = true;             // DS_NO_WIDE unset: the chunked kernels of ds_wide.h for more than 10 slot tiles where they are faster
    bool wide_all = false;            // DS_WIDE_ALL: ... everywhere (tests, A/B runs)
    int dbg = 0;                      // DS_DBG (kernel development): 32 = phase stamps of one wave; 1 / 2 switch arithmetic off in a `make EXP=1` build only
    // optional per-kernel timing with HIP events on the caller's stream (ds_profile_*)
    bool prof_on = false;
    int prof_only = -1;               // >= 0: record events for this kernel kind only (keeps the timed region undisturbed)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[DS_PROF_KINDS];
    std::vector<hipEvent_t> prof_pool;
    unsigned long long* clk_dev = nullptr;   // [2] cycles / ticks accumulated by the hidden-layer kernel while profiling (in-kernel clock probe)
    bool prof_failed = false;         // an event could not be created / recorded: ds_profile_read reports it
};

namespace ds {
namespace host {

// records an event pair around the launches issued while it is alive
struct ProfScope {
    ds_system* s; int kind; hipStream_t st; hipEvent_t e0 = nullptr, e1 = nullptr;
    static hipEvent_t get(ds_system* s) {
        if (!s->prof_pool.empty()) { hipEvent_t e = s->prof_pool.back(); s->prof_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { s->prof_failed = true; return nullptr; }
        return e;
    }
    ProfScope(ds_system* s_, int kind_, hipStream_t st_) : s(s_), kind(kind_), st(st_) {
        if (s->prof_on && (s->prof_only < 0 || s->prof_only == kind)) {
            e0 = get(s); e1 = get(s);
            if (!e0 || !e1 || hipEventRecord(e0, st) != hipSuccess) { s->prof_failed = true; recycle(); }
        }
    }
    void recycle() {
        if (e0) s->prof_pool.push_back(e0);
        if (e1) s->prof_pool.push_back(e1);
        e0 = e1 = nullptr;
    }
    ~ProfScope() {
        if (e0) {
            if (hipEventRecord(e1, st) == hipSuccess) s->prof_ev[kind].push_back({e0, e1});
            else { s->prof_failed = true; recycle(); }
        }
    }
};

template <typename T> ds::SysDev<T>& dev(ds_system* s);
template <> inline ds::SysDev<double>& dev<double>(ds_system* s) { return s->sd; }
template <> inline ds::SysDev<float>& dev<float>(ds_system* s) { return s->sf; }

// ---------------------------------------------------------------- the workspace layouts of the two chains
// forward-Laplacian chain on Bc walkers
template <typename T> struct Carve {
    T *G[2], *MEAN[2], *ZB, *H2[2], *Q, *MOUT, *MINV, *DETS, *TR, *XL, *YO;
};
template <typename T> Carve<T> carve(const ds_system* s, Arena<T>& a, int64_t Bc) {
    const WsLayout& w = s->ws;
    Carve<T> c;
    for (T*& g : c.G) g = a.take(w.G * Bc);
    for (T*& m : c.MEAN) m = a.take(w.MEAN * Bc);
    c.ZB = a.take(w.ZB * Bc);
    for (T*& h : c.H2) h = a.take(w.H2 * Bc);
    c.Q = a.take(w.Q * Bc);
    c.MOUT = a.take(w.MOUT * Bc); c.MINV = a.take(w.MINV * Bc);
    c.DETS = a.take(w.DETS * Bc); c.TR = a.take(w.TR * Bc);
    c.XL = a.take(w.XL * Bc); c.YO = a.take(w.YO * Bc);
    return c;
}

// The value chain (log psi only) on `Bc` walkers = ceil(Bc / PV) groups; see ds_value.h.
// Buffers of one value-chain pass over ng groups.  The plain pass ping-pongs two G / H2 buffers; the
// gradient pass keeps every layer's activations (Gl[l] = input of layer l, Gl[n_layers] = orbital-head input).
template <typename T> struct ValBufs {
    T* Gl[DS_MAX_LAYERS + 1];
    T* H2l[DS_MAX_LAYERS + 1];
    T *MEAN0, *MEANS, *ZB, *Q, *MOUT, *DETS, *PARTM;     // MEANS: spin means of a hidden layer's input (scratch of k_spin_mean)
    T* PHI[2];              // orbital GEMM output per spin channel (the plain pass reuses ZB for both)
    T* SORB[2];             // use_last_layer: shared term of the orbital head
    T* MINV;                // optional inverses, laid out like MOUT (walker-interleaved)
    T* PM[DS_MAX_LAYERS];   // fused pair stream (k_pair_stream_val): segment sums of pair layer l (PM[0] = PARTM) ...
    bool pm_fit;            // ... which have room in the H2 buffer that path leaves idle
    bool keep;              // gradient passes: every layer's activations and the raw orbital products PHI stay in memory
                            // (MOUT may then be null: the orbital matrices themselves are not formed, ds_pretrain_loss_vjp)
};

template <typename T>
ValBufs<T> carve_value(const ds_system* s, Arena<T>& a, int64_t ng) {
    const ds::SysDev<double>& S = s->sd;      // (the dims of sd and sf are the same)
    const WsLayout& L = s->wsv;
    ValBufs<T> b{};
    T* G[2]; T* MEAN[2]; T* H2[2];
    for (T*& g : G) g = a.take(L.G * ng);
    for (T*& m : MEAN) m = a.take(L.MEAN * ng);
    b.ZB = a.take(L.ZB * ng);
    for (T*& h : H2) h = a.take(L.H2 * ng);
    b.Q = a.take(L.Q * ng); b.MOUT = a.take(L.MOUT * ng);
    b.DETS = a.take(L.DETS * ng); b.PARTM = a.take(L.PARTM * ng);
    b.MEAN0 = MEAN[0]; b.MEANS = MEAN[1];
    for (int l = 0; l <= S.n_layers; ++l) { b.Gl[l] = G[l & 1]; b.H2l[l] = H2[l & 1]; }
    for (int sp = 0; sp < 2; ++sp)            // inside ZB, once per spin: PHI first, S of the orbital head behind it
        a.part(b.ZB, L.ZB * ng, [&](Arena<T>& z) {
            b.PHI[sp] = z.take((size_t)(sp == 0 ? S.n_up : S.n_dn) * S.ocols[sp] * ds::PV * ng);
            b.SORB[sp] = z.take((size_t)S.ocols[sp] * ds::PV * ng);
        });
    // the sums of the fused pair stream's layers 1.. go into the second H2 buffer, which that path leaves unused (a PARTM block is
    // 3/16 of an H2 buffer); without room for them the pair layers run one by one
    Arena<T> idle{H2[1], L.H2 * ng};
    b.PM[0] = b.PARTM;
    for (int l = 1; l < S.n_double && l < DS_MAX_LAYERS; ++l) b.PM[l] = idle.take(L.PARTM * ng);
    b.pm_fit = idle.ok;
    b.MINV = nullptr;
    return b;
}

// A pass whose result is promised to be the same bits for any workspace size runs its value chain in launches whose size the workspace
// decides, and a launch of 512 or more (group, electron) tiles takes the int8 split of the residual hidden layers (ds_value.hip), which
// agrees with the float64 kernels to 1e-12, not to the bit.  Such a pass decides once, from the configurations of the whole call:
// every launch inside the scope, the forward of the undisplaced walkers included, takes the same kernels.
struct ValI8Call {
    ds_system* s;
    ValI8Call(ds_system* s_, int64_t n_elec, int64_t configurations) : s(s_) {
        s->val_i8_call = n_elec * ((configurations + ds::PV - 1) / ds::PV) >= s->val_i8_min_tiles ? 1 : -1;
    }
    ~ValI8Call() { s->val_i8_call = 0; }
    ValI8Call(const ValI8Call&) = delete;
    ValI8Call& operator=(const ValI8Call&) = delete;
};

// ---------------------------------------------------------------- the workspace of the pseudopotential energy (ds_sample.hip, ds_dmc.hip)
// groups of PV configurations per chunk of the passes that walk configurations: a chunk has at most 65535 of them
constexpr int64_t OB_MAX_GROUPS = 65535 / ds::PV;
// groups per chunk that a *_workspace_bytes entry point provides at most (groups_per_pass): what ds_dmc_step_ecp keeps room for
constexpr int64_t ECP_RESERVE = 64;
// Workspace of ds_ecp_energy for B walkers, at most `cap` pairs, nq points per pair and chunks of ng groups of PV configurations.
// Shared by all chunks: log|psi(R)| (B,), phase(R) (B,2), and in 8-byte elements (2 elements each: room in either element size) per
// walker the rotation, E_loc, the pair count, the offsets (B + 1) and the flag, per pair its record (walker; electron and atom; r
// and dhat; v_l(r)) and its nq terms.  Per chunk: the displaced rows, their log|psi| / phase, and the value chain's buffers for ng
// groups (on a 64-element border), which also serve the forward of the walkers themselves.
template <typename T> struct EcpWs {
    T *LA0, *PH0, *XD, *LA, *PH;
    double *ROT, *ELOC, *PR, *PVL, *TERM;
    long long *CNT, *OFF, *PW;
    int *BAD, *PI;
    void* wsv; int64_t wsv_bytes;
};
template <typename T> EcpWs<T> carve_ecp(const ds_system* s, Arena<T>& a, int64_t B, int64_t cap, int nq, int64_t ng) {
    const size_t nc = (size_t)ng * ds::PV, b = (size_t)B, p = (size_t)cap;
    EcpWs<T> w{};
    w.LA0 = a.take(b); w.PH0 = a.take(2 * b);
    a.align(2);
    w.ROT = (double*)a.take(2 * 9 * b); w.ELOC = (double*)a.take(2 * b);
    w.CNT = (long long*)a.take(2 * b); w.OFF = (long long*)a.take(2 * (b + 1)); w.BAD = (int*)a.take(2 * ((b + 1) / 2));
    w.PW = (long long*)a.take(2 * p); w.PI = (int*)a.take(2 * p);
    w.PR = (double*)a.take(2 * 4 * p); w.PVL = (double*)a.take(2 * 3 * p); w.TERM = (double*)a.take(2 * 2 * p * (size_t)nq);
    w.XD = a.take(nc * 3 * s->sd.N); w.LA = a.take(nc); w.PH = a.take(2 * nc);
    a.align(64);
    w.wsv = a.take(s->wsv.per_walker * (size_t)ng);
    w.wsv_bytes = (int64_t)(s->wsv.per_walker * (size_t)ng * sizeof(T));
    return w;
}
inline int64_t ecp_bytes(const ds_system* s, int64_t B, int64_t cap, int nq, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_ecp<double>(s, a, B, cap, nq, ng); }) * (s->dtype == 0 ? 8 : 4);
}

// ---------------------------------------------------------------- launch geometry that the chains and the reverse sweep share
// workgroup size and grid.z of k_jet_gemm<NB>: at most 1024/NB threads (= its launch bound) per workgroup
inline void gemm_geom(int Nout, int NB, dim3* block, unsigned* gz, int ST = 0) {
    const int nw = Nout / (16 * NB), wmax = (NB == 3 || ST > 5) ? 4 : 1024 / NB / 64;
    int wpb = nw < wmax ? nw : wmax;
    // prefer a multiple of 4 waves per workgroup that divides the wave count: every SIMD then holds the same
    // number of waves (a SIMD with a single wave reaches only 3/4 of the MFMA issue rate)
    for (int c = wpb - wpb % 4; c >= 4; c -= 4)
        if (nw % c == 0) { wpb = c; break; }
    *block = dim3(wpb * 64);
    *gz = (unsigned)((nw + wpb - 1) / wpb);
}

// ---------------------------------------------------------------- what one unit calls in another
// (element types cross as void* + s->dtype, as in the C ABI; the templates are instantiated for double and float in their home unit)

// ds_api.hip: bytes a *_workspace_bytes entry point may ask for: 80 GiB, at most 40 % of the free device memory, at least 1 GiB
int64_t workspace_budget();

// ds_value.hip: the log-psi forward (the samplers, the one-body ratios); the value chain on one chunk (the gradient passes)
int logpsi_forward(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* ws, int64_t ws_bytes,
                   hipStream_t st);
template <typename T>
int run_value_chain(ds_system* s, const T* params, const T* x, int64_t Bc, const ValBufs<T>& vb, hipStream_t st, T* out_logabs, T* out_phase);
// ... and a kernel instance that the reverse sweep launches too: k_jet_gemm<T, 4, 5, 0> (arguments as the kernel's)
template <typename T>
void launch_gemm_plain(dim3 grid, dim3 block, hipStream_t st, const T* X, size_t x_walker_stride, size_t x_tile_stride, const T* W, int K,
                       const T* X2, size_t x2_walker_stride, const T* W2, int K2, int n_tiles, T* Z, size_t z_walker_stride,
                       size_t z_tile_stride, int Nout, int P, const T* Sb, const T* bias, const ds::OrbEpi<T>& oe);
// ... and the int8 split (ds_i8.h has one including unit): whether layer l of either chain runs as one, the bytes of the weight planes a
// handle needs (0: no layer of either chain can), and the layer itself (weight planes prepared once per call)
bool int8_energy_layer(const ds_system* s, int l);
bool int8_value_layer(const ds_system* s, int l);
size_t i8_planes_bytes(const ds_system* s);
void launch_layer_i8(ds_system* s, int l, bool value_epilogue, const double* Wloc, int Kloc, int Nout, const double* Gin, size_t tile_stride,
                     const double* Sb, double* Gout, int ntiles, hipStream_t st);

// ds_gradpass.hip: k_spin_mean (ds_grad.h; block 256), which the value chain launches too
template <typename T> void launch_spin_mean(dim3 grid, hipStream_t st, const ds::SysDev<T>& S, const T* G, int Kh, T* MEAN);

// ds_chain.hip: the walker gradient of log psi (the importance sampler)
int logpsi_grad_forward(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* out_grad,
                        void* ws, int64_t ws_bytes, hipStream_t st);
// ... the same chain with the kinetic energy as well, and the Ewald triple (B,3) behind it (the DMC step)
int energy_grad_forward(ds_system* s, const void* params, const void* x, int64_t B, void* out_ke, void* out_ew3, void* out_logabs,
                        void* out_phase, void* out_grad, void* ws, int64_t ws_bytes, hipStream_t st);
// ... the number of its layers that run as an int8 split (dump: in a stage dump, which has no low-rank layer 1)
int int8_energy_layers(const ds_system* s, bool dump);
// ... and the two residual kernels that both chains launch (block 256, arguments as the kernels')
template <typename T> void launch_pair_res_add(dim3 grid, hipStream_t st, const T* Hin, int Kin, T* Hout, int Kout, int n_res, int NP);
template <typename T>
void launch_layer_res_add(dim3 grid, hipStream_t st, const T* Xin, size_t x_ws, size_t x_ts, T* Gout, size_t g_ws, size_t g_ts, int n_res,
                          int Nout, int P);

// ds_sample.hip: the pseudopotential energy (ds_ecp.h) on a workspace of its own layout (carve_ecp): the body of ds_ecp_energy, which
// the DMC step runs on a sub-range of its workspace.  Arguments as ds_ecp_energy's; *pairs_total (host, optional) receives the pair
// total that the call reads back -- also when it fails because the total exceeds `cap` -- and pairs_total_dev (device, optional) a
// copy of it; *view (optional) the carved EcpWs<T> of the system's element type: the offsets, the pair records, the rotations and
// the term buffer that the evaluation leaves in `ws`.  ecp_tmove: the heat-bath T-move of the DMC step (k_ecp_tmove) on such a
// view, for the walkers in x that were just evaluated.  ecp_check: what ds_ecp_workspace_bytes and ds_ecp_energy refuse alike (also
// a null descriptor); ecp_n_quad: N_q; ecp_default_groups: the groups per chunk that ds_ecp_workspace_bytes provides
int ecp_energy_forward(ds_system* s, const ds_ecp* e, const void* params, const void* x, int64_t B, uint64_t seed, uint64_t offset,
                       const double* rotations, int64_t cap, double* out_energy, int64_t* out_pairs, void* out_ratio, double* out_rotation,
                       void* ws, int64_t ws_bytes, hipStream_t st, int64_t* pairs_total, int64_t* pairs_total_dev, void* view = nullptr);
int ecp_tmove(ds_system* s, const ds_ecp* e, const void* view, void* x, int64_t B, double tau, const double* weight, const double* energy,
              const double* uniforms, uint64_t seed, uint64_t offset, uint64_t step, int* choice, int* out_choice, hipStream_t st);
int ecp_check(const ds_system* s, const ds_ecp* e, int64_t B, int64_t pair_capacity);
int ecp_n_quad(const ds_ecp* e);
int64_t ecp_default_groups(const ds_system* s, int64_t B, int64_t pair_capacity, int nq);

// ds_observe.hip: the sums of ds_ion_forces on rows [nw][2][A][3] that another call has filled (ds_ecp_forces): k_force_part over the
// groups of FORCE_SUM_GROUP (= ds::FORCE_GROUP) walkers into part [groups][12 A + 1], then k_force_final onto sums, the groups in order
constexpr int64_t FORCE_SUM_GROUP = 256;
int force_sums(const double* rows, int64_t nw, int A, double* part, double* sums, hipStream_t st);

// ds_det.hip: the determinant stage of both chains.  Energy chain: inverse + determinant of channel ch, then tr(Y_d), sum Y_d Y_d^T;
// value chain: log det of every channel (and the inverses when vb.MINV is set)
template <typename T>
void launch_det_inverse(const ds_system* s, const ds::SysDev<T>& S, const Carve<T>& c, int ch, int64_t Bc, hipStream_t st);
template <typename T>
int launch_det_trace(const ds_system* s, const ds::SysDev<T>& S, const Carve<T>& c, int ch, int64_t Bc, hipStream_t st);
template <typename T>
void launch_det_value(const ds_system* s, const ds::SysDev<T>& S, const ValBufs<T>& vb, int64_t Bc, hipStream_t st);

}  // namespace host
}  // namespace ds
