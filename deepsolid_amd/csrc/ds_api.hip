// ds_api.hip -- C-ABI entry points of libdeepsolid_hip.so (see include/deepsolid_hip.h).
// Host side only: builds the device tables of one simulation cell, carves the caller's
// workspace and launches the kernels of ds_kernels.h on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/deepsolid_hip.h"
#include "ds_grad.h"
#include "ds_kfac.h"
#include "ds_tiles.h"
#include "ds_mcmc.h"
#include "ds_obs.h"
#include "ds_realspace.h"
#include "ds_onebody.h"
#include "ds_i8.h"

// the per-slot-tile-count kernel instances live in ds_tiles_inst.hip (five slot-tile ranges x two element types)
namespace ds {
#define DS_DECL(p) const TileOps<double>* tile_ops_f64_p##p(int); const TileOps<float>* tile_ops_f32_p##p(int);
DS_DECL(0) DS_DECL(1) DS_DECL(2) DS_DECL(3) DS_DECL(4)
#undef DS_DECL
template <> const TileOps<double>* tile_ops<double>(int st) {
    const TileOps<double>* (*parts[])(int) = {tile_ops_f64_p0, tile_ops_f64_p1, tile_ops_f64_p2, tile_ops_f64_p3, tile_ops_f64_p4};
    for (auto f : parts)
        if (const TileOps<double>* o = f(st)) return o;
    return nullptr;
}
template <> const TileOps<float>* tile_ops<float>(int st) {
    const TileOps<float>* (*parts[])(int) = {tile_ops_f32_p0, tile_ops_f32_p1, tile_ops_f32_p2, tile_ops_f32_p3, tile_ops_f32_p4};
    for (auto f : parts)
        if (const TileOps<float>* o = f(st)) return o;
    return nullptr;
}
}  // namespace ds

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_OK(call)                                                              \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) return fail("%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename I> inline I rup(I x, int m) { return (x + m - 1) / m * m; }

// A workspace as a stack of elements of T.  Every layout below is ONE function over an arena and serves both as the size of the
// layout and as its pointers: with a base, take(n) hands out the next n elements (carve mode); with a null base it only counts
// (measure mode: `used` is the extent).  An entry point checks `ok` after carving and before its first launch.
template <typename T> struct Arena {
    T* base = nullptr;
    size_t cap = SIZE_MAX, used = 0;
    bool ok = true;                                  // false once more was taken than `cap` -- here or in a part() of this arena
    T* take(size_t n) { T* p = base ? base + used : nullptr; used += n; ok = ok && used <= cap; return p; }
    void align(size_t k) { take((k - used % k) % k); }
    // a buffer of n elements already handed out, carved up again (buffers that live inside an idle one); its overrun counts here
    template <typename F> void part(T* buf, size_t n, F&& carve) { Arena a{buf, n}; carve(a); ok = ok && a.ok; }
};
template <typename T> Arena<T> arena_of(void* ws, int64_t ws_bytes) { return Arena<T>{(T*)ws, (size_t)std::max<int64_t>(ws_bytes, 0) / sizeof(T)}; }
// extent, in elements, of a layout function
template <typename F> size_t measure(F&& layout) { Arena<double> a; layout(a); return a.used; }

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

inline int carve_fail(const char* what) { return fail("internal: %s: workspace carve exceeds its size", what); }

void inv3(const double* a, double* o) {
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                       a[2] * (a[3] * a[7] - a[4] * a[6]);
    o[0] = (a[4] * a[8] - a[5] * a[7]) / det; o[1] = (a[2] * a[7] - a[1] * a[8]) / det; o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = (a[5] * a[6] - a[3] * a[8]) / det; o[4] = (a[0] * a[8] - a[2] * a[6]) / det; o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = (a[3] * a[7] - a[4] * a[6]) / det; o[7] = (a[1] * a[6] - a[0] * a[7]) / det; o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
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

}  // namespace

struct ds_system {
    ds_system_desc d;                 // scalar fields only (pointers invalid after create)
    int dtype;
    ds::SysDev<double> sd;
    ds::SysDev<float> sf;
    void* blob64 = nullptr;
    void* blob32 = nullptr;
    std::vector<ds_param_block> blocks;
    int64_t nparams = 0;
    WsLayout ws;                      // forward-Laplacian chain, per walker
    WsLayout wsv;                     // value chain, per group of PV walkers
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
    bool use_pm_skip = true;          // DS_NO_PM_SKIP unset: the dense float64 hidden layer skips the structurally zero slot tiles of its pair-mean rows
    bool use_lr = true;               // DS_NO_LOWRANK unset: the first hidden layer runs on the low-rank form of its input (k_layer1_lr)
    void* lr_w0t = nullptr;           // transposed / padded layer-0 weights of that kernel, refilled from the parameters at every call
    int64_t val_i8_min_tiles = 512;   // (group, electron) tiles from which they do: two per CU (DS_I8_VAL_MIN_TILES overrides: measurements)
    bool use_i8_val = true;           // DS_NO_I8_VAL unset: the value chain's residual hidden layers run as the int8 split too (large batches)
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

namespace {

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

template <typename T>
void fill_tables(ds_system* s, const ds_system_desc* d, ds::SysDev<T>& S, std::vector<T>& host) {
    auto push = [&](const double* p, size_t n) {
        size_t off = host.size();
        for (size_t i = 0; i < n; ++i) host.push_back((T)p[i]);
        while (host.size() % 4) host.push_back(0);
        return off;
    };
    double pinv[9], sinv[9];
    inv3(d->prim_a, pinv);
    inv3(d->sim_a, sinv);
    // lattice displacement tables
    double disp[81], shift[81];
    int q = 0;
    for (int a = -1; a <= 1; ++a)               // ewaldsum.py:54-56 meshgrid 'ij' of arange(-1,2)
        for (int b = -1; b <= 1; ++b)
            for (int c = -1; c <= 1; ++c, ++q)
                for (int k = 0; k < 3; ++k)
                    disp[3 * q + k] = a * d->sim_a[k] + b * d->sim_a[3 + k] + c * d->sim_a[6 + k];
    q = 0;
    for (int a = 0; a < 3; ++a)                 // distance.py:66-68 meshgrid default 'xy': point = (x[b], y[a], z[c]) - 1
        for (int b = 0; b < 3; ++b)
            for (int c = 0; c < 3; ++c, ++q)
                for (int k = 0; k < 3; ++k)
                    shift[3 * q + k] = (b - 1) * d->sim_a[k] + (a - 1) * d->sim_a[3 + k] + (c - 1) * d->sim_a[6 + k];
    size_t o_pa = push(d->prim_a, 9), o_pi = push(pinv, 9), o_sa = push(d->sim_a, 9), o_si = push(sinv, 9);
    size_t o_pav = push(d->prim_AV, 3 * d->n_sym), o_pbv = push(d->prim_BV, 3 * d->n_sym);
    size_t o_sav = push(d->sim_AV, 3 * d->n_sym), o_sbv = push(d->sim_BV, 3 * d->n_sym);
    size_t o_at = push(d->prim_atoms, 3 * d->n_atoms_prim);
    // k-vector table per spin; with full_det every spin block sees the concatenated list (network.py:452-454)
    std::vector<double> kcat(d->klist_up, d->klist_up + 3 * d->n_up);
    if (d->n_dn) kcat.insert(kcat.end(), d->klist_dn, d->klist_dn + 3 * d->n_dn);
    size_t o_k0, o_k1;
    if (d->full_det) { o_k0 = o_k1 = push(kcat.data(), kcat.size()); }
    else { o_k0 = push(d->klist_up, 3 * d->n_up); o_k1 = d->n_dn ? push(d->klist_dn, 3 * d->n_dn) : o_k0; }
    size_t o_sat = push(d->sim_atoms, 3 * d->n_atoms_sim), o_q = push(d->sim_charges, d->n_atoms_sim);
    size_t o_d27 = push(disp, 81), o_s27 = push(shift, 81);
    size_t o_g = push(d->gpoints, 3 * (size_t)d->n_g), o_gw = push(d->gweight, d->n_g);
    size_t o_ir = push(d->ion_exp_re, d->n_g), o_ii = push(d->ion_exp_im, d->n_g);
    // integer coordinates of the G mesh in the reciprocal basis: n_j = G . a_j / 2 pi (ewaldsum.py:68-89 builds G from them);
    // the phase tables of k_ewald are used when they are exact integers and N x (table length) fits comfortably in LDS
    std::vector<double> gidx(3 * (size_t)d->n_g, 0.0);
    int nmin[3] = {0, 0, 0}, nmax[3] = {0, 0, 0};
    bool integral = d->n_g > 0 && !getenv("DS_EWALD_DIRECT");
    for (int g = 0; g < d->n_g && integral; ++g)
        for (int j = 0; j < 3; ++j) {
            const double v = (d->gpoints[3 * g] * d->sim_a[3 * j] + d->gpoints[3 * g + 1] * d->sim_a[3 * j + 1] +
                              d->gpoints[3 * g + 2] * d->sim_a[3 * j + 2]) / 6.283185307179586476925286766559;
            const double r = std::nearbyint(v);
            if (std::fabs(v - r) > 1e-6 || std::fabs(r) > 30000) { integral = false; break; }
            gidx[3 * (size_t)g + j] = r;
            if (g == 0 || r < nmin[j]) nmin[j] = (int)r;
            if (g == 0 || r > nmax[j]) nmax[j] = (int)r;
        }
    int goff[3] = {0, 0, 0}, glen = 0;
    if (integral) {
        for (int j = 0; j < 3; ++j) { goff[j] = glen; glen += nmax[j] - nmin[j] + 1; }
        if ((size_t)(d->n_up + d->n_dn) * glen * 2 * sizeof(T) > 64 * 1024) integral = false;
    }
    if (integral) {
        for (int g = 0; g < d->n_g; ++g)
            for (int j = 0; j < 3; ++j) gidx[3 * (size_t)g + j] += goff[j] - nmin[j];
    } else glen = 0;
    size_t o_gi = push(gidx.data(), integral ? gidx.size() : 0);
    S.gidx = (const T*)o_gi; S.g_len = glen;
    for (int j = 0; j < 3; ++j) { S.g_nmin[j] = nmin[j]; S.g_off[j] = goff[j]; }
    // offsets are turned into pointers after the upload
    S.prim_a = (const T*)o_pa; S.prim_ainv = (const T*)o_pi; S.sim_a = (const T*)o_sa; S.sim_ainv = (const T*)o_si;
    S.prim_AV = (const T*)o_pav; S.prim_BV = (const T*)o_pbv; S.sim_AV = (const T*)o_sav; S.sim_BV = (const T*)o_sbv;
    S.atoms = (const T*)o_at; S.klist[0] = (const T*)o_k0; S.klist[1] = (const T*)o_k1;
    S.sim_atoms = (const T*)o_sat; S.sim_charges = (const T*)o_q; S.disp27 = (const T*)o_d27; S.shift27 = (const T*)o_s27;
    S.gpoints = (const T*)o_g; S.gweight = (const T*)o_gw; S.ion_re = (const T*)o_ir; S.ion_im = (const T*)o_ii;
    S.N = d->n_up + d->n_dn; S.n_up = d->n_up; S.n_dn = d->n_dn; S.A = d->n_atoms_prim; S.L = d->n_sym; S.K = d->n_det;
    S.nch = d->n_dn > 0 ? 2 : 1;
    S.D = 3 * S.N + 2; S.P = rup(S.D, 16); S.NP = rup(S.N * S.N, 16);
    S.n_layers = d->n_layers; S.n_double = d->use_last_layer ? d->n_layers : d->n_layers - 1;   // network.py:134
    S.dist_type = d->distance_type; S.nf = d->distance_type == 0 ? 4 : 7;
    S.h1[0] = rup(S.nf * S.A, 4); S.h2[0] = rup(S.nf, 4);      // zero rows pad 'tri' (7 features) to the MFMA k-step
    int ldk = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        S.h1[l + 1] = d->hidden_single[l];
        S.h2[l + 1] = d->hidden_double[l];
        ldk = std::max(ldk, S.h1[l] + S.nch * S.h2[l]);
    }
    ldk = std::max(ldk, S.h1[d->n_layers] + (d->use_last_layer ? S.nch * S.h2[d->n_layers] : 0));
    S.ldk = ldk;
    S.full_det = d->full_det; S.env_type = d->envelope_type; S.bias_orb = d->bias_orbitals;
    if (d->full_det) {
        S.norb[0] = S.norb[1] = S.N; S.n_detch = 1; S.det_n[0] = S.N; S.det_n[1] = 0;
        S.mat_ch[0] = S.mat_ch[1] = 0; S.row_off[0] = 0; S.row_off[1] = d->n_up;
    } else {
        S.norb[0] = d->n_up; S.norb[1] = d->n_dn; S.n_detch = S.nch; S.det_n[0] = d->n_up; S.det_n[1] = d->n_dn;
        S.mat_ch[0] = 0; S.mat_ch[1] = 1; S.row_off[0] = S.row_off[1] = 0;
    }
    S.nparam[0] = S.norb[0] * d->n_det; S.nparam[1] = d->n_dn ? S.norb[1] * d->n_det : 0;
    S.nparam_max = std::max(S.nparam[0], S.nparam[1]);
    S.ocols[0] = rup(2 * S.nparam[0], 64); S.ocols[1] = rup(2 * S.nparam[1], 64);
    S.As = d->n_atoms_sim; S.NG = d->n_g; S.dist_mode = d->dist_mode;
    S.alpha = (T)d->ewald_alpha; S.ee_const = (T)d->ee_const; S.ei_const = (T)d->ei_const; S.ii_total = (T)d->ii_total;
    (void)s;
}

template <typename T> void relocate(ds::SysDev<T>& S, const T* base) {
    auto fix = [&](const T*& p) { p = base + (size_t)p; };
    fix(S.prim_a); fix(S.prim_ainv); fix(S.sim_a); fix(S.sim_ainv); fix(S.prim_AV); fix(S.prim_BV); fix(S.sim_AV);
    fix(S.sim_BV); fix(S.atoms); fix(S.klist[0]); fix(S.klist[1]); fix(S.sim_atoms); fix(S.sim_charges); fix(S.disp27);
    fix(S.shift27); fix(S.gpoints); fix(S.gweight); fix(S.ion_re); fix(S.ion_im); fix(S.gidx);
}

template <typename T> ds::SysDev<T>& dev(ds_system* s);
template <> ds::SysDev<double>& dev<double>(ds_system* s) { return s->sd; }
template <> ds::SysDev<float>& dev<float>(ds_system* s) { return s->sf; }

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

void build_layouts(ds_system* s) {
    const ds::SysDev<double>& S = s->sd;
    int64_t off = 0;
    auto add = [&](int rows, int cols) {
        ds_param_block b{off, rows, cols};
        s->blocks.push_back(b);
        off += (int64_t)rows * cols;
        off = (off + 15) / 16 * 16;      // 128-byte alignment of every block
        return (int)s->blocks.size() - 1;
    };
    for (int l = 0; l < S.n_layers; ++l) {
        s->i_wloc.push_back(add(S.h1[l] + S.nch * S.h2[l], S.h1[l + 1]));
        s->i_wsh.push_back(add(S.nch * S.h1[l], S.h1[l + 1]));
        s->i_b.push_back(add(1, S.h1[l + 1]));
    }
    for (int l = 0; l < S.n_double; ++l) {
        s->i_w2.push_back(add(S.h2[l], S.h2[l + 1]));
        s->i_b2.push_back(add(1, S.h2[l + 1]));
    }
    for (int c = 0; c < S.nch; ++c) {
        // network.py:129-130,178: with use_last_layer the orbital head takes the symmetric features (h | means | pair means)
        s->i_worb.push_back(add(S.h1[S.n_layers] + (s->use_last ? S.nch * S.h2[S.n_layers] : 0), S.ocols[c]));
        s->i_wsh_orb.push_back(s->use_last ? add(S.nch * S.h1[S.n_layers], S.ocols[c]) : -1);
        s->i_borb.push_back(S.bias_orb ? add(1, 2 * S.nparam[c]) : -1);
        s->i_pi.push_back(add(S.A, S.nparam[c]));
        const int sig_rows = S.env_type == 0 ? S.A : (S.env_type == 1 ? 3 * S.A : 9 * S.A);   // network.py:146-152
        s->i_sg.push_back(add(sig_rows, S.nparam[c]));
    }
    s->nparams = off;
    WsLayout& w = s->ws;
    int h1max = 0, h2max = 0;
    for (int l = 0; l <= S.n_layers; ++l) { h1max = std::max(h1max, S.h1[l]); h2max = std::max(h2max, S.h2[l]); }
    w.G = (size_t)S.N * S.ldk * S.P;
    w.MEAN = (size_t)S.nch * h1max * S.P;
    w.ZB = (size_t)std::max(2 * h1max, std::max(S.ocols[0], S.ocols[1])) * S.P;   // shared spin-mean term S of one layer (of two: the low-rank layer 1 needs S of layer 0 too) / orbital head
    for (int c = 0; c < S.nch; ++c)                  // ... or the orbital GEMM output of one spin
        w.ZB = std::max(w.ZB, (size_t)(c == 0 ? S.n_up : S.n_dn) * S.ocols[c] * S.P);
    w.H2 = (size_t)h2max * 5 * S.NP;
    w.Q = (size_t)S.N * S.nparam_max * 10;
    size_t mo = 0, mi = 0, de = 0, tr = 0;
    for (int c = 0; c < 2; ++c) {                     // c = determinant channel
        const size_t n = c < S.n_detch ? S.det_n[c] : 0;
        w.mout_off[c] = mo; w.minv_off[c] = mi; w.dets_off[c] = de; w.tr_off[c] = tr;
        mo += (size_t)S.K * n * n * 2 * S.P;
        mi += (size_t)S.K * n * n * 2;
        de += (size_t)S.K * 4;
        tr += (size_t)S.K * 2 * S.P;
    }
    w.MOUT = mo; w.MINV = rup(mi, 16); w.DETS = rup(de, 16); w.TR = tr;
    w.XL = (size_t)S.N * (S.h1[0] + S.nch * S.h2[0]) * S.P;
    w.YO = (size_t)rup(S.N * S.h1[1] * 2, 16);
    w.per_walker = measure([&](Arena<double>& a) { carve<double>(s, a, 1); });
    // value chain: the slot axis carries PV walkers (ds_value.h)
    WsLayout& v = s->wsv;
    const size_t PV = ds::PV;
    v = w;
    v.G = (size_t)S.N * S.ldk * PV;
    v.MEAN = (size_t)S.nch * h1max * PV;
    v.ZB = (size_t)std::max(h1max, std::max(S.ocols[0], S.ocols[1])) * PV;
    for (int c = 0; c < S.nch; ++c) v.ZB = std::max(v.ZB, (size_t)((c == 0 ? S.n_up : S.n_dn) + 1) * S.ocols[c] * PV);
    v.H2 = (size_t)(PV / 5) * h2max * 5 * S.NP;
    v.Q = (size_t)S.N * S.nparam_max * 2 * PV;
    mo = 0;
    for (int c = 0; c < 2; ++c) {
        const size_t n = c < S.n_detch ? S.det_n[c] : 0;
        v.mout_off[c] = mo;
        mo += (size_t)S.K * n * n * 2 * PV;
    }
    v.MOUT = mo; v.MINV = 0; v.TR = 0;
    v.DETS = w.DETS * PV;             // DETS stays per walker
    v.PARTM = (size_t)(PV / 5) * h2max * 5 * (S.NP / 16) * ds::PM_SLOTS;
    v.per_walker = measure([&](Arena<double>& a) { carve_value<double>(s, a, 1); });
}

// ---------------------------------------------------------------- launch helpers
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

// Value chain: the wave tile of a GEMM launch follows the number of workgroups it would have with 64-feature waves.  A 4096-walker
// batch (52 groups of 80 walkers x 24 electrons) fills the chip's 512 four-wave slots 2.4 times over; the 512 walkers of a GPU's
// share of a split batch make 168 workgroups -- each a serial chain of K/4 x 20 MFMAs on a SIMD of its own.  32- / 16-feature waves
// in four-wave workgroups: 2 x / 4 x the workgroups, chains a half / a quarter as long; the same products in the same order
// (bit-identical results).  DS_VAL_NB forces one width (tests, measurements).
inline int val_nb(int forced, int64_t wgs64) { return forced ? forced : (wgs64 >= 1024 ? 4 : (wgs64 >= 448 ? 2 : 1)); }
inline void val_geom(int Nout, int NB, dim3* block, unsigned* gz) {
    if (NB >= 3) { gemm_geom(Nout, NB, block, gz); return; }
    *block = dim3(256);
    *gz = (unsigned)((Nout + 64 * NB - 1) / (64 * NB));
}

// k_m2_combine_val: rows per workgroup (grid.z chunks inside one partner spin)
inline int m2_rc(int K2) { return K2 % 16 == 0 ? 16 : K2; }

// k_m2_expand: feature splits (grid.z) so that a workgroup's pair jets take at most ~8 KB of LDS
template <typename T> inline unsigned m2_split(int K2, int N) {
    unsigned z = 1;
    while (z < 8 && K2 % (2 * z) == 0 && (size_t)(K2 / z) * 5 * N * sizeof(T) > 8192) z *= 2;
    return z;
}

enum Stop { STOP_NONE = 0, STOP_G0, STOP_G1, STOP_G2, STOP_G3, STOP_H2_0, STOP_H2_1, STOP_H2_2, STOP_MEAN0, STOP_Q,
            STOP_MOUT, STOP_MINV, STOP_DETS, STOP_TR };

template <typename T> struct DumpReq { int stop; T* out; int64_t cap; int64_t written; };

template <typename T>
int copy_out(DumpReq<T>* dr, const T* src, size_t n, hipStream_t st) {
    size_t m = std::min<size_t>(n, (size_t)dr->cap);
    HIP_OK(hipMemcpyAsync(dr->out, src, m * sizeof(T), hipMemcpyDeviceToDevice, st));
    dr->written = (int64_t)m;
    return 0;
}

// A dense residual hidden layer l with the shape of the int8 split (ds_i8.h: float64, 256 features from K = 320 rows).  The slot axis and
// the switch are the caller's: the energy chain (plan_chain: 5 slot tiles) ...
inline bool i8_shape(const ds_system* s, int l) {
    const ds::SysDev<double>& S = s->sd;
    return s->dtype == 0 && l >= 1 && s->res1[l] && S.h1[l + 1] == ds::i8::NOUT && S.h1[l] + S.nch * S.h2[l] == 320;
}
// ... and the value chain (its column axis is 80 walkers whatever the electron count: any float64 cell with such a layer; whether a
// call takes it depends on its batch)
inline bool int8_value_layer(const ds_system* s, int l) { return s->use_i8_val && ds::PV == ds::i8::P && i8_shape(s, l); }

// digit planes + column scales of layer l's per-electron weights: prepared by the first launch of a C-ABI call that needs them (the
// 20 forwards of an mcmc_step, the chunks of a local-energy batch and the value / energy chains of one call share them)
inline void i8_prepare(ds_system* s, int l, const double* Wloc, int Kloc, int Nout, hipStream_t st, uint8_t** wp, double** sw) {
    const size_t slot = ds::i8::wp_bytes(64 * 5) + ds::i8::NOUT * sizeof(double);
    *wp = (uint8_t*)s->i8_wp + (size_t)l * slot;
    *sw = (double*)(*wp + ds::i8::wp_bytes(64 * 5));
    if (s->i8_prepped[l] != s->call_seq) {
        hipLaunchKernelGGL(ds::i8::k_i8_prep_w, dim3(ds::i8::NOUT / 16), dim3(256), 0, st, Wloc, Kloc, Nout, *wp, *sw);
        s->i8_prepped[l] = s->call_seq;
    }
}

// ---------------------------------------------------------------- the plan of the forward-Laplacian chain
// Which kernel variant every stage of run_chain launches.  All dispatch predicates of the chain live in plan_chain; run_chain executes
// the plan, and the producer and the consumer of a buffer read the same entry of it.
enum class LayerKind {
    Dense,            // k_jet_gemm EPI 1 (+ k_layer_res_add behind it when res_sep)
    DenseRes,         // k_jet_gemm EPI 2: the residual inside the GEMM
    L0Stats,          // layer 0 in front of the low-rank layer 1 as one kernel: k_layer0_stats
    L0Epi9Means,      // ... as two: k_jet_gemm EPI 9 (output dropped), then k_layer0_means per slot chunk
    LowRank1,         // k_layer1_lr: the first hidden layer on the low-rank form of the layer-0 output
    Int8              // i8::k_layer_i8: the per-electron contraction as an int8 split
};
struct PairPlan {     // pair-stream layer l (l < n_double)
    bool res, res_sep;                        // residual inside the kernel / added by k_pair_res_add behind it
    bool expand;                              // k_two_layer_expand: the layer writes the pair-mean rows of one-electron layer l + 1 itself
    bool write_out;                           // the output itself has a reader (another pair layer, or the orbital head's pair means)
    unsigned xz; int EW, NW; size_t xlds;     // k_two_layer_expand: feature splits, electrons and waves per workgroup, LDS bytes
};
struct LayerPlan {    // one-electron layer l
    LayerKind kind;
    bool res_sep;         // k_layer_res_add follows
    bool wide;            // the chunked form of the kind's kernel (ds_wide.h)
    bool pm_mask;         // the layer sets oe.pm_*: its kernel skips the structurally zero slot tiles of the pair-mean rows
    bool pm_unwritten;    // ... and never reads them: the producer of the rows may leave those tiles unwritten
    int prof_kind;
    PairPlan pair;
};
enum class OrbKind { Orb3, Wide, Ldsb, Gemm };
template <typename T> struct ChainPlan {
    const ds::TileOps<T>* to;     // the kernels instantiated per jet-slot tile count (ds_tiles.h)
    bool lr_on;                   // layers 0 and 1 run as L0Stats / L0Epi9Means + LowRank1
    int lr_nc;                    // column tiles of the low-rank layer's per-electron weights C (instances: 2, 3, 4)
    int g4;                       // > 0: DenseRes layers and the orbital head multiply the last slot tile as g4 groups of four columns
    LayerPlan layer[DS_MAX_LAYERS];
    OrbKind orb[2];               // orbital head per spin
    int count(LayerKind k, int n_layers) const {
        int n = 0;
        for (int l = 0; l < n_layers; ++l) n += layer[l].kind == k ? 1 : 0;
        return n;
    }
};

// dump: a stage dump shows the dense path's buffers (no low-rank layer, no fused pair expansion, every tile written)
template <typename T>
int plan_chain(const ds_system* s, bool dump, ChainPlan<T>* p) {
    const ds::SysDev<double>& S = s->sd;      // (the dims of sd and sf are the same)
    const ds::TileOps<T>* to = p->to = ds::tile_ops<T>(S.P / 16);
    if (!to) return fail("no kernel instance for %d slot tiles (N = %d electrons)", S.P / 16, S.N);
    const int ST = to->ST;
    // wide slot ranges: 64-feature x 4/5-tile wave tiles in slot chunks (ds_wide.h), where they are the faster form (or everywhere)
    const bool wide = s->use_wide && to->gemm_wide != nullptr;
    auto gemm_wide = [&](int epi) { return wide && (s->wide_all || ds::gemm_wide_faster<T>(epi)); };
    // Low-rank first hidden layer (k_layer1_lr): layer 0 reads its input tiles from their own buffer XL (layer 1 needs them again
    // while it overwrites G[0]) and does not write its dense output -- k_layer0_stats leaves (y, oL) per electron and the spin means
    // of the output (the input of layer 1's shared term), layer 1 recomputes its residual rows from the layer-0 input.
    const int K0loc = S.h1[0] + S.nch * S.h2[0], K0sh = S.nch * S.h1[0];
    p->lr_nc = std::max(2, (K0loc + K0sh + 4 + 15) / 16);
    // (worth it when the weights C cost fewer products than the rows they replace: Kh / 4 k-steps of NB x NC tiles against
    //  (Kh - K0 - 4) / 4 k-steps of NB x ST -- not for the one- or two-tile cells, N <= 10)
    p->lr_on = !dump && s->use_lr && S.n_layers >= 2 && !s->res1[0] && p->lr_nc <= 4 && S.h1[1] % 16 == 0 && (S.nch * S.h2[1]) % 4 == 0 &&
               3 * (K0loc + K0sh + 4) <= S.h1[1] && p->lr_nc * S.h1[1] < (S.h1[1] - K0loc - K0sh - 4) * ST;
    // the last slot tile as 4-column groups where at most 12 of its 16 columns are jets (instances: three groups on five tiles -- 73 .. 76
    // jets, 24 electrons --, one group on ten tiles -- 48 electrons: two jets on the tenth tile)
    const int used = S.D - 16 * (ST - 1);
    p->g4 = !s->use_g4 ? 0 : (ST == 5 && used > 8 && used <= 12) ? 3 : (ST == 10 && used <= 4) ? 1 : 0;
    for (int l = 0; l < S.n_layers; ++l) {
        const int Kh = S.h1[l], K2 = S.h2[l], Nout = S.h1[l + 1], Kloc = Kh + S.nch * K2;
        LayerPlan& lp = p->layer[l];
        lp = LayerPlan{};
        if (Nout % 64 || Nout > 1024) return fail("hidden_single must be a multiple of 64 and <= 1024 (got %d)", Nout);
        if (l < S.n_double) {
            PairPlan& pp = lp.pair;
            const int K2o = S.h2[l + 1];
            if (K2o != 32 && K2o != 16) return fail("hidden_double must be 16 or 32 (got %d)", K2o);
            if (K2 % 4) return fail("pair-stream width %d is not a multiple of 4", K2);
            // (a first pair layer as wide as the pair features: its residual is added by k_pair_res_add behind the layer)
            pp.res_sep = s->res2[l] && l == 0;
            pp.res = s->res2[l] && !pp.res_sep;
            pp.xz = (!pp.res && K2o == 32) ? 2 : 1;       // (a residual layer keeps its operands: all features in one workgroup)
            pp.write_out = l + 1 < S.n_double || s->use_last;
            // two electrons per workgroup where the output is written and a single electron's pairs would end in the middle of a 128-byte line
            pp.EW = (pp.write_out && S.N % 16 == 8 && pp.xz == 2) ? 2 : 1;
            pp.NW = (pp.EW * S.N + 15) / 16;
            pp.xlds = ((size_t)(K2o / pp.xz) * 5 * pp.EW * S.N + (size_t)pp.EW * S.nch * (K2o / pp.xz) * 5) * sizeof(T);
            // the layer and the spin means of its output in one kernel (a workgroup per electron) when the output jets of an electron's
            // pairs fit the LDS: the next level's rows land in the buffer the one-electron layer below writes its output to
            pp.expand = !dump && s->use_pair_expand && !pp.res_sep && l + 1 < S.n_layers && pp.NW <= 8 && pp.xlds <= 150 * 1024;
        }
        const bool res = s->res1[l];
        // a first layer as wide as its input features: the residual is added by k_layer_res_add behind the layer (see there)
        lp.res_sep = res && l == 0 && (Kloc % 16 != 0 || S.nf * S.A != Nout);
        if (res && !lp.res_sep && Kloc % 16) return fail("residual layer with K = %d: the GEMM's operand ring needs K %% 16 == 0", Kloc);
        if (p->lr_on && l == 1) {
            lp.kind = LayerKind::LowRank1;
            lp.wide = wide && (s->wide_all || ds::lr_wide_faster<T>(p->lr_nc));
        } else if (p->lr_on && l == 0) {
            const bool one_kernel = to->layer0_stats && ds::layer0_stats_instance(ST, K0loc / 4);
            lp.kind = one_kernel ? LayerKind::L0Stats : LayerKind::L0Epi9Means;
            lp.wide = !one_kernel && gemm_wide(9);
        } else if (s->use_i8 && S.P == ds::i8::P && i8_shape(s, l)) {
            lp.kind = LayerKind::Int8;      // (float64, 5 slot tiles)
        } else if (res && !lp.res_sep) {
            lp.kind = LayerKind::DenseRes;
            lp.wide = gemm_wide(2);
        } else {
            lp.kind = LayerKind::Dense;
            lp.wide = gemm_wide(1);
        }
        lp.prof_kind = l == 0 ? DS_PROF_SINGLE_FIRST : (lp.kind == LayerKind::LowRank1 ? DS_PROF_SINGLE_LR : DS_PROF_SINGLE_HIDDEN);
        // Pair-mean rows: layer 0 (EPI 1 / 9: own-feature rows, then the pair-mean rows per partner spin) and the residual hidden layers
        // (EPI 2: whole rounds of four k-steps per partner spin) run them under tile masks.
        // (first finding: every layer-0 kind gets the mask fields, a DenseRes layer 0 with K2 % 16 != 0 included)
        lp.pm_mask = s->use_pm_skip && (l == 0 || (lp.kind == LayerKind::DenseRes && Kh % 16 == 0 && K2 % 16 == 0));
        // The masked tiles of a hidden layer's rows stay unwritten when its kernel never reads them: the low-rank layer 1 (it skips them by
        // itself) and the float64 masked instances.  The chunked kernels of ds_wide.h have no masks: they read every slot.
        lp.pm_unwritten = !dump && l >= 1 && !lp.wide &&
                          (lp.kind == LayerKind::LowRank1 ? s->use_pm_skip : (lp.pm_mask && ds::pm_instance<T>(ST)));
    }
    // orbital head
    const int Korb = S.h1[S.n_layers] + (s->use_last ? S.nch * S.h2[S.n_layers] : 0);
    if (Korb % 16) return fail("orbital head with K = %d: the GEMM's operand ring needs K %% 16 == 0", Korb);
    for (int sp = 0; sp < S.nch; ++sp) {
        const int OC = S.ocols[sp];
        // 192 columns (n_s*K = 96) would give 3 waves of 64 columns per workgroup and leave SIMDs with a single wave;
        // 48-column waves give 4 balanced waves (the MFMA pipe needs >= 2 waves per SIMD, profiles/r01_mfma_f64_probe.json)
        if (to->gemm_orb3 && OC % 256 != 0 && OC % 192 == 0) p->orb[sp] = OrbKind::Orb3;
        else if (gemm_wide(5)) p->orb[sp] = OrbKind::Wide;
        else if (to->orbital_lb && s->use_ldsb && OC % 64 == 0) p->orb[sp] = OrbKind::Ldsb;      // float32 wide cells: jet rows staged in LDS (ds_ldsb.h)
        else p->orb[sp] = OrbKind::Gemm;
    }
    return 0;
}

// Inverse + determinant of the orbital matrices of determinant channel ch: in-place Gauss-Jordan with one lane per matrix row where an
// instance exists (k_det_inv_wave), else the LDS Gauss-Jordan kernel; value = slot 0 of slot tile 0
template <typename T>
void launch_det_inverse(const ds_system* s, const ds::SysDev<T>& S, const Carve<T>& c, int ch, int64_t Bc, hipStream_t st) {
    const WsLayout& L = s->ws;
    const int n = S.det_n[ch];
    const size_t sh = (size_t)n * 2 * n * sizeof(ds::Cx<T>) + 16;
    if (s->no_lu_wave || !ds::launch_det_inv_wave<T>(n, dim3(S.K, (unsigned)Bc), st, S, c.MOUT, L.MOUT, L.mout_off[ch], ch, 16, c.MINV, L.MINV,
                                                     L.minv_off[ch], c.DETS, L.DETS, L.dets_off[ch], S.P))
        hipLaunchKernelGGL((ds::k_det_inverse<T>), dim3(S.K, (unsigned)Bc), dim3(64), sh, st, S, c.MOUT, L.MOUT, L.mout_off[ch], ch,
                           c.MINV, L.MINV, L.minv_off[ch], c.DETS, L.DETS, L.dets_off[ch], S.P, 16, 1, 1);
}

// tr(Y_d), sum Y_d Y_d^T of Y_d = d_d M . M^-1 for determinant channel ch: the instance by matrix size n
template <typename T>
int launch_det_trace(const ds_system* s, const ds::SysDev<T>& S, const Carve<T>& c, int ch, int64_t Bc, hipStream_t st) {
    const WsLayout& L = s->ws;
    const int n = S.det_n[ch];
    const dim3 grid(S.K, (unsigned)Bc);
    unsigned long long* const clk = (s->dbg & 32) ? s->clk_dev + 2 : (unsigned long long*)nullptr;
#define DS_TR_ARGS S, c.MOUT, L.MOUT, L.mout_off[ch], ch, c.MINV, L.MINV, L.minv_off[ch], c.TR, L.TR, L.tr_off[ch], c.DETS, L.DETS, L.dets_off[ch]
    // matrix-core version when the real expansion (2n) is a whole number of k-steps and a slot tile (or half of one) of Y fits LDS
    const int nt = (2 * n + 15) / 16;
    // (nt >= 3: 8-wave workgroups, one per CU at these sizes; their [512] reduction buffer is counted for all)
    const size_t ybytes16 = (size_t)n * 2 * n * 16 * sizeof(T) + 512 * sizeof(ds::Cx<T>);
    const size_t ybytes8 = (size_t)n * 2 * n * 8 * sizeof(T) + 512 * sizeof(ds::Cx<T>);
    const bool sw8 = ybytes16 > 160 * 1024;
    const size_t ybytes = sw8 ? ybytes8 : ybytes16;
    if ((2 * n) % 4 == 0 && ybytes <= 160 * 1024 && nt <= 6 && !s->det_valu) {
#define DS_TRMF(NTV, SWV, NWV, NF) hipLaunchKernelGGL((ds::k_det_trace_mfma<T, NTV, SWV, NWV, NF>), grid, dim3(64 * NWV), ybytes, st, DS_TR_ARGS, clk)
#define DS_TRM(NTV, SWV, NWV) hipLaunchKernelGGL((ds::k_det_trace_mfma<T, NTV, SWV, NWV>), grid, dim3(64 * NWV), ybytes, st, DS_TR_ARGS)
        if (sw8 && (n == 32 || n == 48)) {
            // row-split mode: half the rows of a full slot tile in LDS, nothing computed twice
            // (4 waves: the A fragments + three operand sets need the 512-register budget; 8 waves with one set less
            //  measured slower, 71.3 vs 68.7 ms per diamond step)
            constexpr int NWS = 4;
            const size_t sbytes = (size_t)(n / 2) * 2 * n * 16 * sizeof(T) + 512 * sizeof(ds::Cx<T>);
#define DS_TRS(NTV) hipLaunchKernelGGL((ds::k_det_trace_mfma_split<T, NTV, NWS, (NTV <= 4 || sizeof(T) == 4 ? 2 : 1)>), grid, dim3(64 * NWS), sbytes, st, DS_TR_ARGS, clk)
            if (n == 32) DS_TRS(4); else DS_TRS(6);        // 2n = 16 NT exactly
#undef DS_TRS
        } else if (sw8) { if (nt <= 4) DS_TRM(4, 8, 4); else DS_TRM(6, 8, 4); }
        else if (n == 12) {
            // (pair table in LDS, one operand tile: 37.2 KB -- Y + the table -- and < 128 registers: four workgroups per CU)
            const size_t tbytes = (size_t)n * 2 * n * 16 * sizeof(T) + 512;      // Y + the pair table (78 x 4 bytes)
            hipLaunchKernelGGL((ds::k_det_trace_mfma<T, 2, 16, 4, 12>), grid, dim3(256), tbytes, st, DS_TR_ARGS, clk);
        } else if (n == 24) DS_TRMF(3, 16, 8, 24);      // (compile-time n: see the kernel)
        else if (nt == 1) DS_TRM(1, 16, 4); else if (nt == 2) DS_TRM(2, 16, 4); else if (nt == 3) DS_TRM(3, 16, 8); else if (nt == 4) DS_TRM(4, 16, 8);
        else DS_TRM(6, 16, 4);
#undef DS_TRM
#undef DS_TRMF
    } else if (n > 16 && n <= 64 && !s->det_valu) {
        // any other size (odd n, or a slot tile of Y beyond the LDS): blocks of 16 electrons, two blocks of Y at a time
        const size_t bbytes = (size_t)2 * 16 * 32 * 16 * sizeof(T) + (size_t)(S.P + 256) * sizeof(ds::Cx<T>);
#define DS_TRB(KSMV) hipLaunchKernelGGL((ds::k_det_trace_blocked<T, KSMV>), grid, dim3(256), bbytes, st, DS_TR_ARGS)
        if (n <= 48) DS_TRB(24); else if (n <= 56) DS_TRB(28); else DS_TRB(32);
#undef DS_TRB
    } else {
        // VALU kernel
#define DS_TRACE(NMAX, SP)                                                                                                    \
    do {                                                                                                                      \
        const int rp = ((n * SP + 63) / 64 * 64) / SP;            /* rows per pass: whole waves, >= n when it fits */        \
        const int nthr = std::min(256, rp * SP);                                                                               \
        const size_t sh = ((size_t)n * n + (size_t)SP * (n * n + 1) + nthr) * sizeof(ds::Cx<T>);                               \
        hipLaunchKernelGGL((ds::k_det_trace<T, NMAX, SP>), grid, dim3(nthr), sh, st, DS_TR_ARGS);                              \
    } while (0)
        if (n <= 16) DS_TRACE(16, 16);
        else if (n <= 32) DS_TRACE(32, 8);
        else if (n <= 64) DS_TRACE(64, 2);      // LDS: (1 + SP) n^2 complex must stay below 160 KiB
        else return fail("n_s = %d > 64 electrons per spin is not supported", n);
#undef DS_TRACE
    }
#undef DS_TR_ARGS
    return 0;
}

// The forward-Laplacian chain on a chunk of Bc walkers: executes plan_chain's plan.
template <typename T>
int run_chain(ds_system* s, const T* params, const T* x, int64_t Bc, Arena<T> ws, hipStream_t st, T* out_ke, T* out_logabs,
              T* out_phase, DumpReq<T>* dr, T* out_grad = nullptr) {
    const ds::SysDev<T>& S = dev<T>(s);
    const WsLayout& L = s->ws;
    const Carve<T> c = carve<T>(s, ws, Bc);
    if (!ws.ok) return carve_fail("forward-Laplacian chain");
    auto blk = [&](int i) { return params + s->blocks[i].offset; };
    const int stop = dr ? dr->stop : STOP_NONE;
    ChainPlan<T> plan;
    if (int rc = plan_chain<T>(s, dr != nullptr, &plan)) return rc;
    const ds::TileOps<T>* to = plan.to;
    const int NB = to->NB, ST = to->ST, lr_nc = plan.lr_nc;
    const bool lr_on = plan.lr_on;
    const int K0loc = S.h1[0] + S.nch * S.h2[0], K0sh = S.nch * S.h1[0];
    // 1. features
    {
        ProfScope ps(s, DS_PROF_FEATURES, st);
        size_t sh = (size_t)(9 * S.N) * sizeof(T) + (size_t)S.N * S.A * S.nf * sizeof(ds::Jet5<T>);
        hipLaunchKernelGGL((ds::k_features<T>), dim3((unsigned)Bc), dim3(256), sh, st, S, x, blk(s->i_pi[0]), blk(s->i_sg[0]),
                           blk(s->i_pi[S.nch - 1]), blk(s->i_sg[S.nch - 1]), lr_on ? c.XL : c.G[0], lr_on ? K0loc : S.ldk, c.MEAN[0], c.H2[0], c.Q);
    }
    if (lr_on) {
        const int n = S.h1[1] * 16 * lr_nc;
        hipLaunchKernelGGL((ds::k_lr_w0t<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, blk(s->i_wloc[0]), blk(s->i_wsh[0]), K0loc, K0sh,
                           S.h1[1], 16 * lr_nc, (T*)s->lr_w0t);
    }
    if (stop == STOP_MEAN0) return copy_out(dr, c.MEAN[0], (size_t)S.nch * S.h1[0] * S.P * Bc, st);
    if (stop == STOP_H2_0) return copy_out(dr, c.H2[0], (size_t)S.h2[0] * 5 * S.NP * Bc, st);
    if (stop == STOP_Q) return copy_out(dr, c.Q, L.Q * Bc, st);
    int gi = 0, hi = 0;               // current G / H2 buffer
    for (int l = 0; l < S.n_layers; ++l) {
        const LayerPlan& lp = plan.layer[l];
        const int Kh = S.h1[l], K2 = S.h2[l], Nout = S.h1[l + 1];
        // spin means of the pair stream -> rows [Kh, Kh + nch*K2) of the layer input, unless the pair layer behind them wrote them
        if (!(l > 0 && plan.layer[l - 1].pair.expand)) {
            ProfScope ps(s, DS_PROF_M2_EXPAND, st);
            const bool xl = lr_on && l == 0;
            hipLaunchKernelGGL((ds::k_m2_expand<T>), dim3(S.N, (unsigned)Bc, m2_split<T>(K2, S.N)), dim3(256), (size_t)(K2 * 5 * S.N + S.nch * K2 * 5) / m2_split<T>(K2, S.N) * sizeof(T), st, S,
                               c.H2[hi], K2, xl ? c.XL : c.G[gi], Kh, xl ? K0loc : S.ldk, lp.pm_unwritten ? 1 : 0);
        }
        if (stop == STOP_G0 + l) return copy_out(dr, c.G[gi], L.G * Bc, st);
        // pair stream layer
        if (l < S.n_double) {
            const PairPlan& pp = lp.pair;
            const int K2o = S.h2[l + 1];
            const T* W2 = blk(s->i_w2[l]); const T* b2 = blk(s->i_b2[l]);
            ProfScope ps(s, DS_PROF_TWO_LAYER, st);
            if (pp.expand) {
                // (the rows of level l + 1 land in the buffer the one-electron layer below writes its output to)
#define DS_TWOX(NT2, RES) hipLaunchKernelGGL((ds::k_two_layer_expand<T, NT2, RES>), dim3(S.N / pp.EW, (unsigned)Bc, pp.xz), dim3(64 * pp.NW), pp.xlds, st, S, c.H2[hi], K2, W2, b2, \
                                             pp.write_out ? c.H2[hi ^ 1] : (T*)nullptr, c.G[gi ^ 1], S.h1[l + 1], S.ldk, plan.layer[l + 1].pm_unwritten ? 1 : 0, pp.EW)
                if (K2o == 32 && pp.res) DS_TWOX(2, true);
                else if (pp.res) DS_TWOX(1, true);
                else DS_TWOX(1, false);
#undef DS_TWOX
            } else {
                const dim3 grid((S.NP / 16 + 3) / 4, (unsigned)Bc);
#define DS_TWO(NT2, RES) hipLaunchKernelGGL((ds::k_two_layer<T, NT2, RES, false>), grid, dim3(256), 0, st, S, c.H2[hi], K2, W2, b2, c.H2[hi ^ 1])
                if (K2o == 32) { if (pp.res) DS_TWO(2, true); else DS_TWO(2, false); }
                else { if (pp.res) DS_TWO(1, true); else DS_TWO(1, false); }
#undef DS_TWO
            }
            if (pp.res_sep)
                hipLaunchKernelGGL((ds::k_pair_res_add<T>), dim3((unsigned)(((size_t)K2o * 5 * S.NP + 255) / 256), (unsigned)Bc), dim3(256), 0, st, c.H2[hi], K2, c.H2[hi ^ 1], K2o,
                                   S.nf, S.NP);
        }
        // one-electron stream layer: GEMM over the N electron tiles + the shared spin-mean tile, then epilogue
        const int Kloc = Kh + S.nch * K2, Ksh = S.nch * Kh;
        {
            dim3 block; unsigned gz;
            gemm_geom(Nout, NB, &block, &gz, ST);
            dim3 wblock; unsigned wgz;                     // geometry of the wide kernels (NB = 4, four waves)
            gemm_geom(Nout, 4, &wblock, &wgz, 6);
            const size_t gws = (size_t)S.N * S.ldk * S.P, gts = (size_t)S.ldk * S.P;
            const bool lr1 = lp.kind == LayerKind::LowRank1;
            T* Sl = lr1 ? c.ZB + (size_t)Bc * S.h1[1] * S.P : c.ZB;      // this layer's shared term
            {
                // shared spin-mean term S (one tile per walker): layer 0 from the MEAN buffer of k_features,
                // hidden layers straight from the electron rows of G (means formed on the fly)
                ProfScope ps(s, DS_PROF_SHARED_TERM, st);
                if (l == 0 || lr1) {
                    // a plain product on ready spin means: those of the input features (MEAN[0], k_features), or -- in front of the
                    // low-rank layer 1 -- those of the layer-0 output (MEAN[1], k_layer0_stats); S of layer 0 stays in front of S of layer 1
                    const ds::GemmArgs<T> ga{nullptr, 0, 0, nullptr, 0, l == 0 ? c.MEAN[0] : c.MEAN[1], (size_t)Ksh * S.P, blk(s->i_wsh[l]), Ksh, 0,
                                             Sl, (size_t)Nout * S.P, 0, Nout, S.P, nullptr, blk(s->i_b[l]), ds::OrbEpi<T>{}};
                    to->gemm(6, dim3(1, (unsigned)Bc, gz), block, st, ga);
                } else {
                    // (its own geometry: as many waves per workgroup as possible, every workgroup re-forms the spin means)
                    dim3 sblock; unsigned sgz;
                    gemm_geom(Nout, NB, &sblock, &sgz);
                    if (ST > 10 && sblock.x > 512) { sblock = dim3(512); sgz = (unsigned)((Nout / (16 * NB) + 7) / 8); }      // (k_shared_term's launch bound for wide slot ranges)
                    to->shared_term(dim3(1, (unsigned)Bc, sgz), sblock, 2 * 16 * S.P * sizeof(T), st, S, c.G[gi], blk(s->i_wsh[l]), Kh, Sl, Nout, S.P,
                                    blk(s->i_b[l]), 0);
                }
            }
            // ... then the N electron tiles with the fused epilogue
            ProfScope ps(s, lp.prof_kind, st);
            // layer input tiles: G[gi], or (layer 0 in front of the low-rank layer 1) the XL buffer
            const T* Xin = (lr_on && l == 0) ? c.XL : c.G[gi];
            const size_t xws = (lr_on && l == 0) ? (size_t)S.N * K0loc * S.P : gws, xts = (lr_on && l == 0) ? (size_t)K0loc * S.P : gts;
            const dim3 lgrid(S.N * gz, (unsigned)Bc, 1), wgrid(S.N * wgz, (unsigned)Bc, 1);
            auto layer_gemm = [&](int epi, const ds::GemmArgs<T>& g) {
                if (lp.wide) to->gemm_wide(epi, wgrid, wblock, st, g); else to->gemm(epi, lgrid, block, st, g);
            };
            ds::GemmArgs<T> ga{Xin, xws, xts, blk(s->i_wloc[l]), Kloc, nullptr, 0, nullptr, 0, S.N, c.G[gi ^ 1], gws, gts, Nout, S.P, c.ZB, blk(s->i_b[l]),
                               ds::OrbEpi<T>{}};
            if (lp.pm_mask) { ga.oe.pm_k0 = Kh / 4; ga.oe.pm_ks = K2 / 4; ga.oe.pm_nup = S.n_up; ga.oe.pm_nch = S.nch; }
            switch (lp.kind) {
            case LayerKind::LowRank1: {
                // first hidden layer on the low-rank form of the layer-0 output (ds_gemm.h: k_layer1_lr)
                const ds::LrArgs<T> la{c.XL, (size_t)S.N * K0loc * S.P, (size_t)K0loc * S.P, c.MEAN[0], (size_t)K0sh * S.P, K0loc, K0sh,
                                       (const T*)s->lr_w0t, c.G[gi], gws, gts, blk(s->i_wloc[l]), Kh, S.nch * K2, c.G[gi ^ 1], gws, gts, Sl,
                                       Nout, S.P, S.N, c.YO, L.YO, blk(s->i_wloc[0]), c.ZB, s->dbg >> 8, S.n_up, S.nch};
                if (lp.wide) to->layer1_lr_wide(lr_nc, s->res1[l], wgrid, wblock, st, la); else to->layer1_lr(lr_nc, s->res1[l], lgrid, block, st, la);
                break;
            }
            case LayerKind::L0Stats:
                // layer 0 without its dense output: (y, oL) per electron + the spin means of the output (ds_gemm.h), in one kernel
                to->layer0_stats(K0loc / 4, dim3(S.nch * (unsigned)((Nout + 63) / 64), (unsigned)Bc), st, S, c.XL, (size_t)S.N * K0loc * S.P,
                                 (size_t)K0loc * S.P, blk(s->i_wloc[0]), c.ZB, Nout, S.P, c.YO, c.MEAN[1]);
                break;
            case LayerKind::L0Epi9Means: {
                // ... or (y, oL) from the layer kernel with the output dropped (EPI 9), then the means per slot chunk (k_layer0_means)
                ga.Z = c.YO; ga.zws = L.YO; ga.zts = (size_t)2 * Nout;
                layer_gemm(9, ga);
                constexpr int STC = 5;
                const unsigned nfb = (unsigned)((Nout + 63) / 64), nck = (unsigned)((S.P / 16 + STC - 1) / STC);
                hipLaunchKernelGGL((ds::k_layer0_means<T, STC>), dim3(S.nch * nfb * nck, (unsigned)Bc), dim3(256), 0, st, S, c.XL,
                                   (size_t)S.N * K0loc * S.P, (size_t)K0loc * S.P, blk(s->i_wloc[0]), K0loc, c.ZB, Nout, S.P, c.YO, c.MEAN[1]);
                break;
            }
            case LayerKind::Int8: {
                // dense residual layer of the 5-slot-tile float64 cells: the per-electron contraction as a 47-bit fixed-point split on the
                // int8 matrix pipe (ds_i8.h); float64 in, float64 out, same shared term, same epilogue
                uint8_t* wp; double* sw;
                i8_prepare(s, l, (const double*)blk(s->i_wloc[l]), Kloc, Nout, st, &wp, &sw);
                const int ntiles = (int)(Bc * S.N);
                const dim3 igrid((unsigned)std::min<int64_t>(ntiles, s->n_cu));
                hipLaunchKernelGGL((ds::i8::k_layer_i8<5, 2>), igrid, dim3(512), ds::i8::lds_bytes(), st, (const double*)c.G[gi], gts, (const uint4*)wp,
                                   (const double*)sw, (const double*)Sl, S.N, (double*)c.G[gi ^ 1], ntiles);
                break;
            }
            case LayerKind::DenseRes:
                ga.oe.dbg = s->dbg & 3;                 // (timing experiments: 1 = no epilogue, 2 = accumulators start at zero)
                ga.oe.g4 = plan.g4;
                if (l > 0 && s->prof_on && (s->prof_only < 0 || s->prof_only == DS_PROF_SINGLE_HIDDEN)) { ga.oe.clk = s->clk_dev; ga.oe.dbg = s->dbg; }
                layer_gemm(2, ga);
                break;
            case LayerKind::Dense:
                layer_gemm(1, ga);
                if (lp.res_sep)
                    hipLaunchKernelGGL((ds::k_layer_res_add<T>), dim3(S.N, (unsigned)Bc), dim3(256), 0, st, Xin, xws, xts, c.G[gi ^ 1], gws, gts, S.nf * S.A, Nout, S.P);
                break;
            }
        }
        gi ^= 1;
        if (l < S.n_double) {
            hi ^= 1;
            if (stop == STOP_H2_1 + l) return copy_out(dr, c.H2[hi], (size_t)S.h2[l + 1] * 5 * S.NP * Bc, st);
        }
    }
    if (stop == STOP_G0 + S.n_layers) return copy_out(dr, c.G[gi], L.G * Bc, st);
    // orbitals: GEMM over the electrons of one spin with the envelope/phase product rule fused in
    const int Kl = S.h1[S.n_layers], K2l = S.h2[S.n_layers];
    if (s->use_last) {
        ProfScope ps(s, DS_PROF_M2_EXPAND, st);
        hipLaunchKernelGGL((ds::k_m2_expand<T>), dim3(S.N, (unsigned)Bc, m2_split<T>(K2l, S.N)), dim3(256), (size_t)(K2l * 5 * S.N + S.nch * K2l * 5) / m2_split<T>(K2l, S.N) * sizeof(T), st, S,
                           c.H2[hi], K2l, c.G[gi], Kl, S.ldk, 0);
    }
    for (int sp = 0; sp < S.nch; ++sp) {
        const int ns = sp == 0 ? S.n_up : S.n_dn, i0 = sp == 0 ? 0 : S.n_up, OC = S.ocols[sp];
        const int Korb = Kl + (s->use_last ? S.nch * K2l : 0);
        dim3 block; unsigned gz;
        gemm_geom(OC, NB, &block, &gz, ST);
        if (s->use_last) {
            ProfScope ps(s, DS_PROF_SHARED_TERM, st);
            to->shared_term(dim3(1, (unsigned)Bc, gz), block, 2 * 16 * S.P * sizeof(T), st, S, c.G[gi], blk(s->i_wsh_orb[sp]), Kl, c.ZB, OC, S.P,
                            (const T*)nullptr, 0);
        }
        ProfScope ps(s, DS_PROF_ORBITAL, st);
        const int ch = S.mat_ch[sp];
        ds::OrbEpi<T> oe{c.Q, c.MOUT, L.MOUT, L.mout_off[ch], S.N, i0, S.nparam[sp], S.nparam_max, S.norb[sp], S.det_n[ch],
                         S.row_off[sp], S.bias_orb ? blk(s->i_borb[sp]) : (const T*)nullptr, nullptr};
        oe.g4 = plan.g4;      // (the launchers fall back to 16-column products where they have no such instance)
        const ds::GemmArgs<T> ga{c.G[gi] + (size_t)i0 * S.ldk * S.P, (size_t)S.N * S.ldk * S.P, (size_t)S.ldk * S.P, blk(s->i_worb[sp]), Korb,
                                 nullptr, 0, nullptr, 0, ns, nullptr, 0, 0, OC, S.P, s->use_last ? (const T*)c.ZB : (const T*)nullptr, nullptr, oe};
        dim3 ob; unsigned oz;      // geometry of the 48-column waves / of the wide kernel
        switch (plan.orb[sp]) {
        case OrbKind::Orb3:
            gemm_geom(OC, 3, &ob, &oz);
            to->gemm_orb3(dim3(ns * oz, (unsigned)Bc, 1), ob, st, ga);
            break;
        case OrbKind::Wide:
            gemm_geom(OC, 4, &ob, &oz, 6);
            to->gemm_wide(5, dim3(ns * oz, (unsigned)Bc, 1), ob, st, ga);
            break;
        case OrbKind::Ldsb:
            to->orbital_lb(dim3(ns * (unsigned)(OC / 64), (unsigned)Bc, 1), st, ga);
            break;
        case OrbKind::Gemm:
            to->gemm(5, dim3(ns * gz, (unsigned)Bc, 1), block, st, ga);
            break;
        }
    }
    if (stop == STOP_MOUT) return copy_out(dr, c.MOUT, L.MOUT * Bc, st);
    // determinants (ch = determinant channel)
    for (int ch = 0; ch < S.n_detch; ++ch) {
        ProfScope ps(s, DS_PROF_DET_INVERSE, st);
        launch_det_inverse<T>(s, S, c, ch, Bc, st);
    }
    if (stop == STOP_MINV) return copy_out(dr, c.MINV, L.MINV * Bc, st);
    for (int ch = 0; ch < S.n_detch; ++ch) {
        ProfScope ps(s, DS_PROF_DET_TRACE, st);
        if (int rc = launch_det_trace<T>(s, S, c, ch, Bc, st)) return rc;
    }
    if (stop == STOP_DETS) return copy_out(dr, c.DETS, L.DETS * Bc, st);
    if (stop == STOP_TR) return copy_out(dr, c.TR, L.TR * Bc, st);
    {
        ProfScope ps(s, DS_PROF_COMBINE, st);
        hipLaunchKernelGGL((ds::k_combine<T>), dim3((unsigned)Bc), dim3(64), 0, st, S, c.TR, L.TR, L.tr_off[1], c.DETS, L.DETS,
                           L.dets_off[1], out_ke, out_logabs, out_phase, out_grad);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// The value chain (log psi / orbital matrices) on a chunk of Bc walkers.
template <typename T>
int run_value_chain(ds_system* s, const T* params, const T* x, int64_t Bc, const ValBufs<T>& vb, hipStream_t st, T* out_logabs,
                    T* out_phase) {
    const ds::SysDev<T>& S = dev<T>(s);
    const WsLayout& L = s->wsv;
    const int PV = ds::PV;
    const int64_t ng = (Bc + PV - 1) / PV;
    T* ZB = vb.ZB; T* Q = vb.Q; T* MOUT = vb.MOUT; T* DETS = vb.DETS;
    auto blk = [&](int i) { return params + s->blocks[i].offset; };
    // workgroups per 80-walker group: at least FV_SPLIT, and enough for ~2048 workgroups in all (13 groups of diamond walkers
    // x 16 were 208 workgroups looping 180 times each)
    const unsigned fsplit = (unsigned)std::min<int64_t>(256, std::max<int64_t>(ds::FV_SPLIT, (2048 + ng - 1) / ng));
    hipLaunchKernelGGL((ds::k_features_val<T, 0>), dim3((unsigned)ng, fsplit), dim3(256), 0, st, S, x, (long)Bc, blk(s->i_pi[0]),
                       blk(s->i_sg[0]), blk(s->i_pi[S.nch - 1]), blk(s->i_sg[S.nch - 1]), vb.Gl[0], vb.MEAN0, vb.H2l[0], Q);
    hipLaunchKernelGGL((ds::k_features_val<T, 1>), dim3((unsigned)ng, fsplit), dim3(256), 0, st, S, x, (long)Bc, blk(s->i_pi[0]),
                       blk(s->i_sg[0]), blk(s->i_pi[S.nch - 1]), blk(s->i_sg[S.nch - 1]), vb.Gl[0], vb.MEAN0, vb.H2l[0], Q);
    const size_t gws = (size_t)S.N * S.ldk * PV, gts = (size_t)S.ldk * PV;
    // (a first pair layer with a residual -- added behind the layer by k_pair_res_add -- has no segment sums of its final output)
    const bool fuse_means = S.n_up >= 8 && (S.n_dn >= 8 || S.n_dn == 0) && !(S.n_double >= 1 && s->res2[0]);
    // log psi only: every pair layer in one launch, activations in registers (k_pair_stream_val).  Needs equal pair widths with a
    // kernel instance, no residual on the first pair layer (its input has another width anyway) and the segment sums as the only
    // consumer of the pair stream.  The sums of layer l go to vb.PM[l] (carve_value).
    bool fuse_pairs = fuse_means && !vb.keep && s->use_pair_fuse && S.n_double >= 1 && S.n_double <= ds::PS_MAX_LAYERS && !s->res2[0] &&
                      S.h2[0] % 4 == 0 && (S.h2[1] == 16 || S.h2[1] == 32) && vb.pm_fit;
    for (int l = 1; l < S.n_double; ++l) fuse_pairs = fuse_pairs && S.h2[l + 1] == S.h2[1];
    auto pm_of = [&](int l) -> T* { return fuse_pairs ? vb.PM[l] : vb.PARTM; };
    if (fuse_pairs) {
        ds::PairStreamArgs<T> pa{};
        pa.H0 = vb.H2l[0]; pa.Kin0 = S.h2[0]; pa.nl = S.n_double;
        for (int l = 0; l < S.n_double; ++l) { pa.W[l] = blk(s->i_w2[l]); pa.b[l] = blk(s->i_b2[l]); pa.res[l] = s->res2[l] ? 1 : 0; pa.PM[l] = pm_of(l); }
        dim3 grid((S.NP / 16 + 3) / 4, (unsigned)(ng * (PV / 5)));
        if (S.h2[1] == 32) hipLaunchKernelGGL((ds::k_pair_stream_val<T, 2>), grid, dim3(256), 0, st, S, pa);
        else hipLaunchKernelGGL((ds::k_pair_stream_val<T, 1>), grid, dim3(256), 0, st, S, pa);
    }
    for (int l = 0; l < S.n_layers; ++l) {
        const int Kh = S.h1[l], K2 = S.h2[l], Nout = S.h1[l + 1];
        T* Gin = vb.Gl[l]; T* Gout = vb.Gl[l + 1];
        // the pair stream stops changing after the last two-electron layer
        T* Hin = vb.H2l[l < S.n_double ? l : S.n_double];
        // partner means of the pair stream -> rows [Kh, Kh + nch*K2): layer 0 from H2 itself; later layers from the segment sums
        // the previous pair layer left behind (no second pass over H2) when every spin has >= 8 electrons
        if (l > 0 && l <= S.n_double && fuse_means)
            hipLaunchKernelGGL((ds::k_m2_combine_val<T>), dim3(S.N, (unsigned)ng, (unsigned)(S.nch * K2 / m2_rc(K2))), dim3(256), (size_t)m2_rc(K2) * PV * sizeof(T), st, S, pm_of(l - 1), K2, Gin, Kh, m2_rc(K2));
        else
            hipLaunchKernelGGL((ds::k_m2_expand_val<T>), dim3(S.N, (unsigned)ng), dim3(256), 0, st, S, Hin, K2, Gin, Kh);
        if (l < S.n_double && !fuse_pairs) {
            const int K2o = S.h2[l + 1];
            if (K2o != 32 && K2o != 16) return fail("hidden_double must be 16 or 32 (got %d)", K2o);
            dim3 grid((S.NP / 16 + 3) / 4, (unsigned)(ng * (PV / 5)));
            const bool res_sep = s->res2[l] && l == 0;
            const bool res = s->res2[l] && !res_sep;
            const T* W2 = blk(s->i_w2[l]); const T* b2 = blk(s->i_b2[l]);
            // the last pair layer's output is only needed as means unless the activations are kept (gradient pass) or the
            // orbital head / a later layer reads H2 again without a pair layer in between
            T* Hnext = (fuse_means && !vb.keep && l + 1 == S.n_double) ? (T*)nullptr : vb.H2l[l + 1];
            T* pmv = fuse_means ? vb.PARTM : (T*)nullptr;
#define DS_TWO(NT2, RES) hipLaunchKernelGGL((ds::k_two_layer<T, NT2, RES, true>), grid, dim3(256), 0, st, S, Hin, K2, W2, b2, Hnext, pmv)
            if (K2o == 32) { if (res) DS_TWO(2, true); else DS_TWO(2, false); }
            else { if (res) DS_TWO(1, true); else DS_TWO(1, false); }
#undef DS_TWO
            if (res_sep)
                hipLaunchKernelGGL((ds::k_pair_res_add<T>), dim3((unsigned)(((size_t)K2o * 5 * S.NP + 255) / 256), (unsigned)(ng * (PV / 5))), dim3(256), 0, st, Hin, K2, Hnext, K2o,
                                   S.nf, S.NP);
        }
        if (Nout % 64 || Nout > 1024) return fail("hidden_single must be a multiple of 64 and <= 1024 (got %d)", Nout);
        const int Kloc = Kh + S.nch * K2, Ksh = S.nch * Kh;
        const bool res_sep = s->res1[l] && l == 0 && (Kloc % 16 != 0 || S.nf * S.A != Nout);      // (see plan_chain)
        if (s->res1[l] && !res_sep && Kloc % 16) return fail("residual layer with K = %d: the GEMM's operand ring needs K %% 16 == 0", Kloc);
        dim3 block; unsigned gz;
        gemm_geom(Nout, 4, &block, &gz);
        // (a float32 MFMA lasts half as long: the same rule on half the count -- diamond, 1024 walkers: forward 3.46 -> 3.40 ms)
        const int nbh = val_nb(s->val_nb, (int64_t)S.N * ng * gz / (sizeof(T) == 4 ? 2 : 1));
        if (l == 0)
            hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 7>), dim3(1, (unsigned)ng, gz), block, 0, st, (const T*)nullptr, (size_t)0, (size_t)0,
                               (const T*)nullptr, 0, vb.MEAN0, (size_t)Ksh * PV, blk(s->i_wsh[l]), Ksh, 0, ZB, (size_t)Nout * PV, (size_t)0, Nout, PV,
                               (const T*)nullptr, blk(s->i_b[l]), ds::OrbEpi<T>{});
        else {
            // hidden layers: spin means over the electrons in a bandwidth-bound pass that fills the chip (a group is one
            // workgroup's worth of GEMM), then the shared term as a K = nch*Kh product on them
            hipLaunchKernelGGL((ds::k_spin_mean<T>), dim3((unsigned)((Ksh * PV + 255) / 256), (unsigned)ng), dim3(256), 0, st, S, Gin, Kh, vb.MEANS);
            // one tile per 80-walker group: with 64-feature waves a 4096-walker batch is 208 waves on 1024 SIMDs, each a serial chain
            // of Ksh/4 x 20 MFMAs (75 us at Ksh = 512).  16-feature waves in 64-feature workgroups: four times the waves on four
            // times the CUs, a quarter of the chain each (same products in the same order: bit-identical)
            // few groups: 16-walker column blocks as well (grid.x; operand and output advance by 16 columns per block), five times
            // the waves with a fifth of the chain
            if (nbh < 4 && Ksh % 16 == 0)
                hipLaunchKernelGGL((ds::k_jet_gemm<T, 1, 1, 7>), dim3(PV / 16, (unsigned)ng, (unsigned)(Nout / 64)), dim3(256), 0, st, (const T*)nullptr, (size_t)0, (size_t)16,
                                   (const T*)nullptr, 0, vb.MEANS, (size_t)Ksh * PV, blk(s->i_wsh[l]), Ksh, 0, ZB, (size_t)Nout * PV, (size_t)16, Nout, PV,
                                   (const T*)nullptr, blk(s->i_b[l]), ds::OrbEpi<T>{});
            else
                hipLaunchKernelGGL((ds::k_jet_gemm<T, 1, 5, 7>), dim3(1, (unsigned)ng, (unsigned)(Nout / 64)), dim3(256), 0, st, (const T*)nullptr, (size_t)0, (size_t)0,
                                   (const T*)nullptr, 0, vb.MEANS, (size_t)Ksh * PV, blk(s->i_wsh[l]), Ksh, 0, ZB, (size_t)Nout * PV, (size_t)0, Nout, PV,
                                   (const T*)nullptr, blk(s->i_b[l]), ds::OrbEpi<T>{});
        }
#define DS_VHID(NBV) { dim3 hb; unsigned hz; val_geom(Nout, NBV, &hb, &hz); \
            hipLaunchKernelGGL((ds::k_jet_gemm<T, NBV, 5, 4>), dim3(S.N, (unsigned)ng, hz), hb, (ds::gemm_stash_bytes<T, NBV, 5>(hb.x)), st, Gin, gws, gts, blk(s->i_wloc[l]), Kloc, \
                               (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, S.N, Gout, gws, gts, Nout, PV, ZB, blk(s->i_b[l]), ds::OrbEpi<T>{}); }
        // residual hidden layers of the 256-feature networks with enough (group, electron) tiles to give every CU's persistent workgroup
        // two or more: the int8 split of the forward-Laplacian chain (ds_i8.h) with the value epilogue -- 43 us per tile against the
        // float64 MFMA kernel's 73 (the float64 MFMA shares the FP64 datapath with the tanh polynomials, the int8 MFMA does not)
        if (sizeof(T) == 8 && int8_value_layer(s, l) && (int64_t)S.N * ng >= (int64_t)s->val_i8_min_tiles) {
            uint8_t* wp; double* sw;
            i8_prepare(s, l, (const double*)blk(s->i_wloc[l]), Kloc, Nout, st, &wp, &sw);
            const int ntiles = (int)(S.N * ng);
            hipLaunchKernelGGL((ds::i8::k_layer_i8<5, 4>), dim3((unsigned)std::min<int64_t>(ntiles, s->n_cu)), dim3(512), ds::i8::lds_bytes(), st, (const double*)Gin, gts,
                               (const uint4*)wp, (const double*)sw, (const double*)ZB, S.N, (double*)Gout, ntiles);
        } else if (s->res1[l] && !res_sep) {
            if (nbh == 4) DS_VHID(4) else if (nbh == 2) DS_VHID(2) else DS_VHID(1)
        } else {
#undef DS_VHID
            hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 3>), dim3(S.N, (unsigned)ng, gz), block, 0, st, Gin, gws, gts, blk(s->i_wloc[l]), Kloc,
                               (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, S.N, Gout, gws, gts, Nout, PV, ZB, blk(s->i_b[l]), ds::OrbEpi<T>{});
            if (res_sep)
                hipLaunchKernelGGL((ds::k_layer_res_add<T>), dim3(S.N, (unsigned)ng), dim3(256), 0, st, (const T*)Gin, gws, gts, Gout, gws, gts, S.nf * S.A, Nout, PV);
        }
    }
    T* Gl = vb.Gl[S.n_layers];
    const int Kl = S.h1[S.n_layers], K2l = S.h2[S.n_layers];
    if (s->use_last) {
        if (fuse_means) hipLaunchKernelGGL((ds::k_m2_combine_val<T>), dim3(S.N, (unsigned)ng, (unsigned)(S.nch * K2l / m2_rc(K2l))), dim3(256), (size_t)m2_rc(K2l) * PV * sizeof(T), st, S, pm_of(S.n_double - 1), K2l, Gl, Kl, m2_rc(K2l));
        else hipLaunchKernelGGL((ds::k_m2_expand_val<T>), dim3(S.N, (unsigned)ng), dim3(256), 0, st, S, vb.H2l[S.n_double], K2l, Gl, Kl);
    }
    for (int sp = 0; sp < S.nch; ++sp) {
        const int ns = sp == 0 ? S.n_up : S.n_dn, i0 = sp == 0 ? 0 : S.n_up, OC = S.ocols[sp];
        const int Korb = Kl + (s->use_last ? S.nch * K2l : 0);
        if (Korb % 16) return fail("orbital head with K = %d: the GEMM's operand ring needs K %% 16 == 0", Korb);
        dim3 oblock; unsigned ogz;
        gemm_geom(OC, 4, &oblock, &ogz);
        T* Sorb = vb.SORB[sp];
        if (s->use_last)
            hipLaunchKernelGGL((ds::k_shared_term<T, 4, 5>), dim3(1, (unsigned)ng, ogz), oblock, 2 * 16 * PV * sizeof(T), st, S, Gl,
                               blk(s->i_wsh_orb[sp]), Kl, Sorb, OC, PV, (const T*)nullptr, 0);
        if (vb.keep) {
            // gradient pass: the raw products PHI are kept (k_orbital_bwd reads them), the product with q is its own kernel
            hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 0>), dim3(ns, (unsigned)ng, ogz), oblock, 0, st, Gl + (size_t)i0 * S.ldk * PV,
                               gws, gts, blk(s->i_worb[sp]), Korb, (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, ns, vb.PHI[sp], (size_t)ns * OC * PV, (size_t)0,
                               OC, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            if (MOUT)
                hipLaunchKernelGGL((ds::k_orbital_epilogue_val<T>), dim3(ns, (unsigned)ng), dim3(256), 0, st, S, vb.PHI[sp], (size_t)ns * OC * PV, Q, MOUT, sp,
                                   L.MOUT, L.mout_off[S.mat_ch[sp]], S.bias_orb ? blk(s->i_borb[sp]) : (const T*)nullptr,
                                   s->use_last ? (const T*)Sorb : (const T*)nullptr);
            continue;
        }
        // log psi only: the product with the envelope x phase factor q is the GEMM's epilogue (EPI 8): no PHI buffer, no second kernel
        ds::OrbEpi<T> oe{Q, MOUT, L.MOUT, L.mout_off[S.mat_ch[sp]], S.N, i0, S.nparam[sp], S.nparam_max, S.norb[sp], S.det_n[S.mat_ch[sp]],
                         S.row_off[sp], S.bias_orb ? blk(s->i_borb[sp]) : (const T*)nullptr, nullptr};
#define DS_VORB(NBV, BLK, GZ) hipLaunchKernelGGL((ds::k_jet_gemm<T, NBV, 5, 8>), dim3(ns, (unsigned)ng, GZ), BLK, 0, st, Gl + (size_t)i0 * S.ldk * PV, \
                           gws, gts, blk(s->i_worb[sp]), Korb, (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, ns, (T*)nullptr, (size_t)0, (size_t)0, \
                           OC, PV, s->use_last ? (const T*)Sorb : (const T*)nullptr, (const T*)nullptr, oe)
        // 192 columns would be three 64-column waves per workgroup: 48-column waves give four balanced ones (as in the
        // forward-Laplacian chain's orbital head): 131 -> 94 us per 4096 bcc-Li walkers
        const bool w48 = OC % 256 != 0 && OC % 192 == 0;
        const int nbo = val_nb(s->val_nb, (int64_t)ns * ng * (w48 ? OC / 192 : ogz) / (sizeof(T) == 4 ? 2 : 1));
        if (nbo < 4) DS_VORB(1, dim3(256), (unsigned)((OC + 63) / 64));
        else if (w48) DS_VORB(3, dim3(256), (unsigned)(OC / 192));
        else DS_VORB(4, oblock, ogz);
#undef DS_VORB
    }
    if (out_logabs || out_phase || vb.MINV) {
        const size_t dstride = s->ws.DETS;
        for (int sp = 0; sp < S.n_detch; ++sp) {
            const int n = S.det_n[sp];
            if (!vb.MINV && n <= 16) {              // log det only: register LU, four lanes per matrix
                // both determinant channels in one launch when they take the same instance (a channel alone is 64 workgroups
                // per 512 walkers -- a latency chain on a quarter of the chip)
                auto rof = [](int m) { return m <= 4 ? 1 : (m <= 8 ? 2 : (m <= 12 ? 3 : 4)); };
                const bool both = sp + 1 < S.n_detch && S.det_n[sp + 1] <= 16 && rof(S.det_n[sp + 1]) == rof(n);
                const dim3 lgrid(S.K, (unsigned)((Bc + 63) / 64), both ? 2 : 1);
                const ds::DetOff2 off{{L.mout_off[sp], both ? L.mout_off[sp + 1] : 0}, {s->ws.dets_off[sp], both ? s->ws.dets_off[sp + 1] : 0}};
#define DS_LU(RV) hipLaunchKernelGGL((ds::k_det_lu_val<T, RV>), lgrid, dim3(256), 0, st, S, MOUT, L.MOUT, off, sp, (long)Bc, DETS, dstride)
                if (n <= 4) DS_LU(1); else if (n <= 8) DS_LU(2); else if (n <= 12) DS_LU(3); else DS_LU(4);
#undef DS_LU
                if (both) ++sp;
                continue;
            }
            if (!vb.MINV && n <= (sizeof(T) == 4 ? 64 : 48) && !s->no_lu_wave) {      // log det only, one lane per row (float64: 48 x 2 x 2 VGPRs per row)
                const dim3 wgrid(S.K, (unsigned)Bc);
#define DS_LUW(NCV) hipLaunchKernelGGL((ds::k_det_lu_wave<T, NCV>), wgrid, dim3(64), 0, st, S, MOUT, L.MOUT, L.mout_off[sp], sp, (long)Bc, DETS, dstride, \
                                       s->ws.dets_off[sp])
                if (n <= 24) DS_LUW(24); else if (n <= 32) DS_LUW(32); else if (n <= 48) DS_LUW(48); else DS_LUW((sizeof(T) == 4 ? 64 : 48));
#undef DS_LUW
                continue;
            }
            size_t sh = (size_t)n * 2 * n * sizeof(ds::Cx<T>) + 16;
            hipLaunchKernelGGL((ds::k_det_inverse<T>), dim3(S.K, (unsigned)Bc), dim3(64), sh, st, S, MOUT, L.MOUT, L.mout_off[sp], sp,
                               vb.MINV, L.MOUT, L.mout_off[sp], DETS, dstride, s->ws.dets_off[sp], PV, PV, PV, PV);
        }
        if (out_logabs || out_phase)
            hipLaunchKernelGGL((ds::k_combine_val<T>), dim3((unsigned)((Bc + 255) / 256)), dim3(256), 0, st, S, DETS, dstride, s->ws.dets_off[1], (long)Bc,
                               out_logabs, out_phase);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int logpsi_impl(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* ws, int64_t ws_bytes,
                hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int64_t cg = groups_that_fit(ws_bytes, sizeof(T), PassSize{0, s->wsv.per_walker});
    if (cg < 1) return fail("workspace too small for the value chain: %lld bytes < %zu per group", (long long)ws_bytes, s->wsv.per_walker * sizeof(T));
    const int64_t chunk = cg * ds::PV;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t Bc = std::min(chunk, B - b0);
        Arena<T> a = arena_of<T>(ws, ws_bytes);
        const ValBufs<T> vb = carve_value<T>(s, a, (Bc + ds::PV - 1) / ds::PV);
        if (!a.ok) return carve_fail("value chain");
        int rc = run_value_chain<T>(s, (const T*)params, (const T*)x + b0 * 3 * S.N, Bc, vb, st, out_logabs ? (T*)out_logabs + b0 : nullptr,
                                    out_phase ? (T*)out_phase + 2 * b0 : nullptr);
        if (rc) return rc;
    }
    return 0;
}

template <typename T>
int orbitals_impl(ds_system* s, const void* params, const void* x, int64_t B, void* out_up, void* out_dn, void* ws, int64_t ws_bytes,
                  hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int64_t cg = groups_that_fit(ws_bytes, sizeof(T), PassSize{0, s->wsv.per_walker});
    if (cg < 1) return fail("workspace too small for the value chain");
    const int64_t chunk = cg * ds::PV;
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t Bc = std::min(chunk, B - b0);
        Arena<T> a = arena_of<T>(ws, ws_bytes);
        const ValBufs<T> vb = carve_value<T>(s, a, (Bc + ds::PV - 1) / ds::PV);
        if (!a.ok) return carve_fail("value chain");
        T* mout = vb.MOUT;
        int rc = run_value_chain<T>(s, (const T*)params, (const T*)x + b0 * 3 * S.N, Bc, vb, st, nullptr, nullptr);
        if (rc) return rc;
        for (int sp = 0; sp < S.n_detch; ++sp) {
            const int n = S.det_n[sp];
            T* o = (T*)(sp == 0 ? out_up : out_dn);
            if (!o) continue;
            const size_t per = (size_t)S.K * n * n * 2;
            hipLaunchKernelGGL((ds::k_gather_val<T>), dim3((unsigned)((per + 255) / 256), (unsigned)Bc), dim3(256), 0, st, mout, s->wsv.MOUT,
                               s->wsv.mout_off[sp], per, (long)b0, (long)Bc, o);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int local_energy_impl(ds_system* s, const void* params, const void* x, int64_t B, void* out_ke, void* out_ewald, void* out_logabs,
                      void* out_phase, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    int64_t chunk = ws_bytes / (int64_t)(s->ws.per_walker * sizeof(T));
    if (chunk < 1) return fail("workspace too small: %lld bytes < %zu per walker", (long long)ws_bytes, s->ws.per_walker * sizeof(T));
    chunk = std::min<int64_t>(chunk, 65535);      // grid.y carries the walker index
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t Bc = std::min(chunk, B - b0);
        const T* xb = (const T*)x + b0 * 3 * S.N;
        int rc = run_chain<T>(s, (const T*)params, xb, Bc, arena_of<T>(ws, ws_bytes), st, out_ke ? (T*)out_ke + 2 * b0 : nullptr,
                              out_logabs ? (T*)out_logabs + b0 : nullptr, out_phase ? (T*)out_phase + 2 * b0 : nullptr, nullptr);
        if (rc) return rc;
    }
    if (out_ewald) {
        // ee + ei + ii summed into one number per walker by a tiny epilogue: reuse the workspace head
        T* tmp = (T*)ws;
        for (int64_t b0 = 0; b0 < B; b0 += chunk) {
            const int64_t Bc = std::min(chunk, B - b0);
            size_t sh = ds::ewald_lds_bytes(S);
            ProfScope ps(s, DS_PROF_EWALD, st);
            hipLaunchKernelGGL((ds::k_ewald<T>), dim3((unsigned)Bc), dim3(256), sh, st, S, (const T*)x + b0 * 3 * S.N, tmp);
            hipLaunchKernelGGL((ds::k_sum3<T>), dim3((unsigned)((Bc + 255) / 256)), dim3(256), 0, st, tmp, Bc, (T*)out_ewald + b0);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int logpsi_grad_impl(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* out_grad,
                     void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int64_t chunk = std::min<int64_t>(ws_bytes / (int64_t)(s->ws.per_walker * sizeof(T)), 65535);
    if (chunk < 1) return fail("workspace too small");
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t Bc = std::min(chunk, B - b0);
        int rc = run_chain<T>(s, (const T*)params, (const T*)x + b0 * 3 * S.N, Bc, arena_of<T>(ws, ws_bytes), st, nullptr, out_logabs ? (T*)out_logabs + b0 : nullptr,
                              out_phase ? (T*)out_phase + 2 * b0 : nullptr, nullptr, (T*)out_grad + b0 * 3 * S.N * 2);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ parameter gradient (reverse sweep, ds_grad.h)
struct GradPlan {
    size_t wt_total;                 // transposed weights, shared by all groups (elements)
    size_t wlocT[DS_MAX_LAYERS], wshT[DS_MAX_LAYERS], worbT[2];
    int kpad[DS_MAX_LAYERS];         // rows of W * ZBAR per layer (Kloc rounded up to the GEMM's 64-feature blocks)
    size_t phi_off[2], phi_total, gbar, hb, h2, w2s, sbar, wshorbT[2];
    int korb, korb_pad;                // rows of the orbital-head input (with use_last_layer: h | pair means) and padded
};

int grad_plan(const ds_system* s, GradPlan* gp) {
    const ds::SysDev<double>& S = s->sd;
    const size_t PV = ds::PV;
    if (S.n_double != (s->use_last ? S.n_layers : S.n_layers - 1)) return fail("parameter gradient: unexpected layer counts");
    size_t off = 0;
    int h1max = 0, h2max = 0, ocmax = 0;
    for (int l = 0; l <= S.n_layers; ++l) { h1max = std::max(h1max, S.h1[l]); h2max = std::max(h2max, S.h2[l]); }
    const int Kl = S.h1[S.n_layers];
    gp->korb = Kl + (s->use_last ? S.nch * S.h2[S.n_layers] : 0);
    gp->korb_pad = s->use_last ? rup(gp->korb, 64) : Kl;
    int kpmax = gp->korb_pad;
    for (int l = 0; l < S.n_layers; ++l) {
        const int Kh = S.h1[l], Nout = S.h1[l + 1], Kloc = Kh + S.nch * S.h2[l];
        gp->kpad[l] = rup(Kloc, 64);
        gp->wlocT[l] = off; if (l > 0) off += (size_t)Nout * gp->kpad[l];
        gp->wshT[l] = off; if (l > 0) off += (size_t)Nout * S.nch * Kh;
        if (l > 0) kpmax = std::max(kpmax, gp->kpad[l]);
    }
    for (int c = 0; c < S.nch; ++c) {
        gp->worbT[c] = off; off += (size_t)S.ocols[c] * gp->korb_pad;
        gp->wshorbT[c] = off; if (s->use_last) off += (size_t)S.ocols[c] * S.nch * Kl;
        ocmax = std::max(ocmax, S.ocols[c]);
    }
    gp->wt_total = rup(off, 16);
    size_t phi = 0;
    for (int c = 0; c < S.nch; ++c) { gp->phi_off[c] = phi; phi += (size_t)(c == 0 ? S.n_up : S.n_dn) * S.ocols[c] * PV; }
    gp->phi_total = phi;
    gp->gbar = (size_t)S.N * kpmax * PV;
    gp->hb = (size_t)S.N * h1max * PV;
    gp->h2 = (size_t)(PV / 5) * h2max * 5 * S.NP;
    gp->w2s = (size_t)(PV / 5) * h2max * h2max;
    gp->sbar = (size_t)std::max(h1max, ocmax) * PV;
    return 0;
}

// A gradient pass has three parts, shared by its three entry points (ds_logpsi_vjp, ds_kfac_factors, ds_pretrain_loss_vjp):
//   1. run_value_chain with every activation kept (buffers: carve_grad),
//   2. a seed that fills PHIBAR / QBAR (seed_logdet: cotangent of log psi; seed_mse: residual of the orbital-matching loss),
//   3. sweep_from_seed: PHIBAR / QBAR -> every parameter's partial sums -> grad.
template <typename T> struct GradBufs {
    ValBufs<T> vb;
    T *MEANL, *MEANBAR, *MEANBAR2, *QBAR, *PB[2], *CW, *GBAR, *HB[2], *ZBAR, *SBAR, *H2BAR[2], *Z2BAR, *PART, *W2S;
};

template <typename T>
GradBufs<T> carve_grad(const ds_system* s, const GradPlan& gp, Arena<T>& a, int64_t ng) {
    const ds::SysDev<double>& S = s->sd;      // (the dims of sd and sf are the same)
    const WsLayout& V = s->wsv;
    const size_t PV = ds::PV;
    const int L = S.n_layers;
    GradBufs<T> b{};
    ValBufs<T>& vb = b.vb;
    vb.keep = true;
    for (int l = 0; l <= L; ++l) vb.Gl[l] = a.take(V.G * ng);
    for (int l = 0; l <= S.n_double; ++l) vb.H2l[l] = a.take(gp.h2 * ng);
    for (int l = S.n_double + 1; l <= L; ++l) vb.H2l[l] = vb.H2l[S.n_double];
    vb.MEAN0 = a.take(V.MEAN * ng);
    b.MEANL = a.take(V.MEAN * ng);
    vb.MEANS = b.MEANL;                       // forward scratch; the reverse sweep refills it layer by layer
    b.MEANBAR = a.take(V.MEAN * ng);
    vb.ZB = a.take(V.ZB * ng);
    vb.Q = a.take(V.Q * ng); b.QBAR = a.take(V.Q * ng);
    vb.MOUT = a.take(V.MOUT * ng); vb.MINV = a.take(V.MOUT * ng);
    vb.DETS = a.take(V.DETS * ng); vb.PARTM = a.take(V.PARTM * ng);
    T* const phi = a.take(gp.phi_total * ng);
    T* const pb = a.take(gp.phi_total * ng);
    for (int c = 0; c < S.nch; ++c) { vb.PHI[c] = phi + gp.phi_off[c] * ng; b.PB[c] = pb + gp.phi_off[c] * ng; }
    b.CW = a.take((size_t)S.K * 2 * PV * ng);
    b.GBAR = a.take(gp.gbar * ng);
    for (T*& h : b.HB) h = a.take(gp.hb * ng);
    b.ZBAR = a.take(gp.hb * ng);
    b.SBAR = a.take(gp.sbar * ng);
    for (T*& h : b.H2BAR) h = a.take(gp.h2 * ng);
    b.Z2BAR = a.take(gp.h2 * ng);
    b.PART = a.take((size_t)s->nparams * ng);
    b.W2S = a.take(gp.w2s * ng);              // split partials of the pair-stream weight gradients
    if (s->use_last) {
        b.MEANBAR2 = a.take(V.MEAN * ng);
        for (int c = 0; c < S.nch; ++c) vb.SORB[c] = a.take((size_t)S.ocols[c] * PV * ng);
    }
    return b;
}

// transposed, zero-padded weights for the W * ZBAR products of the sweep, shared by all groups
template <typename T>
void grad_transposes(ds_system* s, const GradPlan& gp, const T* params, T* WT, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    auto blk = [&](int i) { return params + s->blocks[i].offset; };
    const int L = S.n_layers, Kl = S.h1[L];
    auto transpose = [&](const T* W, int rows, int cols, T* out, int ldt) {
        const size_t n = (size_t)cols * ldt;
        hipLaunchKernelGGL((ds::k_transpose_pad<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, rows, cols, out, ldt);
    };
    for (int l = 1; l < L; ++l) {
        const int Kh = S.h1[l], Nout = S.h1[l + 1], Kloc = Kh + S.nch * S.h2[l];
        transpose(blk(s->i_wloc[l]), Kloc, Nout, WT + gp.wlocT[l], gp.kpad[l]);
        transpose(blk(s->i_wsh[l]), S.nch * Kh, Nout, WT + gp.wshT[l], S.nch * Kh);
    }
    for (int c = 0; c < S.nch; ++c) {
        transpose(blk(s->i_worb[c]), gp.korb, S.ocols[c], WT + gp.worbT[c], gp.korb_pad);
        if (s->use_last) transpose(blk(s->i_wsh_orb[c]), S.nch * Kl, S.ocols[c], WT + gp.wshorbT[c], S.nch * Kl);
    }
}

// Seed of the log-psi VJP: determinants -> orbital head.  `cot`: (Bc, 2) cotangents of this chunk's walkers
template <typename T>
int seed_logdet(ds_system* s, const GradPlan& gp, const GradBufs<T>& gb, const T* params, const T* cot, int64_t Bc, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const WsLayout& V = s->wsv;
    const int PV = ds::PV;
    const int64_t ng = (Bc + PV - 1) / PV;
    const ValBufs<T>& vb = gb.vb;
    auto blk = [&](int i) { return params + s->blocks[i].offset; };
    hipLaunchKernelGGL((ds::k_det_weights<T>), dim3((unsigned)((ng * PV + 63) / 64)), dim3(64), 0, st, S, vb.DETS, s->ws.DETS,
                       s->ws.dets_off[1], cot, (long)Bc, gb.CW);
    for (int sp = 0; sp < S.nch; ++sp) {
        const int ns = sp == 0 ? S.n_up : S.n_dn;
        const size_t pgs = (size_t)ns * S.ocols[sp] * PV;
        HIP_OK(hipMemsetAsync(gb.PB[sp], 0, pgs * ng * sizeof(T), st));
        hipLaunchKernelGGL((ds::k_orbital_bwd<T>), dim3(ns, (unsigned)ng), dim3(256), 0, st, S, vb.PHI[sp], pgs, vb.Q, vb.MINV, V.MOUT,
                           V.mout_off[S.mat_ch[sp]], gb.CW, sp, (long)Bc, S.bias_orb ? blk(s->i_borb[sp]) : (const T*)nullptr,
                           s->use_last ? (const T*)vb.SORB[sp] : (const T*)nullptr, gb.PB[sp], gb.QBAR);
    }
    return 0;
}

// Seed of the orbital-matching loss (reference pretrain.py:70-94), ds_grad.h: k_orbital_bwd_mse.  `tgt[sp]`: this chunk's
// walkers of the spin's target; `B_total`: walkers of the whole call (the mean runs over all of them); LPART: N * ng loss
// partials, added to out_loss[0] (overwritten when `first`)
template <typename T>
int seed_mse(ds_system* s, const GradPlan& gp, const GradBufs<T>& gb, const T* params, const T* const tgt[2], int64_t Bc,
             int64_t B_total, T* LPART, bool first, double* out_loss, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int PV = ds::PV;
    const int64_t ng = (Bc + PV - 1) / PV;
    const ValBufs<T>& vb = gb.vb;
    auto blk = [&](int i) { return params + s->blocks[i].offset; };
    // the reference's list has one entry per active spin (mean over the entries), or the one dense matrix with full_det
    const double c_s = 1.0 / (double)S.n_detch;
    for (int sp = 0; sp < S.nch; ++sp) {
        const int ns = sp == 0 ? S.n_up : S.n_dn, n = S.det_n[S.mat_ch[sp]];
        const size_t pgs = (size_t)ns * S.ocols[sp] * PV;
        const double w = c_s / ((double)B_total * S.K * n * n);
        HIP_OK(hipMemsetAsync(gb.PB[sp], 0, pgs * ng * sizeof(T), st));
        hipLaunchKernelGGL((ds::k_orbital_bwd_mse<T>), dim3(ns, (unsigned)ng), dim3(256), 0, st, S, vb.PHI[sp], pgs, vb.Q, tgt[sp], sp,
                           (long)Bc, S.bias_orb ? blk(s->i_borb[sp]) : (const T*)nullptr,
                           s->use_last ? (const T*)vb.SORB[sp] : (const T*)nullptr, (T)(2.0 * w), (T)w, gb.PB[sp], gb.QBAR, LPART);
    }
    hipLaunchKernelGGL((ds::k_loss_final<T>), dim3(1), dim3(256), 0, st, LPART, (long)(S.N * ng), first ? 0 : 1, out_loss);
    return 0;
}

// ------------------------------------------------------------------ KFAC factor pass (ds_kfac.h), hooks of sweep_from_seed
// One entry per `repeated_dense` block of the reference (network.py:430-446), in the order single[0..], double[0..], orbital[0..]
struct KfacBlockPlan {
    ds_kfac_block pub;               // what ds_kfac_layout reports
    ds::KfacRows rows;               // reference rows against padded rows
    int dout_pad, omap, nparam;      // rows of the cotangent in memory; orbital column packing (ds_gemm.h: orb_col)
};
struct KfacPlan {
    std::vector<KfacBlockPlan> blocks;
    int64_t total = 0;               // elements of `factors`
    size_t p1 = 0, p2 = 0, p3 = 0, aux = 0;                  // per group of PV walkers: partials of P1 / P2 / G and the operand v
    int nsplit2 = ds::PV / 5;        // pair layers: waves per 32 x 32 block (one per 5-walker tile, as their weight gradient)
};

int kfac_plan(const ds_system* s, KfacPlan* kp) {
    const ds::SysDev<double>& S = s->sd;
    const int L = S.n_layers, nf_in = S.nf * S.A;
    auto add = [&](int kind, int index, ds::KfacRows R, int d_out, int dout_pad, int repeats, int omap, int nparam, int nsplit,
                   std::initializer_list<int> pbs) {
        KfacBlockPlan b{};
        R.d_in = R.kh + R.nmean * R.kh + R.npm * R.k2 + R.bias;
        b.rows = R; b.dout_pad = dout_pad; b.omap = omap; b.nparam = nparam;
        b.pub.kind = kind; b.pub.index = index; b.pub.has_bias = R.bias; b.pub.d_in = R.d_in; b.pub.d_out = d_out; b.pub.repeats = repeats;
        for (int i = 0; i < 3; ++i) b.pub.param_blocks[i] = -1;
        for (int pb : pbs) if (pb >= 0) b.pub.param_blocks[b.pub.n_param_blocks++] = pb;
        b.pub.a_offset = kp->total; kp->total += (int64_t)R.d_in * R.d_in;
        b.pub.g_offset = kp->total; kp->total += (int64_t)d_out * d_out;
        const size_t Kloc = (size_t)R.Kh + (size_t)R.npm * R.K2, K2t = Kloc + (size_t)R.nmean * R.Kh + 1;
        kp->p1 = std::max(kp->p1, (size_t)nsplit * (Kloc + 1) * (Kloc + 1));
        if (R.nmean) { kp->p2 = std::max(kp->p2, K2t * K2t); kp->aux = std::max(kp->aux, (K2t - 1) * ds::PV); }
        kp->p3 = std::max(kp->p3, (size_t)nsplit * dout_pad * dout_pad);
        kp->blocks.push_back(b);
    };
    for (int l = 0; l < L; ++l)
        add(0, l, ds::KfacRows{l == 0 ? nf_in : s->ref_single[l - 1], S.h1[l], S.nch, l == 0 ? S.nf : s->ref_double[l - 1], S.h2[l], S.nch, 1, 0},
            s->ref_single[l], S.h1[l + 1], S.N, 0, 0, 1, {s->i_wloc[l], s->i_wsh[l], s->i_b[l]});
    for (int l = 0; l < S.n_double; ++l)
        add(1, l, ds::KfacRows{l == 0 ? S.nf : s->ref_double[l - 1], S.h2[l], 0, 0, 0, 0, 1, 0}, s->ref_double[l], S.h2[l + 1], S.N * S.N, 0, 0,
            kp->nsplit2, {s->i_w2[l], s->i_b2[l]});
    for (int c = 0; c < S.nch; ++c) {
        const int nm = s->use_last ? S.nch : 0;
        add(2, c, ds::KfacRows{s->ref_single[L - 1], S.h1[L], nm, s->ref_double[L - 1], S.h2[L], nm, S.bias_orb ? 1 : 0, 0}, 2 * S.nparam[c],
            S.ocols[c], c == 0 ? S.n_up : S.n_dn, 1, S.nparam[c], 1,
            {s->i_worb[c], s->use_last ? s->i_wsh_orb[c] : -1, S.bias_orb ? s->i_borb[c] : -1});
    }
    auto r4 = [](size_t v) { return (v + 3) / 4 * 4; };       // (the operands are read as 4-element vectors)
    kp->p1 = r4(kp->p1); kp->p2 = r4(kp->p2); kp->p3 = r4(kp->p3); kp->aux = r4(kp->aux);
    return 0;
}

template <typename T> struct KfacSink {
    const KfacPlan* kp;
    T *P1, *P2, *P3, *AUX;           // ng groups each
    T* factors;
    int64_t B_total;
    bool first;
};

// K rows of one operand of k_syrk in its tile layout (ds_kfac.h): where the rows live and which columns count
template <typename T> struct SyrkTiles {
    const T* base = nullptr;
    size_t group_stride = 0, tile_stride = 0;
    int ld = 0, n_tiles = 0;         // row stride, tiles per group
    int J = 0, JP = 0;               // columns of a tile, columns per walker of the tile
    int qfix = -1, tw = 0;           // valid columns per walker (-1: the walkers inside the batch), walkers per tile step
};

// [tile = electron][row][PV]: one column per walker of the group
template <typename T>
SyrkTiles<T> walker_tiles(const T* base, size_t group_stride, size_t tile_stride, int n_tiles) {
    SyrkTiles<T> t;
    t.base = base; t.group_stride = group_stride; t.tile_stride = tile_stride; t.n_tiles = n_tiles;
    t.ld = t.J = t.JP = ds::PV;
    return t;
}

// [tile = 5-walker block][row][5][NP]: the pair axis of k_two_bwd, N^2 of its NP columns per walker are pairs
template <typename T>
SyrkTiles<T> pair_tiles(const T* base, int rows, int N, int NP) {
    SyrkTiles<T> t;
    t.J = t.ld = 5 * NP; t.JP = NP; t.qfix = N * N; t.tw = 5; t.n_tiles = ds::PV / 5;
    t.base = base; t.tile_stride = (size_t)rows * t.J; t.group_stride = t.tile_stride * t.n_tiles;
    return t;
}

// the operands of a block: X (input rows) and Z (cotangent of the output); Gaux is the G buffer the spin means and the sums
// over the electrons e0 .. e0 + ne - 1 are taken from (one-electron layers, orbital head with use_last_layer), else null
template <typename T> struct KfacOperands {
    SyrkTiles<T> X, Z;
    const T* Gaux = nullptr;
    int e0 = 0, ne = 0;
};

template <typename T>
void kfac_emit(ds_system* s, const KfacSink<T>& ks, const KfacBlockPlan& b, const KfacOperands<T>& o, int nsplit, int64_t Bc,
               hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int PV = ds::PV;
    const int64_t ng = (Bc + PV - 1) / PV;
    const ds::KfacRows& R = b.rows;
    const int Kloc = R.Kh + R.npm * R.K2, K2t = Kloc + R.nmean * R.Kh + 1;
    // part[group][split] = the upper blocks of x x^T over K rows of x (and a virtual row of ones)
    auto syrk = [&](const SyrkTiles<T>& x, int K, bool ones, T* part, int nsp) {
        const int Kt = K + (ones ? 1 : 0), nb = (Kt + 31) / 32, nblk = nb * (nb + 1) / 2 * nsp;
        hipLaunchKernelGGL((ds::k_syrk<T>), dim3((unsigned)((nblk + 3) / 4), (unsigned)ng), dim3(256), 0, st, x.base, x.group_stride,
                           x.tile_stride, x.ld, x.n_tiles, x.J, K, ones ? 1 : 0, x.JP, x.qfix, x.tw, (long)Bc, part, (size_t)Kt * Kt, nsp);
    };
    syrk(o.X, Kloc, true, ks.P1, nsplit);
    if (R.nmean) {
        const int rows = K2t - 1;
        hipLaunchKernelGGL((ds::k_kfac_aux<T>), dim3((unsigned)((rows * PV + 255) / 256), (unsigned)ng), dim3(256), 0, st, S, o.Gaux, Kloc, R.Kh,
                           R.nmean, o.e0, o.ne, (long)Bc, ks.AUX);
        syrk(walker_tiles<T>(ks.AUX, (size_t)rows * PV, 0, 1), rows, true, ks.P2, 1);
    }
    syrk(o.Z, b.dout_pad, false, ks.P3, nsplit);
    const T scale = (T)(1.0 / ((double)ks.B_total * b.pub.repeats));
    const long na = (long)R.d_in * R.d_in, ngo = (long)b.pub.d_out * b.pub.d_out;
    hipLaunchKernelGGL((ds::k_kfac_assemble<T>), dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, R, (const T*)ks.P1, (long)(ng * nsplit),
                       (const T*)ks.P2, (long)ng, (T)b.pub.repeats, scale, ks.first ? 1 : 0, ks.factors + b.pub.a_offset);
    hipLaunchKernelGGL((ds::k_kfac_assemble_g<T>), dim3((unsigned)((ngo + 255) / 256)), dim3(256), 0, st, b.pub.d_out, b.dout_pad, b.omap,
                       b.nparam, (const T*)ks.P3, (long)(ng * nsplit), scale, ks.first ? 1 : 0, ks.factors + b.pub.g_offset);
}

// PHIBAR / QBAR of a chunk -> parameter gradient: grad = (first ? 0 : grad) + this chunk's sums
template <typename T>
int sweep_from_seed(ds_system* s, const GradPlan& gp, const GradBufs<T>& gb, const T* params, const T* WT, const T* x, int64_t Bc,
                    bool first, T* grad, hipStream_t st, const KfacSink<T>* ks = nullptr) {
    // ks: the KFAC factor pass (ds_kfac_factors) -- every tagged layer's A and G from the operands of its weight gradient;
    // grad may then be null (no packed gradient wanted)
    const ds::SysDev<T>& S = dev<T>(s);
    const int PV = ds::PV;
    const int64_t ng = (Bc + PV - 1) / PV;
    const size_t np = (size_t)s->nparams;
    const int L = S.n_layers, Kl = S.h1[L];
    auto blk = [&](int i) { return params + s->blocks[i].offset; };
    auto boff = [&](int i) { return (size_t)s->blocks[i].offset; };
    const ValBufs<T>& vb = gb.vb;
    T* const* PB = gb.PB; T* const* HB = gb.HB; T* const* H2BAR = gb.H2BAR;
    T *MEANL = gb.MEANL, *MEANBAR = gb.MEANBAR, *MEANBAR2 = gb.MEANBAR2, *QBAR = gb.QBAR, *GBAR = gb.GBAR, *ZBAR = gb.ZBAR, *SBAR = gb.SBAR,
      *Z2BAR = gb.Z2BAR, *PART = gb.PART, *W2S = gb.W2S;
    {
        HIP_OK(hipMemsetAsync(PART, 0, np * ng * sizeof(T), st));
        const size_t gws = (size_t)S.N * S.ldk * PV, gts = (size_t)S.ldk * PV;
        auto outer = [&](const T* X, size_t xg, size_t xt, int ldx, const T* Z, size_t zg, size_t zt, int ldz, int nt, int J, int K,
                         int Nc, size_t off, int nsplit = 1) {
            const int nwt = ((K + 31) / 32) * ((Nc + 31) / 32) * nsplit;
            T* dst = nsplit == 1 ? PART + off : W2S;
            hipLaunchKernelGGL((ds::k_outer_gemm<T>), dim3((unsigned)((nwt + 3) / 4), (unsigned)ng), dim3(256), 0, st, X, xg, xt, ldx, Z, zg,
                               zt, ldz, nt, J, K, Nc, dst, nsplit == 1 ? np : (size_t)K * Nc, nsplit);
            if (nsplit > 1)
                hipLaunchKernelGGL((ds::k_reduce_splits<T>), dim3((unsigned)((K * Nc + 255) / 256), (unsigned)ng), dim3(256), 0, st, W2S,
                                   nsplit, K * Nc, PART + off, np);
        };
        for (int sp = 0; sp < S.nch; ++sp) {
            const int ns = sp == 0 ? S.n_up : S.n_dn, i0 = sp == 0 ? 0 : S.n_up, OC = S.ocols[sp];
            const size_t pgs = (size_t)ns * OC * PV;
            outer(vb.Gl[L] + (size_t)i0 * S.ldk * PV, gws, gts, PV, PB[sp], pgs, (size_t)OC * PV, PV, ns, PV, gp.korb, OC, boff(s->i_worb[sp]));
            if (ks) {
                KfacOperands<T> o;
                o.X = walker_tiles<T>(vb.Gl[L] + (size_t)i0 * S.ldk * PV, gws, gts, ns);
                o.Z = walker_tiles<T>(PB[sp], pgs, (size_t)OC * PV, ns);
                o.Gaux = vb.Gl[L]; o.e0 = i0; o.ne = ns;
                kfac_emit<T>(s, *ks, ks->kp->blocks[L + S.n_double + sp], o, 1, Bc, st);
            }
            if (S.bias_orb)
                hipLaunchKernelGGL((ds::k_orb_bias_grad<T>), dim3(2 * S.nparam[sp], (unsigned)ng), dim3(256), 0, st, PB[sp], pgs, ns, OC,
                                   S.nparam[sp], PART + boff(s->i_borb[sp]), np);
            const int Kop = gp.korb_pad;
            dim3 block; unsigned gz;
            gemm_geom(Kop, 4, &block, &gz);
            hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 0>), dim3(ns, (unsigned)ng, gz), block, 0, st, PB[sp], pgs, (size_t)OC * PV,
                               WT + gp.worbT[sp], OC, (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, ns, GBAR + (size_t)i0 * Kop * PV,
                               (size_t)S.N * Kop * PV, (size_t)0, Kop, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            if (s->use_last) {
                // shared term of the orbital head (network.py:535): S_orb = W_sh^T mean_i h_i, one per spin channel
                const int Ksh = S.nch * Kl;
                if (sp == 0)
                    hipLaunchKernelGGL((ds::k_spin_mean<T>), dim3((unsigned)((Ksh * PV + 255) / 256), (unsigned)ng), dim3(256), 0, st, S, vb.Gl[L],
                                       Kl, MEANL);
                hipLaunchKernelGGL((ds::k_sum_tiles<T>), dim3((unsigned)((OC * PV + 255) / 256), (unsigned)ng), dim3(256), 0, st, PB[sp], pgs, ns,
                                   OC * PV, SBAR);
                outer(MEANL, (size_t)Ksh * PV, 0, PV, SBAR, (size_t)OC * PV, 0, PV, 1, PV, Ksh, OC, boff(s->i_wsh_orb[sp]));
                gemm_geom(Ksh, 4, &block, &gz);
                hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 0>), dim3(1, (unsigned)ng, gz), block, 0, st, (const T*)nullptr, (size_t)0, (size_t)0,
                                   (const T*)nullptr, 0, SBAR, (size_t)OC * PV, WT + gp.wshorbT[sp], OC, 0, sp == 0 ? MEANBAR : MEANBAR2,
                                   (size_t)Ksh * PV, (size_t)0, Ksh, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            }
        }
        hipLaunchKernelGGL((ds::k_env_grad<T>), dim3((unsigned)ng, S.nch), dim3(256), 0, st, S, x, (long)Bc, vb.Gl[0], QBAR,
                           blk(s->i_pi[0]), blk(s->i_sg[0]), blk(s->i_pi[S.nch - 1]), blk(s->i_sg[S.nch - 1]), PART, np,
                           (long)boff(s->i_pi[0]), (long)boff(s->i_sg[0]), (long)boff(s->i_pi[S.nch - 1]), (long)boff(s->i_sg[S.nch - 1]));
        // ---- layers, last to first
        const T* D1 = GBAR; int ld1 = gp.korb_pad; const T* MB = s->use_last ? MEANBAR : nullptr; const T* CARRY = nullptr;
        const T* MB2 = s->use_last && S.nch > 1 ? MEANBAR2 : nullptr;
        int hbi = 0, h2i = 0;
        if (s->use_last)       // the last level of the pair stream feeds the orbital head only
            hipLaunchKernelGGL((ds::k_pair_scatter<T>), dim3((S.NP + 255) / 256, S.h2[L] * 5, (unsigned)(ng * (PV / 5))), dim3(256), 0, st, S, GBAR,
                               gp.korb_pad, Kl, S.h2[L], H2BAR[h2i]);
        for (int l = L - 1; l >= 0; --l) {
            const int Kh = S.h1[l], K2 = S.h2[l], Nout = S.h1[l + 1], Kloc = Kh + S.nch * K2, Ksh = S.nch * Kh;
            const bool res = s->res1[l];
            T* HBc = HB[hbi];
            if (res)
                hipLaunchKernelGGL((ds::k_layer_bwd_prep<T, true>), dim3(Nout / 4, (unsigned)ng), dim3(4 * PV), 0, st, S, D1, ld1, MB, MB2, CARRY,
                                   vb.Gl[l + 1], vb.Gl[l], Nout, HBc, ZBAR, SBAR, PART + boff(s->i_b[l]), np);
            else
                hipLaunchKernelGGL((ds::k_layer_bwd_prep<T, false>), dim3(Nout / 4, (unsigned)ng), dim3(4 * PV), 0, st, S, D1, ld1, MB, MB2, CARRY,
                                   vb.Gl[l + 1], vb.Gl[l], Nout, HBc, ZBAR, SBAR, PART + boff(s->i_b[l]), np);
            outer(vb.Gl[l], gws, gts, PV, ZBAR, (size_t)S.N * Nout * PV, (size_t)Nout * PV, PV, S.N, PV, Kloc, Nout, boff(s->i_wloc[l]));
            if (ks) {
                KfacOperands<T> o;
                o.X = walker_tiles<T>(vb.Gl[l], gws, gts, S.N);
                o.Z = walker_tiles<T>(ZBAR, (size_t)S.N * Nout * PV, (size_t)Nout * PV, S.N);
                o.Gaux = vb.Gl[l]; o.e0 = 0; o.ne = S.N;
                kfac_emit<T>(s, *ks, ks->kp->blocks[l], o, 1, Bc, st);
            }
            const T* MEANl = vb.MEAN0;
            if (l > 0) {
                hipLaunchKernelGGL((ds::k_spin_mean<T>), dim3((unsigned)((S.nch * Kh * PV + 255) / 256), (unsigned)ng), dim3(256), 0, st, S,
                                   vb.Gl[l], Kh, MEANL);
                MEANl = MEANL;
            }
            outer(MEANl, (size_t)Ksh * PV, 0, PV, SBAR, (size_t)Nout * PV, 0, PV, 1, PV, Ksh, Nout, boff(s->i_wsh[l]));
            const int Kpad = gp.kpad[l];
            if (l > 0) {
                dim3 block; unsigned gz;
                gemm_geom(Kpad, 4, &block, &gz);
                hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 0>), dim3(S.N, (unsigned)ng, gz), block, 0, st, ZBAR, (size_t)S.N * Nout * PV,
                                   (size_t)Nout * PV, WT + gp.wlocT[l], Nout, (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, S.N, GBAR,
                                   (size_t)S.N * Kpad * PV, (size_t)0, Kpad, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
                gemm_geom(Ksh, 4, &block, &gz);
                hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 0>), dim3(1, (unsigned)ng, gz), block, 0, st, (const T*)nullptr, (size_t)0,
                                   (size_t)0, (const T*)nullptr, 0, SBAR, (size_t)Nout * PV, WT + gp.wshT[l], Nout, 0, MEANBAR,
                                   (size_t)Ksh * PV, (size_t)0, Ksh, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            }
            // pair stream
            const dim3 pgrid((S.NP / 16 + 3) / 4, (unsigned)(ng * (PV / 5)));
            if (l == S.n_double) {
                if (l > 0)
                    hipLaunchKernelGGL((ds::k_pair_scatter<T>), dim3((S.NP + 255) / 256, K2 * 5, (unsigned)(ng * (PV / 5))), dim3(256), 0, st, S,
                                       GBAR, Kpad, Kh, K2, H2BAR[h2i]);
            } else {
                const int K2o = S.h2[l + 1];
                const bool res2 = s->res2[l], dx = l > 0;
                const T* W2 = blk(s->i_w2[l]);
                T* HBn = H2BAR[h2i]; T* HBi = H2BAR[h2i ^ 1];
#define DS_TWOB(NTI, NTO, RES, DX) hipLaunchKernelGGL((ds::k_two_bwd<T, NTI, NTO, RES, DX>), pgrid, dim3(256), 0, st, S, HBn, vb.H2l[l + 1], \
                                                      vb.H2l[l], W2, GBAR, Kpad, Kh, Z2BAR, HBi, K2)
                if (!dx) {
                    // (the first pair layer: no cotangent of its input; with the reference's residual there tanh(z) = sqrt 2 out - in)
                    if (K2o == 32) { if (res2) DS_TWOB(1, 2, true, false); else DS_TWOB(1, 2, false, false); }
                    else { if (res2) DS_TWOB(1, 1, true, false); else DS_TWOB(1, 1, false, false); }
                }
                else if (K2 == 32 && K2o == 32) { if (res2) DS_TWOB(2, 2, true, true); else DS_TWOB(2, 2, false, true); }
                else if (K2 == 16 && K2o == 16) { if (res2) DS_TWOB(1, 1, true, true); else DS_TWOB(1, 1, false, true); }
                else if (K2 == 32 && K2o == 16) DS_TWOB(2, 1, false, true);
                else if (K2 == 16 && K2o == 32) DS_TWOB(1, 2, false, true);
                else return fail("parameter gradient: unsupported pair-stream widths %d -> %d", K2, K2o);
#undef DS_TWOB
                const int J = 5 * S.NP;
                outer(vb.H2l[l], (size_t)(PV / 5) * K2 * J, (size_t)K2 * J, J, Z2BAR, (size_t)(PV / 5) * K2o * J, (size_t)K2o * J, J, PV / 5,
                      J, K2, K2o, boff(s->i_w2[l]), PV / 5);
                if (ks) {
                    KfacOperands<T> o;
                    o.X = pair_tiles<T>(vb.H2l[l], K2, S.N, S.NP);
                    o.Z = pair_tiles<T>(Z2BAR, K2o, S.N, S.NP);
                    kfac_emit<T>(s, *ks, ks->kp->blocks[L + l], o, ks->kp->nsplit2, Bc, st);
                }
                hipLaunchKernelGGL((ds::k_row_sums<T>), dim3(K2o, (unsigned)ng), dim3(256), 0, st, Z2BAR, (size_t)(PV / 5) * K2o * J,
                                   (size_t)K2o * J, J, PV / 5, J, PART + boff(s->i_b2[l]), np);
                h2i ^= 1;
            }
            D1 = GBAR; ld1 = Kpad; MB = MEANBAR; MB2 = nullptr; CARRY = res ? HBc : nullptr;
            hbi ^= 1;
        }
        if (grad)
            hipLaunchKernelGGL((ds::k_reduce_partials<T>), dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, PART, np, (long)ng, (long)np,
                               first ? 0 : 1, grad);
    }
    return 0;
}

// Workspace of a gradient pass over ng groups: [transposed weights | ng groups of carve_grad | KFAC factor pass: ng groups of
// partials, operand and seed cotangent].  `kp`: the KFAC factor pass; `dets` false: the pretraining pass, which forms no orbital
// matrices -- its loss partials (N per group) live in the idle MINV buffer.
template <typename T> struct GradWs {
    T* WT;
    GradBufs<T> gb;
    T *P1, *P2, *P3, *AUX, *cot;     // KFAC factor pass
    T* LPART;                        // pretraining pass
};

template <typename T>
GradWs<T> carve_grad_pass(const ds_system* s, const GradPlan& gp, const KfacPlan* kp, bool dets, Arena<T>& a, int64_t ng) {
    GradWs<T> w{};
    w.WT = a.take(gp.wt_total);
    w.gb = carve_grad<T>(s, gp, a, ng);
    if (kp) {
        a.align(4);                  // k_syrk reads its operands as 4-element vectors
        w.P1 = a.take(kp->p1 * ng);
        w.P2 = a.take(kp->p2 * ng);
        w.P3 = a.take(kp->p3 * ng);
        w.AUX = a.take(kp->aux * ng);
        w.cot = a.take((size_t)2 * ds::PV * ng);
    }
    if (!dets) {
        a.part(w.gb.vb.MINV, s->wsv.MOUT * ng, [&](Arena<T>& idle) { w.LPART = idle.take((size_t)s->sd.N * ng); });
        w.gb.vb.MOUT = w.gb.vb.MINV = nullptr;
    }
    return w;
}

inline PassSize grad_pass_size(const ds_system* s, const GradPlan& gp, const KfacPlan* kp) {
    auto extent = [&](int64_t ng) { return measure([&](Arena<double>& a) { carve_grad_pass<double>(s, gp, kp, true, a, ng); }); };
    return PassSize{extent(0), extent(1) - extent(0)};
}

// ds_vjp_workspace_bytes / ds_kfac_workspace_bytes: the budget of a gradient pass is 32 GiB
int64_t grad_pass_bytes(const ds_system* s, int64_t B, bool kfac) {
    GradPlan gp;
    KfacPlan kp;
    if (grad_plan(s, &gp) || (kfac && kfac_plan(s, &kp))) return -1;
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    const int64_t groups = groups_per_pass(B, esz, grad_pass_size(s, gp, kfac ? &kp : nullptr), (int64_t)32 << 30);
    return (int64_t)measure([&](Arena<double>& a) { carve_grad_pass<double>(s, gp, kfac ? &kp : nullptr, true, a, groups); }) * esz + 256;
}

// The driver of the three passes: per chunk of groups the value chain, `seed(gp, w, b0, Bc, first)` (fills PHIBAR / QBAR of the chunk
// that starts at walker b0), the reverse sweep.  `factors` with `kp`: the KFAC factor pass (ds_kfac_factors).
template <typename T, typename Seed>
int grad_pass(ds_system* s, const char* what, const T* params, const T* x_, int64_t B, T* grad, T* out_logabs, T* out_phase,
              const KfacPlan* kp, T* factors, bool dets, void* ws, int64_t ws_bytes, hipStream_t st, Seed&& seed) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int PV = ds::PV;
    GradPlan gp;
    if (int rc = grad_plan(s, &gp)) return rc;
    const int64_t cg = groups_that_fit(ws_bytes, sizeof(T), grad_pass_size(s, gp, kp));
    if (cg < 1) return fail("workspace too small for %s: %lld bytes", what, (long long)ws_bytes);
    bool first = true;
    for (int64_t b0 = 0; b0 < B; b0 += cg * PV) {
        const int64_t Bc = std::min<int64_t>(cg * PV, B - b0);
        const T* x = x_ + b0 * 3 * S.N;
        Arena<T> a = arena_of<T>(ws, ws_bytes);
        const GradWs<T> w = carve_grad_pass<T>(s, gp, kp, dets, a, (Bc + PV - 1) / PV);
        if (!a.ok) return carve_fail(what);
        if (first) grad_transposes<T>(s, gp, params, w.WT, st);
        if (int rc = run_value_chain<T>(s, params, x, Bc, w.gb.vb, st, out_logabs ? out_logabs + b0 : nullptr,
                                        out_phase ? out_phase + 2 * b0 : nullptr)) return rc;
        if (int rc = seed(gp, w, b0, Bc, first)) return rc;
        const KfacSink<T> ks{kp, w.P1, w.P2, w.P3, w.AUX, factors, B, first};
        if (int rc = sweep_from_seed<T>(s, gp, w.gb, params, w.WT, x, Bc, first, grad, st, kp ? &ks : nullptr)) return rc;
        first = false;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int logpsi_vjp_impl(ds_system* s, const void* params, const void* x, int64_t B, const void* cot, void* grad, void* out_logabs,
                    void* out_phase, void* ws, int64_t ws_bytes, hipStream_t st) {
    return grad_pass<T>(s, "the parameter gradient", (const T*)params, (const T*)x, B, (T*)grad, (T*)out_logabs, (T*)out_phase, nullptr, nullptr,
                        true, ws, ws_bytes, st, [&](const GradPlan& gp, const GradWs<T>& w, int64_t b0, int64_t Bc, bool) {
                            return seed_logdet<T>(s, gp, w.gb, (const T*)params, (const T*)cot + 2 * b0, Bc, st);
                        });
}

// KFAC factor pass: the value chain, the seed (sqrt2, 0) on every walker, one reverse sweep.
template <typename T>
int kfac_factors_impl(ds_system* s, const void* params, const void* x, int64_t B, void* factors, void* grad, void* ws, int64_t ws_bytes,
                      hipStream_t st) {
    KfacPlan kp;
    if (int rc = kfac_plan(s, &kp)) return rc;
    return grad_pass<T>(s, "the KFAC factor pass", (const T*)params, (const T*)x, B, (T*)grad, nullptr, nullptr, &kp, (T*)factors, true, ws,
                        ws_bytes, st, [&](const GradPlan& gp, const GradWs<T>& w, int64_t, int64_t Bc, bool) {
                            hipLaunchKernelGGL((ds::k_kfac_seed<T>), dim3((unsigned)((Bc + 255) / 256)), dim3(256), 0, st, w.cot, (long)Bc);
                            return seed_logdet<T>(s, gp, w.gb, (const T*)params, w.cot, Bc, st);
                        });
}

// Loss and gradient of the orbital-matching pretraining (reference pretrain.py:70-94): the forward stops behind the orbital
// head (no orbital matrices, LU, inverses or determinant weights), the seed is the residual against the target
template <typename T>
int pretrain_loss_vjp_impl(ds_system* s, const void* params, const void* x, int64_t B, const void* target_up, const void* target_dn,
                           void* out_loss, void* grad, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    if (B <= 0) {                                       // the empty batch: zero loss, zero gradient
        HIP_OK(hipMemsetAsync(out_loss, 0, sizeof(double), st));
        HIP_OK(hipMemsetAsync(grad, 0, (size_t)s->nparams * sizeof(T), st));
        return 0;
    }
    if (!target_up || (S.n_dn > 0 && !target_dn)) return fail("ds_pretrain_loss_vjp: a target is needed for every spin with electrons");
    return grad_pass<T>(s, "the parameter gradient", (const T*)params, (const T*)x, B, (T*)grad, nullptr, nullptr, nullptr, nullptr, false, ws,
                        ws_bytes, st, [&](const GradPlan& gp, const GradWs<T>& w, int64_t b0, int64_t Bc, bool first) {
                            const T* tgt[2] = {(const T*)target_up + (size_t)b0 * S.n_up * S.n_up * 2,
                                               target_dn ? (const T*)target_dn + (size_t)b0 * S.n_dn * S.n_dn * 2 : nullptr};
                            return seed_mse<T>(s, gp, w.gb, (const T*)params, tgt, Bc, B, w.LPART, first, (double*)out_loss, st);
                        });
}


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
        if (int rc = logpsi_impl<T>(s, params, x, B, m->LA2, nullptr, m->wsv, m->wsv_bytes, st)) return rc;
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
        if (int rc = logpsi_impl<T>(s, params, m.X2, B, m.LA2, nullptr, m.wsv, m.wsv_bytes, st)) return rc;
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
// groups per chunk: at most 65535 configurations (the grid limit of the chains)
constexpr int64_t OB_MAX_GROUPS = 65535 / ds::PV;

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
    if (int rc = logpsi_impl<T>(s, params, x, B, w.LA0, w.PH0, w.wsv, w.wsv_bytes, st)) return rc;
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
        if (int rc = logpsi_impl<T>(s, params, w.XD, A.n, w.LA, w.PH, w.wsv, w.wsv_bytes, st)) return rc;
        hipLaunchKernelGGL((ds::k_onebody_accumulate<T>), dim3((unsigned)groups), dim3(64 * ds::OB_WAVES), 0, st, A, shifts, (const T*)w.LA0,
                           (const T*)w.PH0, (const T*)w.LA, (const T*)w.PH, kvec, n_k, (T*)out_ratio, w.PART);
        if (n_k > 0 || n_bad)
            hipLaunchKernelGGL(ds::k_onebody_final, dim3((unsigned)((4 * n_k + 2 + 255) / 256)), dim3(256), 0, st, (const double*)w.PART,
                               (long long)groups, n_k, g0 == 0 ? 1 : 0, g0 + chunk >= total ? 1 : 0, w.ACC, nk_sums, (long long*)n_bad);
    }
    HIP_OK(hipGetLastError());
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
        if (int rc = logpsi_grad_impl<T>(s, params, x, B, m.LA2, nullptr, m.GC, m.wsv, m.wsv_bytes, st)) return rc;          // :111
        hipLaunchKernelGGL((ds::k_real_part<T>), ge, blk, 0, st, m.GC, n3, m.G1);
        const T* nz = normals_ ? (const T*)normals_ + (size_t)i * n3 : m.NZ;
        const T* un = uniforms_ ? (const T*)uniforms_ + (size_t)i * B : m.UN;
        if (!normals_) hipLaunchKernelGGL((ds::k_philox_noise<T>), gn, blk, 0, st, key, (unsigned long long)i, ne, (long)B, m.NZ, m.UN);
        hipLaunchKernelGGL((ds::k_max_norm3<T>), dim3(1), dim3(1024), 0, st, m.G1, ne, m.SCR);
        hipLaunchKernelGGL((ds::k_mh_propose_ex<T>), dim3((unsigned)((ne + 255) / 256)), blk, 0, st, S.sim_a, S.sim_ainv, 2, x, nz, (T)width,
                           m.G1, 0, ne, m.X2, m.SCR);                                                                      // :112-115
        if (int rc = logpsi_grad_impl<T>(s, params, m.X2, B, m.LA2, nullptr, m.GC, m.wsv, m.wsv_bytes, st)) return rc;         // :118
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
        if (int rc = logpsi_impl<T>(s, params, m.X2, B, m.LA2, nullptr, m.wsv, m.wsv_bytes, st)) return rc;                  // :205
        hipLaunchKernelGGL((ds::k_mh_accept_ex<T>), dim3((unsigned)B), dim3(64), 0, st, 1, x, lp, m.X2, m.LA2, un, (const T*)nullptr, (T)width,
                           (const T*)atoms, (const T*)nullptr, n_atoms, S.N, (T*)n_accept, (const T*)nullptr);       // :208-222
    }
    HIP_OK(hipGetLastError());
    return 0;
}


// Reference widths -> the widths the kernels run and the residual pattern.  The one-electron kernels run multiples of 64 features,
// the pair kernels 16 or 32; any other width runs with ZERO-PADDED weights and biases, which is exact: a padded feature is
// tanh(0) = 0 in every layer, has zero jets, adds nothing to the spin means and meets zero rows in the next layer.  A residual
// is added exactly where the reference adds one (network.py:525-528: input width == output width, of the reference's widths),
// whatever the padded widths are.  n_in_single / n_in_double: widths of the input features (nf x atoms, nf; nf = 4 'nu', 7 'tri').
int plan_widths(const int32_t* hs, const int32_t* hd, int n_layers, int n_in_single, int n_in_double, int n_double, int32_t* ps,
                int32_t* pd, int32_t* rs, int32_t* rd) {
    if (n_layers < 1 || n_layers > DS_MAX_LAYERS) return fail("bad n_layers");
    for (int l = 0; l < n_layers; ++l) {
        const int a = hs[l], b = hd[l];
        if (a < 1 || a > 1024) return fail("hidden_single: one-electron widths are supported in 1..1024 (layer %d: %d)", l, a);
        if (l < n_double && (b < 1 || b > 32)) return fail("hidden_double: pair-stream widths are supported in 1..32 (layer %d: %d)", l, b);
        ps[l] = rup(a, 64);
        pd[l] = (b >= 1 && b <= 16) ? 16 : 32;            // (beyond n_double the width is unused: network.py:118-121)
        rs[l] = a == (l == 0 ? n_in_single : hs[l - 1]);
        rd[l] = l < n_double && b == (l == 0 ? n_in_double : hd[l - 1]);
    }
    return 0;
}

// d: the descriptor with the DEVICE widths (plan_widths)
int check_arch(const ds_system_desc* d) {
    if (d->dtype != 0 && d->dtype != 1) return fail("dtype must be 0 (f64) or 1 (f32)");
    if (d->distance_type != 0 && d->distance_type != 1) return fail("Unrecognized distance function.");
    if (d->distance_type == 1 && d->envelope_type != 0) return fail("the 'tri' features support the isotropic envelope only");
    if (d->envelope_type < 0 || d->envelope_type > 2) return fail("unknown envelope_type");
    if (d->n_up < 0 || d->n_dn < 0) return fail("n_up and n_dn must be >= 0");
    if (d->n_up < 1) return fail("internal: n_up must be >= 1 here (ds_system_create swaps a spin-down-only cell)");
    if (d->n_layers < 1 || d->n_layers > DS_MAX_LAYERS) return fail("bad n_layers");
    if (d->n_det < 1 || d->n_det > DS_MAX_DETS) return fail("n_det must be in 1..%d", DS_MAX_DETS);
    if (d->n_sym < 3 || d->n_sym > DS_MAX_SYM) return fail("bad n_sym");
    // every shape limit of the kernels is checked HERE, so that a handle that was created never fails at its first launch
    const int N = d->n_up + d->n_dn, tiles = (3 * N + 2 + 15) / 16, nmat = d->full_det ? N : std::max(d->n_up, d->n_dn);
    if (nmat > 64) return fail("determinant matrices larger than 64 x 64 are not supported (n = %d): the trace kernels keep a matrix row per lane group", nmat);
    if (tiles < 1 || tiles > ds::DS_MAX_TILES)
        return fail("no kernel instance for %d jet-slot tiles (N = %d electrons): supported are N <= 128 (64 with full_det)", tiles, N);
    const int n_double = d->use_last_layer ? d->n_layers : d->n_layers - 1;
    const int nch = d->n_dn > 0 ? 2 : 1;
    for (int l = 0; l < d->n_layers; ++l) {
        if (d->hidden_single[l] % 64 || d->hidden_single[l] < 64 || d->hidden_single[l] > 1024)
            return fail("internal: device width %d of layer %d is not a multiple of 64 in 64..1024", d->hidden_single[l], l);
        if (l < n_double && d->hidden_double[l] != 16 && d->hidden_double[l] != 32)
            return fail("internal: device pair width %d of layer %d is not 16 or 32", d->hidden_double[l], l);
    }
    const int k_orb = d->hidden_single[d->n_layers - 1] + (d->use_last_layer ? nch * d->hidden_double[d->n_layers - 1] : 0);
    if (k_orb % 16) return fail("orbital head with K = %d input rows: the GEMM's operand ring needs K %% 16 == 0", k_orb);
    return 0;
}

}  // namespace

// observables (ds_obs.h): one kernel instance per number of q points per lane
namespace {
template <typename T, int QJ>
void launch_obs_partial(const ds::ObsArgs& A, const void* x, int64_t B, int N, int G, double* part, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_obs_partial<T, QJ>), dim3(G), dim3(64), 0, st, A, (const T*)x, (long long)B, N, part);
}

template <typename T>
void obs_partial(const ds::ObsArgs& A, const void* x, int64_t B, int N, int G, double* part, hipStream_t st) {
    switch ((A.n_q + 63) / 64) {    // points per lane
        case 0: case 1: launch_obs_partial<T, 1>(A, x, B, N, G, part, st); break;
        case 2: launch_obs_partial<T, 2>(A, x, B, N, G, part, st); break;
        case 3: case 4: launch_obs_partial<T, 4>(A, x, B, N, G, part, st); break;
        default: launch_obs_partial<T, 8>(A, x, B, N, G, part, st); break;
    }
}
}  // namespace

// ------------------------------------------------------------------ KFAC step (ds_kfac.h): damped inverses, preconditioner
namespace {
struct KfacStepPlan {
    ds::KfacMats M;
    int64_t total = 0, rows = 0, vtotal = 0;      // elements of factors / inverses; rows of all matrices; elements of v / out
    int nmax = 0, tiles_max = 0;                  // largest order; most 32 x 32 output tiles of one block
    // workspace, in doubles: work copy | damped matrix, then refined inverse | residual | traces | pivot inverses |
    // saved column panels | T = A^- V | tile partials
    int64_t o_w = 0, o_m = 0, o_r = 0, o_tr = 0, o_p = 0, o_c = 0, o_t = 0, o_part = 0, doubles = 0;
};

int kfac_step_plan_sized(int nb, const int32_t* d_in, const int32_t* d_out, const int32_t* rep, KfacStepPlan* sp) {
    if (nb < 1 || nb > DS_KFAC_MAX_BLOCKS) return fail("KFAC step: between 1 and 18 blocks");
    ds::KfacMats& M = sp->M;
    std::memset(&M, 0, sizeof(M));
    M.nb = nb;
    for (int b = 0; b < nb; ++b) {
        if (d_in[b] < 1 || d_out[b] < 1 || rep[b] < 1) return fail("KFAC step: block sizes and repeats must be positive");
        const int n2[2] = {d_in[b], d_out[b]};
        for (int h = 0; h < 2; ++h) {
            const int m = 2 * b + h;
            M.n[m] = n2[h]; M.off[m] = (long)sp->total; M.rs[m] = (long)sp->rows;
            sp->total += (int64_t)n2[h] * n2[h]; sp->rows += n2[h];
            sp->nmax = std::max(sp->nmax, n2[h]);
        }
        M.rep[b] = rep[b];
        M.voff[b] = (long)sp->vtotal; sp->vtotal += (int64_t)d_in[b] * d_out[b];
        const int tiles = ((d_in[b] + 31) / 32) * ((d_out[b] + 31) / 32);
        M.toff[b + 1] = M.toff[b] + tiles;
        sp->tiles_max = std::max(sp->tiles_max, tiles);
    }
    auto r8 = [](int64_t v) { return (v + 7) / 8 * 8; };
    sp->o_w = 0;
    sp->o_m = sp->o_w + r8(sp->total);
    sp->o_r = sp->o_m + r8(sp->total);
    sp->o_tr = sp->o_r + r8(sp->total);
    sp->o_p = sp->o_tr + r8(2 * nb);
    sp->o_c = sp->o_p + (int64_t)2 * nb * 1024;
    sp->o_t = sp->o_c + sp->rows * 32;
    sp->o_part = sp->o_t + r8(sp->vtotal);
    sp->doubles = sp->o_part + r8(M.toff[nb]);
    return 0;
}

int kfac_step_plan(const ds_system* s, KfacStepPlan* sp, bool refuse_scalar) {
    if (s->sd.env_type == 2)
        return fail("KFAC step: envelope_type 'full' is not supported (its sigma is the tagged block qmc1, network.py:358-362)");
    KfacPlan kp;
    if (int rc = kfac_plan(s, &kp)) return rc;
    const int nb = (int)kp.blocks.size();
    if (nb > DS_KFAC_MAX_BLOCKS) return fail("KFAC step: more than 18 blocks");
    int32_t di[DS_KFAC_MAX_BLOCKS], dout[DS_KFAC_MAX_BLOCKS], rep[DS_KFAC_MAX_BLOCKS];
    for (int b = 0; b < nb; ++b) {
        di[b] = kp.blocks[b].pub.d_in; dout[b] = kp.blocks[b].pub.d_out; rep[b] = kp.blocks[b].pub.repeats;
        if (refuse_scalar && (di[b] == 1 || dout[b] == 1))
            return fail("KFAC step: a block with d_in == 1 or d_out == 1 is not supported (pi_adjusted_inverse treats it specially, "
                        "utils.py:179-191)");
    }
    return kfac_step_plan_sized(nb, di, dout, rep, sp);
}

template <typename T>
int kfac_inverses_run(const KfacStepPlan& sp, const void* factors, double w, double damping, void* inverses, void* ws, int64_t ws_bytes,
                      hipStream_t st) {
    if (ws_bytes < sp.doubles * 8) return fail("ds_kfac_inverses: workspace too small (ds_kfac_step_workspace_bytes)");
    if (!(w > 0.0)) return fail("ds_kfac_inverses: ema_weight must be positive");
    if (!(damping > 0.0)) return fail("ds_kfac_inverses: damping must be positive");
    double* base = (double*)ws;
    double *W = base + sp.o_w, *M0 = base + sp.o_m, *R = base + sp.o_r, *tr = base + sp.o_tr, *P = base + sp.o_p, *C = base + sp.o_c;
    const unsigned nm = 2u * (unsigned)sp.M.nb;
    const unsigned ge = (unsigned)(((int64_t)sp.nmax * sp.nmax + 255) / 256);
    const int nbmax = (sp.nmax + 31) / 32;
    hipLaunchKernelGGL((ds::k_kinv_trace<T>), dim3(nm), dim3(256), 0, st, sp.M, (const T*)factors, w, tr);
    hipLaunchKernelGGL((ds::k_kinv_prep<T>), dim3(ge, nm), dim3(256), 0, st, sp.M, (const T*)factors, w, damping, (const double*)tr, W, M0);
    for (int k = 0; k < nbmax; ++k) {
        hipLaunchKernelGGL(ds::k_kinv_diag, dim3(nm), dim3(256), 0, st, sp.M, (const double*)W, P, k);
        if (nbmax > 1)
            hipLaunchKernelGGL(ds::k_kinv_panel, dim3((unsigned)((nbmax + 3) / 4), nm), dim3(256), 0, st, sp.M, W, (const double*)P, C, k);
        hipLaunchKernelGGL(ds::k_kinv_update, dim3((unsigned)((nbmax * nbmax + 3) / 4), nm), dim3(256), 0, st, sp.M, W, (const double*)P,
                           (const double*)C, k);
    }
    // one Newton step: R = I - M0 W, then M0 <- W + W R (M0 is free once R exists)
    const dim3 gr((unsigned)((nbmax * nbmax + 3) / 4), nm);
    hipLaunchKernelGGL((ds::k_kinv_refine<1>), gr, dim3(256), 0, st, sp.M, (const double*)M0, (const double*)W, R);
    hipLaunchKernelGGL((ds::k_kinv_refine<2>), gr, dim3(256), 0, st, sp.M, (const double*)W, (const double*)R, M0);
    hipLaunchKernelGGL((ds::k_kinv_finish<T>), dim3(ge, nm), dim3(256), 0, st, sp.M, (const double*)M0, damping, (const double*)tr,
                       (T*)inverses);
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int kfac_precondition_run(const KfacStepPlan& sp, const void* inverses, const void* v, void* out, double* sq, void* ws, int64_t ws_bytes,
                          hipStream_t st) {
    if (ws_bytes < sp.doubles * 8) return fail("ds_kfac_precondition: workspace too small (ds_kfac_step_workspace_bytes)");
    double* base = (double*)ws;
    T* Tm = (T*)(base + sp.o_t);
    double* part = base + sp.o_part;
    const dim3 grid((unsigned)((sp.tiles_max + 3) / 4), (unsigned)sp.M.nb);
    hipLaunchKernelGGL((ds::k_kprec_gemm<T, 1>), grid, dim3(256), 0, st, sp.M, (const T*)inverses, (const T*)v, Tm, (const T*)v, part);
    hipLaunchKernelGGL((ds::k_kprec_gemm<T, 2>), grid, dim3(256), 0, st, sp.M, (const T*)inverses, (const T*)Tm, (T*)out, (const T*)v, part);
    hipLaunchKernelGGL(ds::k_kprec_final, dim3((unsigned)sp.M.nb), dim3(64), 0, st, sp.M, (const double*)part, sq);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // namespace

// the message slot of ds_last_error for the entry points compiled in other objects (ds_hf.hip)
namespace ds {
void set_last_error(const char* msg) { g_err = msg; }
}  // namespace ds

// =============================================================================== C ABI
extern "C" {

const char* ds_last_error(void) { return g_err.c_str(); }

int ds_device_widths(const int32_t* hidden_single, const int32_t* hidden_double, int32_t n_layers, int32_t n_in_single, int32_t n_in_double,
                     int32_t n_double, int32_t* dev_single, int32_t* dev_double, int32_t* res_single, int32_t* res_double) {
    if (!hidden_single || !hidden_double || !dev_single || !dev_double || !res_single || !res_double) return fail("null argument");
    return plan_widths(hidden_single, hidden_double, n_layers, n_in_single, n_in_double, n_double, dev_single, dev_double, res_single, res_double);
}

int ds_system_create(const ds_system_desc* ref_desc, ds_system** out) {
    if (!ref_desc || !out) return fail("null argument");
    // the descriptor carries the REFERENCE's hidden_dims; from here on `desc` has the widths the kernels run
    ds_system_desc dev_desc = *ref_desc;
    int32_t rs[DS_MAX_LAYERS] = {0}, rd[DS_MAX_LAYERS] = {0};
    {
        if (ref_desc->distance_type != 0 && ref_desc->distance_type != 1) return fail("Unrecognized distance function.");
        if (ref_desc->n_layers < 1 || ref_desc->n_layers > DS_MAX_LAYERS) return fail("bad n_layers");
        const int nf = ref_desc->distance_type == 0 ? 4 : 7;
        const int n_double = ref_desc->use_last_layer ? ref_desc->n_layers : ref_desc->n_layers - 1;
        if (int rc = plan_widths(ref_desc->hidden_single, ref_desc->hidden_double, ref_desc->n_layers, nf * ref_desc->n_atoms_prim, nf, n_double,
                                 dev_desc.hidden_single, dev_desc.hidden_double, rs, rd))
            return rc;
    }
    // only spin-down electrons: an extension beyond the reference (its parameter tree drops the empty channel, network.py:113-117, but
    // its forward raises on it, network.py:537-553): the parameter tree is that of the mirrored cell (n_dn, 0) -- run that
    if (dev_desc.n_up == 0 && dev_desc.n_dn > 0) {
        dev_desc.n_up = dev_desc.n_dn;
        dev_desc.n_dn = 0;
        dev_desc.klist_up = dev_desc.klist_dn;
        dev_desc.klist_dn = nullptr;
    }
    if (dev_desc.n_up + dev_desc.n_dn < 1) return fail("n_up + n_dn must be >= 1");
    const ds_system_desc* desc = &dev_desc;
    if (int rc = check_arch(desc)) return rc;
    if (!desc->prim_atoms || !desc->klist_up || (desc->n_dn > 0 && !desc->klist_dn) || !desc->sim_atoms || !desc->sim_charges ||
        (desc->n_g > 0 && (!desc->gpoints || !desc->gweight || !desc->ion_exp_re || !desc->ion_exp_im)))
        return fail("null array pointer in ds_system_desc");
    ds_system* s = new ds_system();
    s->d = *desc;
    for (int l = 0; l < desc->n_layers; ++l) {
        s->ref_single[l] = ref_desc->hidden_single[l];
        s->ref_double[l] = ref_desc->hidden_double[l];
        s->res1[l] = rs[l] != 0;
        s->res2[l] = rd[l] != 0;
    }
    s->dtype = desc->dtype;
    s->use_last = desc->use_last_layer != 0;
    std::vector<double> h64;
    std::vector<float> h32;
    fill_tables<double>(s, desc, s->sd, h64);
    fill_tables<float>(s, desc, s->sf, h32);
    if (hipMalloc(&s->blob64, h64.size() * sizeof(double)) != hipSuccess || hipMalloc(&s->blob32, h32.size() * sizeof(float)) != hipSuccess) {
        delete s;
        return fail("hipMalloc of the system tables failed (is a GPU visible?)");
    }
    if (hipMemcpy(s->blob64, h64.data(), h64.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s->blob32, h32.data(), h32.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        ds_system_destroy(s);
        return fail("upload of the system tables failed");
    }
    relocate<double>(s->sd, (const double*)s->blob64);
    relocate<float>(s->sf, (const float*)s->blob32);
    build_layouts(s);
    {
        int h1max = 0;
        for (int l = 0; l <= s->sd.n_layers; ++l) h1max = std::max(h1max, s->sd.h1[l]);
        if (hipMalloc(&s->lr_w0t, (size_t)h1max * 64 * sizeof(double)) != hipSuccess) {
            ds_system_destroy(s);
            return fail("hipMalloc of the low-rank layer's weight table failed");
        }
    }
    {
        hipDeviceProp_t prop;
        int devid = 0;
        if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.multiProcessorCount > 0)
            s->n_cu = prop.multiProcessorCount;
    }
    if (hipMalloc((void**)&s->clk_dev, 1024 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(s->clk_dev, 0, 1024 * sizeof(unsigned long long)) != hipSuccess) {
        ds_system_destroy(s);
        return fail("hipMalloc of the clock-probe counters failed");
    }
    // environment switches are read here, once; the launch paths never call getenv
    s->det_valu = getenv("DS_DET_VALU") != nullptr;
    if (const char* e = getenv("DS_VAL_NB")) { const int v = atoi(e); s->val_nb = (v == 1 || v == 2 || v == 4) ? v : 0; }
    s->no_lu_wave = getenv("DS_NO_LU_WAVE") != nullptr;
    s->use_lr = getenv("DS_NO_LOWRANK") == nullptr;
    s->use_pm_skip = getenv("DS_NO_PM_SKIP") == nullptr;
    s->use_pair_expand = getenv("DS_NO_PAIR_EXPAND") == nullptr;
    s->use_g4 = getenv("DS_NO_G4") == nullptr;
    s->use_i8 = getenv("DS_I8") != nullptr && getenv("DS_NO_I8") == nullptr;
    s->use_ldsb = getenv("DS_NO_LDSB") == nullptr;
    s->use_pair_fuse = getenv("DS_NO_PAIR_FUSE") == nullptr;
    s->use_i8_val = getenv("DS_NO_I8_VAL") == nullptr;
    for (int l = 0; l < DS_MAX_LAYERS; ++l) s->i8_prepped[l] = ~(uint64_t)0;
    if (const char* e = getenv("DS_I8_VAL_MIN_TILES")) s->val_i8_min_tiles = atoll(e);
    if (const char* e = getenv("DS_DBG")) s->dbg = atoi(e);
    s->use_wide = getenv("DS_NO_WIDE") == nullptr;
    s->wide_all = getenv("DS_WIDE_ALL") != nullptr;
    {
        // digit planes of the int8 layers' weights: only for a handle some layer of which can run as an int8 split (the energy chain has
        // the most such layers in a stage dump: no low-rank layer 1)
        ChainPlan<double> plan;
        bool need = plan_chain<double>(s, true, &plan) == 0 && plan.count(LayerKind::Int8, s->sd.n_layers) > 0;
        for (int l = 1; l < s->sd.n_layers; ++l) need = need || int8_value_layer(s, l);
        if (need && hipMalloc(&s->i8_wp, (size_t)DS_MAX_LAYERS * (ds::i8::wp_bytes(64 * 5) + ds::i8::NOUT * sizeof(double))) != hipSuccess) {
            ds_system_destroy(s);
            return fail("hipMalloc of the int8 layer's weight planes failed");
        }
    }
    // (grid.y carries the walker index: at most 65535 walkers per launch)
    if (const char* e = getenv("DS_CHUNK_WALKERS")) s->chunk_cap = std::min<int64_t>(65535, std::max<int64_t>(1, atol(e)));
    *out = s;
    return 0;
}

void ds_system_destroy(ds_system* s) {
    if (!s) return;
    if (s->clk_dev) (void)hipFree(s->clk_dev);
    if (s->lr_w0t) (void)hipFree(s->lr_w0t);
    if (s->i8_wp) (void)hipFree(s->i8_wp);
    if (s->blob64) (void)hipFree(s->blob64);
    if (s->blob32) (void)hipFree(s->blob32);
    delete s;
}

int64_t ds_param_count(const ds_system* s) { return s ? s->nparams : -1; }

int ds_int8_layers(const ds_system* s) {
    if (!s) return -1;
    ChainPlan<double> plan;
    return plan_chain<double>(s, false, &plan) == 0 ? plan.count(LayerKind::Int8, s->sd.n_layers) : 0;
}

int ds_param_layout(const ds_system* s, ds_param_block* blocks, int max_blocks) {
    if (!s) return -1;
    const int n = (int)s->blocks.size();
    for (int i = 0; i < n && i < max_blocks; ++i) blocks[i] = s->blocks[i];
    return n;
}

int64_t ds_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s) return -1;
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    // walkers are processed in chunks: at most 4096 per chunk, and a scratch budget of at most 80 GiB but never more than 40 % of
    // the device memory that is free when the caller asks (large cells need hundreds of MB per walker: 96 electrons f32 =
    // 0.2 GB; a second DeviceSystem in the process, a smaller GPU or a caching allocator holding old buffers must not turn
    // this into an out-of-memory error).  One 4096-walker pass instead of four 1024-walker passes is 1.5-2 % faster (fewer
    // kernel tails) with bit-identical energies (tools/chunk_sweep.py); DS_CHUNK_WALKERS (read at create) overrides the cap.
    int64_t budget = (int64_t)80 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        budget = std::min<int64_t>(budget, std::max<int64_t>((int64_t)(free_b / 10 * 4), (int64_t)1 << 30));
    const int64_t cap = s->chunk_cap;
    int64_t chunk = std::min<int64_t>(std::max<int64_t>(B, 1), cap);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, budget / ((int64_t)s->ws.per_walker * esz)));
    const int64_t groups = groups_per_pass(B, esz, PassSize{0, s->wsv.per_walker}, budget);
    return std::max((int64_t)s->ws.per_walker * esz * chunk, (int64_t)s->wsv.per_walker * esz * groups) + 256;
}

int ds_local_energy(ds_system* s, const void* params, const void* x, int64_t B, void* out_ke, void* out_ewald, void* out_logabs,
                    void* out_phase, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return s->dtype == 0 ? local_energy_impl<double>(s, params, x, B, out_ke, out_ewald, out_logabs, out_phase, ws, ws_bytes, st)
                         : local_energy_impl<float>(s, params, x, B, out_ke, out_ewald, out_logabs, out_phase, ws, ws_bytes, st);
}

int ds_logpsi(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* ws,
              int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return s->dtype == 0 ? logpsi_impl<double>(s, params, x, B, out_logabs, out_phase, ws, ws_bytes, st)
                         : logpsi_impl<float>(s, params, x, B, out_logabs, out_phase, ws, ws_bytes, st);
}

int ds_logpsi_grad(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* out_grad,
                   void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws || !out_grad) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return s->dtype == 0 ? logpsi_grad_impl<double>(s, params, x, B, out_logabs, out_phase, out_grad, ws, ws_bytes, st)
                         : logpsi_grad_impl<float>(s, params, x, B, out_logabs, out_phase, out_grad, ws, ws_bytes, st);
}

int64_t ds_vjp_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s) return -1;
    return grad_pass_bytes(s, B, false);
}

int ds_logpsi_vjp(ds_system* s, const void* params, const void* x, int64_t B, const void* cot, void* grad, void* out_logabs,
                  void* out_phase, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !cot || !grad || !ws) return fail("null argument");
    hipStream_t st = (hipStream_t)stream;
    if (B <= 0) {
        if (hipMemsetAsync(grad, 0, (size_t)s->nparams * (s->dtype == 0 ? 8 : 4), st) != hipSuccess) return fail("hipMemsetAsync failed");
        return 0;
    }
    return s->dtype == 0 ? logpsi_vjp_impl<double>(s, params, x, B, cot, grad, out_logabs, out_phase, ws, ws_bytes, st)
                         : logpsi_vjp_impl<float>(s, params, x, B, cot, grad, out_logabs, out_phase, ws, ws_bytes, st);
}

int ds_kfac_block_count(const ds_system* s) {
    if (!s) return -1;
    KfacPlan kp;
    return kfac_plan(s, &kp) ? -1 : (int)kp.blocks.size();
}

int ds_kfac_layout(const ds_system* s, ds_kfac_block* blocks, int max_blocks) {
    if (!s) return -1;
    KfacPlan kp;
    if (kfac_plan(s, &kp)) return -1;
    const int n = (int)kp.blocks.size();
    for (int i = 0; i < n && i < max_blocks; ++i) blocks[i] = kp.blocks[i].pub;
    return n;
}

int64_t ds_kfac_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s) return -1;
    return grad_pass_bytes(s, B, true);
}

int ds_kfac_factors(ds_system* s, const void* params, const void* x, int64_t B, void* factors, void* grad_seed, void* ws, int64_t ws_bytes,
                    void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !factors || (B > 0 && (!x || !ws))) return fail("null argument");      // (the empty batch needs no workspace)
    if (s->sd.env_type == 2)
        return fail("ds_kfac_factors: envelope_type 'full' is not supported (its sigma is the tagged block qmc1, network.py:358-362)");
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = s->dtype == 0 ? 8 : 4;
    if (B <= 0) {                                       // the empty batch: zero factors, zero gradient
        KfacPlan kp;
        if (int rc = kfac_plan(s, &kp)) return rc;
        HIP_OK(hipMemsetAsync(factors, 0, (size_t)kp.total * esz, st));
        if (grad_seed) HIP_OK(hipMemsetAsync(grad_seed, 0, (size_t)s->nparams * esz, st));
        return 0;
    }
    return s->dtype == 0 ? kfac_factors_impl<double>(s, params, x, B, factors, grad_seed, ws, ws_bytes, st)
                         : kfac_factors_impl<float>(s, params, x, B, factors, grad_seed, ws, ws_bytes, st);
}

int64_t ds_kfac_step_workspace_bytes(const ds_system* s) {
    if (!s) return -1;
    KfacStepPlan sp;
    if (kfac_step_plan(s, &sp, false)) return -1;
    return sp.doubles * 8;
}

int ds_kfac_inverses(ds_system* s, const void* factors, double ema_weight, double damping, void* inverses, void* ws, int64_t ws_bytes,
                     void* stream) {
    if (!s || !factors || !inverses || !ws) return fail("null argument");
    KfacStepPlan sp;
    if (int rc = kfac_step_plan(s, &sp, true)) return rc;
    return s->dtype == 0 ? kfac_inverses_run<double>(sp, factors, ema_weight, damping, inverses, ws, ws_bytes, (hipStream_t)stream)
                         : kfac_inverses_run<float>(sp, factors, ema_weight, damping, inverses, ws, ws_bytes, (hipStream_t)stream);
}

int ds_kfac_precondition(ds_system* s, const void* inverses, const void* v, void* out, double* sq_norm, void* ws, int64_t ws_bytes,
                         void* stream) {
    if (!s || !inverses || !v || !out || !sq_norm || !ws) return fail("null argument");
    KfacStepPlan sp;
    if (int rc = kfac_step_plan(s, &sp, true)) return rc;
    return s->dtype == 0 ? kfac_precondition_run<double>(sp, inverses, v, out, sq_norm, ws, ws_bytes, (hipStream_t)stream)
                         : kfac_precondition_run<float>(sp, inverses, v, out, sq_norm, ws, ws_bytes, (hipStream_t)stream);
}

int64_t ds_kfac_inverses_sized_workspace_bytes(int n_blocks, const int32_t* d_in, const int32_t* d_out) {
    if (!d_in || !d_out) return -1;
    int32_t rep[DS_KFAC_MAX_BLOCKS];
    for (int b = 0; b < DS_KFAC_MAX_BLOCKS; ++b) rep[b] = 1;
    KfacStepPlan sp;
    if (kfac_step_plan_sized(n_blocks, d_in, d_out, rep, &sp)) return -1;
    return sp.doubles * 8;
}

int ds_kfac_inverses_sized(int dtype, int n_blocks, const int32_t* d_in, const int32_t* d_out, const int32_t* repeats, const void* factors,
                           double ema_weight, double damping, void* inverses, void* ws, int64_t ws_bytes, void* stream) {
    if (!d_in || !d_out || !repeats || !factors || !inverses || !ws) return fail("null argument");
    if (dtype != 0 && dtype != 1) return fail("ds_kfac_inverses_sized: dtype must be 0 (float64) or 1 (float32)");
    KfacStepPlan sp;
    if (int rc = kfac_step_plan_sized(n_blocks, d_in, d_out, repeats, &sp)) return rc;
    return dtype == 0 ? kfac_inverses_run<double>(sp, factors, ema_weight, damping, inverses, ws, ws_bytes, (hipStream_t)stream)
                      : kfac_inverses_run<float>(sp, factors, ema_weight, damping, inverses, ws, ws_bytes, (hipStream_t)stream);
}

int64_t ds_pretrain_workspace_bytes(const ds_system* s, int64_t B) { return ds_vjp_workspace_bytes(s, B); }

int ds_pretrain_loss_vjp(ds_system* s, const void* params, const void* x, int64_t B, const void* target_up, const void* target_dn,
                         void* out_loss, void* grad, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !out_loss || !grad || !ws || (B > 0 && !x)) return fail("null argument");
    hipStream_t st = (hipStream_t)stream;
    return s->dtype == 0 ? pretrain_loss_vjp_impl<double>(s, params, x, B, target_up, target_dn, out_loss, grad, ws, ws_bytes, st)
                         : pretrain_loss_vjp_impl<float>(s, params, x, B, target_up, target_dn, out_loss, grad, ws, ws_bytes, st);
}

int ds_ewald(ds_system* s, const void* x, int64_t B, void* out, void* stream) {
    if (!s || !x || !out) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (s->dtype == 0) {
        size_t sh = ds::ewald_lds_bytes(s->sd);
        hipLaunchKernelGGL((ds::k_ewald<double>), dim3((unsigned)B), dim3(256), sh, st, s->sd, (const double*)x, (double*)out);
    } else {
        size_t sh = ds::ewald_lds_bytes(s->sf);
        hipLaunchKernelGGL((ds::k_ewald<float>), dim3((unsigned)B), dim3(256), sh, st, s->sf, (const float*)x, (float*)out);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_enforce_pbc(const double* latvec, int dtype, const void* x, int64_t n_elec, void* out_x, void* out_wrap, void* stream) {
    if (!latvec || !x || !out_x) return fail("null argument");
    if (n_elec <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    double inv[9];
    inv3(latvec, inv);
    dim3 grid((unsigned)((n_elec + 255) / 256)), block(256);
    if (dtype == 0) {
        ds::Lattice<double> L;
        for (int i = 0; i < 9; ++i) { L.a[i] = latvec[i]; L.ainv[i] = inv[i]; }
        hipLaunchKernelGGL((ds::k_enforce_pbc<double>), grid, block, 0, st, L, (const double*)x, (size_t)n_elec, (double*)out_x,
                           (double*)out_wrap);
    } else if (dtype == 1) {
        ds::Lattice<float> L;
        for (int i = 0; i < 9; ++i) { L.a[i] = (float)latvec[i]; L.ainv[i] = (float)inv[i]; }
        hipLaunchKernelGGL((ds::k_enforce_pbc<float>), grid, block, 0, st, L, (const float*)x, (size_t)n_elec, (float*)out_x,
                           (float*)out_wrap);
    } else {
        return fail("dtype must be 0 or 1");
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t ds_observables_workspace_bytes(int64_t B, int n_q) {
    if (B < 1 || n_q < 0 || n_q > ds::OBS_MAX_Q) return -1;
    return (int64_t)ds::obs_groups(B) * (2 + 3 * n_q) * (int64_t)sizeof(double);
}

int ds_observables(const double* recvec, int dtype, const void* x, int64_t B, int64_t n_elec, const int32_t* q_int, int n_q,
                   int pol_direction, double* out_sums, void* ws, int64_t ws_bytes, void* stream) {
    if (!recvec || !x || !out_sums || !ws) return fail("null argument");
    if (dtype != 0 && dtype != 1) return fail("dtype must be 0 or 1");
    if (B < 1) return fail("B must be >= 1 (got %lld)", (long long)B);
    if (n_elec < 1 || n_elec > ds::OBS_MAX_N) return fail("n_elec must be in 1..%d (got %lld)", ds::OBS_MAX_N, (long long)n_elec);
    if (n_q < 0 || n_q > ds::OBS_MAX_Q) return fail("n_q must be in 0..%d (got %d)", ds::OBS_MAX_Q, n_q);
    if (n_q > 0 && !q_int) return fail("null q_int with n_q = %d", n_q);
    if (pol_direction < -1 || pol_direction > 2) return fail("pol_direction must be -1, 0, 1 or 2 (got %d)", pol_direction);
    const int64_t need = ds_observables_workspace_bytes(B, n_q);
    if (ws_bytes < need) return fail("workspace too small for ds_observables: %lld bytes < %lld", (long long)ws_bytes, (long long)need);
    ds::ObsArgs A;
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(recvec[i])) return fail("recvec[%d] is not finite", i);
        A.g[i] = recvec[i];
    }
    A.n_q = n_q;
    A.pol = pol_direction;
    int pmax = 0;
    for (int k = 0; k < 3 * n_q; ++k) {
        const int32_t n = q_int[k];
        if (n < 0 || n >= ds::OBS_MAX_POW)
            return fail("q point %d: lattice coordinate %d is outside 0..%d", k / 3, (int)n, ds::OBS_MAX_POW - 1);
        A.qn[k] = (signed char)n;
        pmax = std::max(pmax, (int)n);
    }
    for (int k = 3 * n_q; k < 3 * ds::OBS_MAX_Q; ++k) A.qn[k] = 0;
    A.n_pow = pmax + 1;
    hipStream_t st = (hipStream_t)stream;
    const int G = ds::obs_groups(B), K = 2 + 3 * n_q;
    double* part = (double*)ws;
    if (dtype == 0)
        obs_partial<double>(A, x, B, (int)n_elec, G, part, st);
    else
        obs_partial<float>(A, x, B, (int)n_elec, G, part, st);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(ds::k_obs_final, dim3((K + 255) / 256), dim3(256), 0, st, (const double*)part, G, K, out_sums);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_realspace_counts(const double* fold_inv, const int32_t* grid, const double* latvec, const double* latvec_inv, double r_max,
                        int n_r, int dtype, const void* x, int64_t B, int64_t n_elec, int64_t n_up, int64_t* dens, int64_t* pair,
                        void* stream) {
    if (!x) return fail("null argument");
    if (!dens && !pair) return fail("ds_realspace_counts: dens and pair are both null, nothing to count");
    if (dtype != 0 && dtype != 1) return fail("dtype must be 0 or 1");
    if (B < 1) return fail("B must be >= 1 (got %lld)", (long long)B);
    if (n_elec < 1 || n_elec > ds::RS_MAX_N) return fail("n_elec must be in 1..%d (got %lld)", ds::RS_MAX_N, (long long)n_elec);
    if (n_up < 0 || n_up > n_elec) return fail("n_up must be in 0..n_elec = %lld (got %lld)", (long long)n_elec, (long long)n_up);
    ds::RealSpaceArgs A;
    std::memset(&A, 0, sizeof(A));
    A.n_up = (int)n_up;
    A.do_dens = dens != nullptr;
    A.do_pair = pair != nullptr;
    if (dens) {
        if (!fold_inv || !grid) return fail("ds_realspace_counts: the density needs fold_inv and grid");
        long long cells = 1;
        for (int j = 0; j < 3; ++j) {
            if (grid[j] < 1 || grid[j] > ds::RS_MAX_G) return fail("grid[%d] must be in 1..%d (got %d)", j, ds::RS_MAX_G, (int)grid[j]);
            A.g[j] = grid[j];
            cells *= grid[j];
        }
        if (cells > ds::RS_MAX_BINS) return fail("grid has %lld points, at most %lld are supported", cells, ds::RS_MAX_BINS);
        for (int i = 0; i < 9; ++i) {
            if (!std::isfinite(fold_inv[i])) return fail("fold_inv[%d] is not finite", i);
            A.fold_inv[i] = fold_inv[i];
        }
    }
    if (pair) {
        if (!latvec || !latvec_inv) return fail("ds_realspace_counts: the pair counts need latvec and latvec_inv");
        if (n_r < 1 || n_r > ds::RS_MAX_NR) return fail("n_r must be in 1..%d (got %d)", ds::RS_MAX_NR, n_r);
        if (!(r_max > 0.0) || !std::isfinite(r_max)) return fail("r_max must be positive and finite (got %g)", r_max);
        for (int i = 0; i < 9; ++i) {
            if (!std::isfinite(latvec[i]) || !std::isfinite(latvec_inv[i])) return fail("latvec / latvec_inv [%d] is not finite", i);
            A.a[i] = latvec[i];
            A.a_inv[i] = latvec_inv[i];
        }
        A.n_r = n_r;
        A.r_max = r_max;
    }
    hipStream_t st = (hipStream_t)stream;
    // pieces of at most RS_MAX_LAUNCH_WALKERS walkers: the bound behind the uint32 LDS bins (ds_realspace.h)
    for (int64_t b0 = 0; b0 < B; b0 += ds::RS_MAX_LAUNCH_WALKERS) {
        const long long nb = (long long)std::min<int64_t>(B - b0, ds::RS_MAX_LAUNCH_WALKERS);
        const dim3 grid_dim((unsigned)ds::rs_groups(nb)), block(ds::RS_THREADS);
        const size_t off = (size_t)b0 * 3 * (size_t)n_elec;
        if (dtype == 0)
            hipLaunchKernelGGL((ds::k_realspace_counts<double>), grid_dim, block, 0, st, A, (const double*)x + off, nb, (int)n_elec,
                               (unsigned long long*)dens, (unsigned long long*)pair);
        else
            hipLaunchKernelGGL((ds::k_realspace_counts<float>), grid_dim, block, 0, st, A, (const float*)x + off, nb, (int)n_elec,
                               (unsigned long long*)dens, (unsigned long long*)pair);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int ds_mh_propose(ds_system* s, const void* x1, const void* normal, double width, int64_t B, void* x2, void* stream) {
    if (!s || !x1 || !normal || !x2) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t ne = (size_t)B * s->sd.N;
    dim3 grid((unsigned)((ne + 255) / 256)), block(256);
    if (s->dtype == 0)
        hipLaunchKernelGGL((ds::k_mh_propose<double>), grid, block, 0, st, s->sd.sim_a, s->sd.sim_ainv, (const double*)x1,
                           (const double*)normal, width, ne, (double*)x2);
    else
        hipLaunchKernelGGL((ds::k_mh_propose<float>), grid, block, 0, st, s->sf.sim_a, s->sf.sim_ainv, (const float*)x1,
                           (const float*)normal, (float)width, ne, (float*)x2);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_mh_accept(ds_system* s, void* x1, void* lp1, const void* x2, const void* lp2, const void* uniform, int64_t B, void* n_accept,
                 void* stream) {
    if (!s || !x1 || !lp1 || !x2 || !lp2 || !uniform || !n_accept) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (s->dtype == 0)
        hipLaunchKernelGGL((ds::k_mh_accept<double>), dim3((unsigned)B), dim3(64), 0, st, (double*)x1, (double*)lp1, (const double*)x2,
                           (const double*)lp2, (const double*)uniform, 3 * s->sd.N, (double*)n_accept);
    else
        hipLaunchKernelGGL((ds::k_mh_accept<float>), dim3((unsigned)B), dim3(64), 0, st, (float*)x1, (float*)lp1, (const float*)x2,
                           (const float*)lp2, (const float*)uniform, 3 * s->sf.N, (float*)n_accept);
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
    dim3 grid((unsigned)((ne + 255) / 256)), block(256);
    if (s->dtype == 0) {
        if (mode == 2) hipLaunchKernelGGL((ds::k_max_norm3<double>), dim3(1), dim3(1024), 0, st, (const double*)aux, ne, (double*)scratch);
        hipLaunchKernelGGL((ds::k_mh_propose_ex<double>), grid, block, 0, st, s->sd.sim_a, s->sd.sim_ainv, mode, (const double*)x1,
                           (const double*)normal, width, (const double*)aux, n_aux, ne, (double*)x2, (const double*)scratch);
    } else {
        if (mode == 2) hipLaunchKernelGGL((ds::k_max_norm3<float>), dim3(1), dim3(1024), 0, st, (const float*)aux, ne, (float*)scratch);
        hipLaunchKernelGGL((ds::k_mh_propose_ex<float>), grid, block, 0, st, s->sf.sim_a, s->sf.sim_ainv, mode, (const float*)x1,
                           (const float*)normal, (float)width, (const float*)aux, n_aux, ne, (float*)x2, (const float*)scratch);
    }
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
    if (s->dtype == 0) {
        if (mode == 2) hipLaunchKernelGGL((ds::k_max_norm3<double>), dim3(1), dim3(1024), 0, st, (const double*)aux2, ne, (double*)scratch + 1);
        hipLaunchKernelGGL((ds::k_mh_accept_ex<double>), dim3((unsigned)B), dim3(64), 0, st, mode, (double*)x1, (double*)lp1, (const double*)x2,
                           (const double*)logabs2, (const double*)uniform, (const double*)normal, width, (const double*)aux1,
                           (const double*)aux2, n_aux, s->sd.N, (double*)n_accept, (const double*)scratch);
    } else {
        if (mode == 2) hipLaunchKernelGGL((ds::k_max_norm3<float>), dim3(1), dim3(1024), 0, st, (const float*)aux2, ne, (float*)scratch + 1);
        hipLaunchKernelGGL((ds::k_mh_accept_ex<float>), dim3((unsigned)B), dim3(64), 0, st, mode, (float*)x1, (float*)lp1, (const float*)x2,
                           (const float*)logabs2, (const float*)uniform, (const float*)normal, (float)width, (const float*)aux1,
                           (const float*)aux2, n_aux, s->sf.N, (float*)n_accept, (const float*)scratch);
    }
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
    return s->dtype == 0 ? mcmc_step_impl<double>(s, params, x, lp, B, steps, width, philox_seed, philox_offset, normals, uniforms,
                                                  lp_valid, n_accept, ws, ws_bytes, st)
                         : mcmc_step_impl<float>(s, params, x, lp, B, steps, width, philox_seed, philox_offset, normals, uniforms,
                                                 lp_valid, n_accept, ws, ws_bytes, st);
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
    return s->dtype == 0 ? mcmc_step_impl<double>(s, params, x, lp, B, moves, width, philox_seed, philox_offset, normals, uniforms,
                                                  lp_valid, n_accept, ws, ws_bytes, st, first_electron)
                         : mcmc_step_impl<float>(s, params, x, lp, B, moves, width, philox_seed, philox_offset, normals, uniforms,
                                                 lp_valid, n_accept, ws, ws_bytes, st, first_electron);
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
    return s->dtype == 0 ? mcmc_asymmetric_impl<double>(s, params, x, lp, B, steps, width, atoms, n_atoms, philox_seed, philox_offset,
                                                        normals, uniforms, lp_valid, n_accept, ws, ws_bytes, st)
                         : mcmc_asymmetric_impl<float>(s, params, x, lp, B, steps, width, atoms, n_atoms, philox_seed, philox_offset,
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
    return s->dtype == 0 ? mcmc_importance_impl<double>(s, params, x, lp, B, steps, width, philox_seed, philox_offset, normals, uniforms,
                                                        lp_valid, n_accept, ws, ws_bytes, st)
                         : mcmc_importance_impl<float>(s, params, x, lp, B, steps, width, philox_seed, philox_offset, normals, uniforms,
                                                       lp_valid, n_accept, ws, ws_bytes, st);
}

int64_t ds_one_body_workspace_bytes(const ds_system* s, int64_t B, int n_samples) {
    if (!s || B < 1 || n_samples < 1) return -1;
    // as many groups per chunk as ds_workspace_bytes gives the value chain of B * n_samples walkers
    const int64_t esz = s->dtype == 0 ? 8 : 4, total = B * (int64_t)n_samples;
    int64_t budget = (int64_t)80 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        budget = std::min<int64_t>(budget, std::max<int64_t>((int64_t)(free_b / 10 * 4), (int64_t)1 << 30));
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
    return s->dtype == 0 ? one_body_impl<double>(s, params, x, B, n_samples, first_electron, philox_seed, philox_offset, shifts, kvec,
                                                 n_k, nk_sums, out_ratio, out_shift, n_bad, ws, ws_bytes, st)
                         : one_body_impl<float>(s, params, x, B, n_samples, first_electron, philox_seed, philox_offset, shifts, kvec,
                                                n_k, nk_sums, out_ratio, out_shift, n_bad, ws, ws_bytes, st);
}

int ds_energy_stats(ds_system* s, const void* ke, const void* ewald, int64_t B, double* out_stats, void* stream) {
    if (!s || !ke || !ewald || !out_stats) return fail("null argument");
    hipStream_t st = (hipStream_t)stream;
    if (s->dtype == 0)
        hipLaunchKernelGGL((ds::k_energy_stats<double>), dim3(1), dim3(256), 0, st, (const double*)ke, (const double*)ewald, (long)B, out_stats);
    else
        hipLaunchKernelGGL((ds::k_energy_stats<float>), dim3(1), dim3(256), 0, st, (const float*)ke, (const float*)ewald, (long)B, out_stats);
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

int ds_orbitals(ds_system* s, const void* params, const void* x, int64_t B, void* out_up, void* out_dn, void* ws, int64_t ws_bytes,
                void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws || !out_up) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return s->dtype == 0 ? orbitals_impl<double>(s, params, x, B, out_up, out_dn, ws, ws_bytes, st)
                         : orbitals_impl<float>(s, params, x, B, out_up, out_dn, ws, ws_bytes, st);
}

int64_t ds_debug_stage(ds_system* s, const void* params, const void* x, int64_t B, const char* stage, void* out, int64_t out_elems,
                       void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !stage || !out || !ws) { fail("null argument"); return -1; }
    static const struct { const char* name; int stop; } names[] = {
        {"g0", STOP_G0}, {"g1", STOP_G1}, {"g2", STOP_G2}, {"g3", STOP_G3}, {"h2_0", STOP_H2_0}, {"h2_1", STOP_H2_1},
        {"h2_2", STOP_H2_2}, {"mean0", STOP_MEAN0}, {"q", STOP_Q}, {"mout", STOP_MOUT},
        {"minv", STOP_MINV}, {"dets", STOP_DETS}, {"tr", STOP_TR}};
    int stop = -1;
    for (auto& n : names)
        if (!strcmp(n.name, stage)) stop = n.stop;
    if (stop < 0) { fail("unknown stage '%s'", stage); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    const int64_t chunk = ws_bytes / (int64_t)(s->ws.per_walker * esz);
    if (chunk < B) { fail("debug stage needs the whole batch in one chunk"); return -1; }
    int rc;
    int64_t written;
    if (s->dtype == 0) {
        DumpReq<double> dr{stop, (double*)out, out_elems, 0};
        rc = run_chain<double>(s, (const double*)params, (const double*)x, B, arena_of<double>(ws, ws_bytes), st, nullptr, nullptr, nullptr, &dr);
        written = dr.written;
    } else {
        DumpReq<float> dr{stop, (float*)out, out_elems, 0};
        rc = run_chain<float>(s, (const float*)params, (const float*)x, B, arena_of<float>(ws, ws_bytes), st, nullptr, nullptr, nullptr, &dr);
        written = dr.written;
    }
    return rc ? -1 : written;
}

int ds_profile_enable(ds_system* s, int on) {
    if (!s) return fail("null argument");
    for (auto& v : s->prof_ev) {
        for (auto& p : v) { s->prof_pool.push_back(p.first); s->prof_pool.push_back(p.second); }
        v.clear();
    }
    s->prof_on = on != 0;
    s->prof_only = on >= 2 ? on - 2 : -1;      // on = 2 + kind: that kernel kind only
    if (on) HIP_OK(hipMemset(s->clk_dev, 0, 1024 * sizeof(unsigned long long)));
    return 0;
}

int ds_debug_timeline(ds_system* s, uint64_t* out, int n) {
    if (!s || !out || n < 0 || n > 1022) return fail("bad argument");
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, s->clk_dev + 2, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int ds_profile_read_clock(ds_system* s, double* shader_cycles, double* ref_ticks) {
    if (!s || !shader_cycles || !ref_ticks) return fail("null argument");
    unsigned long long h[2] = {0, 0};
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h, s->clk_dev, sizeof h, hipMemcpyDeviceToHost));
    *shader_cycles = (double)h[0];
    *ref_ticks = (double)h[1];
    return 0;
}

int ds_profile_read(ds_system* s, double* ms_total, int64_t* launches) {
    if (!s || !ms_total || !launches) return fail("null argument");
    if (s->prof_failed) { s->prof_failed = false; return fail("profiling: a HIP event could not be created or recorded; the timings are incomplete"); }
    for (int k = 0; k < DS_PROF_KINDS; ++k) {
        double tot = 0;
        for (auto& p : s->prof_ev[k]) {
            HIP_OK(hipEventSynchronize(p.second));
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, p.first, p.second));
            tot += ms;
        }
        ms_total[k] = tot;
        launches[k] = (int64_t)s->prof_ev[k].size();
    }
    return 0;
}

int ds_calib_copy(const void* src, void* dst, int64_t n_elems, void* stream) {
    if (!src || !dst) return fail("null argument");
    hipLaunchKernelGGL(ds::k_calib_copy, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, (const double*)src, (double*)dst, (size_t)n_elems);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t ds_mfma_f64_peak(int64_t iters, int blocks_per_cu, int n_acc, void* scratch, void* stream) {
    const int blocks = 256 * blocks_per_cu;   // 4-wave blocks: blocks_per_cu waves per SIMD
    hipStream_t st = (hipStream_t)stream;
    switch (n_acc) {
        case 1: hipLaunchKernelGGL(ds::k_mfma_peak<1>, dim3(blocks), dim3(256), 0, st, (long)iters, (double*)scratch); break;
        case 2: hipLaunchKernelGGL(ds::k_mfma_peak<2>, dim3(blocks), dim3(256), 0, st, (long)iters, (double*)scratch); break;
        case 4: hipLaunchKernelGGL(ds::k_mfma_peak<4>, dim3(blocks), dim3(256), 0, st, (long)iters, (double*)scratch); break;
        case 8: hipLaunchKernelGGL(ds::k_mfma_peak<8>, dim3(blocks), dim3(256), 0, st, (long)iters, (double*)scratch); break;
        case 16: hipLaunchKernelGGL(ds::k_mfma_peak<16>, dim3(blocks), dim3(256), 0, st, (long)iters, (double*)scratch); break;
        default: fail("n_acc must be 1, 2, 4, 8 or 16"); return -1;
    }
    return (int64_t)blocks * 4 * iters * n_acc * 2048;   // waves * iters * mfma per iter * flop per mfma
}

}  // extern "C"
