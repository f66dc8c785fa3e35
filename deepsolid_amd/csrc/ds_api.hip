// ds_api.hip -- the handle of libdeepsolid_hip.so (see include/deepsolid_hip.h): the device tables of one simulation cell, the
// parameter blocks, the workspace layouts of the two chains, create / destroy, profiling, and the small entry points that keep no
// state.  The subsystems behind the handle have a unit each (ds_host.h lists them).
#include <cstdarg>

#include "ds_host.h"
#include "ds_tiles.h"

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

namespace ds {
namespace host {

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

int64_t workspace_budget() {
    int64_t budget = (int64_t)80 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        budget = std::min<int64_t>(budget, std::max<int64_t>((int64_t)(free_b / 10 * 4), (int64_t)1 << 30));
    return budget;
}

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

template <typename T>
void enforce_pbc(const double* latvec, const double* inv, const void* x, int64_t n_elec, void* out_x, void* out_wrap, hipStream_t st) {
    ds::Lattice<T> L;
    for (int i = 0; i < 9; ++i) { L.a[i] = (T)latvec[i]; L.ainv[i] = (T)inv[i]; }
    hipLaunchKernelGGL((ds::k_enforce_pbc<T>), dim3((unsigned)((n_elec + 255) / 256)), dim3(256), 0, st, L, (const T*)x, (size_t)n_elec, (T*)out_x,
                       (T*)out_wrap);
}

}  // namespace host

void set_last_error(const char* msg) { host::g_err = msg; }

}  // namespace ds

using namespace ds::host;

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
    s->use_pair_recompute = getenv("DS_NO_PAIR_RECOMPUTE") == nullptr;
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
        const size_t bytes = i8_planes_bytes(s);
        if (bytes && hipMalloc(&s->i8_wp, bytes) != hipSuccess) {
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
    const int64_t budget = workspace_budget();
    const int64_t cap = s->chunk_cap;
    int64_t chunk = std::min<int64_t>(std::max<int64_t>(B, 1), cap);
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, budget / ((int64_t)s->ws.per_walker * esz)));
    const int64_t groups = groups_per_pass(B, esz, PassSize{0, s->wsv.per_walker}, budget);
    return std::max((int64_t)s->ws.per_walker * esz * chunk, (int64_t)s->wsv.per_walker * esz * groups) + 256;
}

int ds_enforce_pbc(const double* latvec, int dtype, const void* x, int64_t n_elec, void* out_x, void* out_wrap, void* stream) {
    if (!latvec || !x || !out_x) return fail("null argument");
    if (n_elec <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    double inv[9];
    inv3(latvec, inv);
    if (dtype != 0 && dtype != 1) return fail("dtype must be 0 or 1");
    DS_BY_DTYPE(dtype, enforce_pbc, latvec, inv, x, n_elec, out_x, out_wrap, st);
    HIP_OK(hipGetLastError());
    return 0;
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
