// ds_gradpass.hip -- the gradient passes (ds_grad.h) and the KFAC optimizer (ds_kfac.h): the reverse sweep behind ds_logpsi_vjp,
// ds_kfac_factors, ds_pretrain_loss_vjp, ds_logpsi_jacobian and ds_logpsi_ion_vjp, the Kronecker-factor pass, the per-walker emission
// (ds_jac.h) and the ion sink (ds_iongrad.h) that ride on it, and the KFAC step (damped inverses, preconditioner).  The forward of a pass is the value chain of ds_value.hip.
#include "ds_host.h"
#include "ds_grad.h"
#include "ds_kfac.h"
#include "ds_jac.h"
#include "ds_iongrad.h"

namespace ds {
namespace host {

// k_spin_mean (ds_grad.h) for the value chain too
template <typename T> void launch_spin_mean(dim3 grid, hipStream_t st, const ds::SysDev<T>& S, const T* G, int Kh, T* MEAN) {
    hipLaunchKernelGGL((ds::k_spin_mean<T>), grid, dim3(256), 0, st, S, G, Kh, MEAN);
}
template void launch_spin_mean<double>(dim3, hipStream_t, const ds::SysDev<double>&, const double*, int, double*);
template void launch_spin_mean<float>(dim3, hipStream_t, const ds::SysDev<float>&, const float*, int, float*);

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
GradBufs<T> carve_grad(const ds_system* s, const GradPlan& gp, Arena<T>& a, int64_t ng, bool pair_bwd = true) {
    // pair_bwd false: the ion pass (ds_logpsi_ion_vjp), which runs no pair-stream backward and carves none of its buffers
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
    if (pair_bwd) {
        for (T*& h : b.H2BAR) h = a.take(gp.h2 * ng);
        b.Z2BAR = a.take(gp.h2 * ng);
    }
    b.PART = a.take((size_t)s->nparams * ng);
    if (pair_bwd) b.W2S = a.take(gp.w2s * ng);              // split partials of the pair-stream weight gradients
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

// The per-walker sink of the sweep (ds_logpsi_jacobian, ds_jac.h): row w of `rows` (leading dimension ld) receives walker w's own
// gradient of every parameter block, from the operands the batch-summed gradient is formed from
template <typename T> struct JacSink {
    T* rows;
    size_t ld;
};

// The ion sink of the sweep (ds_logpsi_ion_vjp, ds_iongrad.h): out (walkers of the chunk, A, 3) receives every walker's own
// gradient in the positions of the primitive cell's atoms
struct IonSink {
    double* out;
};

// PHIBAR / QBAR of a chunk -> parameter gradient: grad = (first ? 0 : grad) + this chunk's sums
template <typename T>
int sweep_from_seed(ds_system* s, const GradPlan& gp, const GradBufs<T>& gb, const T* params, const T* WT, const T* x, int64_t Bc,
                    bool first, T* grad, hipStream_t st, const KfacSink<T>* ks = nullptr, const JacSink<T>* js = nullptr,
                    const IonSink* is = nullptr) {
    // ks: the KFAC factor pass (ds_kfac_factors) -- every tagged layer's A and G from the operands of its weight gradient;
    // grad may then be null (no packed gradient wanted)
    // js: the per-walker emission (ds_logpsi_jacobian).  The batch-summed contractions are then not launched at all (grad is null:
    // nobody reads PART); the cotangent chain itself is the same.  With js null nothing below differs from the plain sweep.
    // is: the ion sink (ds_logpsi_ion_vjp).  Only the one-electron cotangent chain runs: nothing that forms a parameter sum is
    // launched (no outer product, row sum, envelope gradient, PART memset or reduction) and the pair-stream backward is left out
    // altogether -- the pair stream reads neither the ions nor the one-electron stream.  Behind layer 0's element-wise kernel
    // k_ion_grad takes ZBAR / SBAR / HB / QBAR to the atoms.  With is null nothing below differs from the plain sweep.
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
        if (!is) HIP_OK(hipMemsetAsync(PART, 0, np * ng * sizeof(T), st));
        const size_t gws = (size_t)S.N * S.ldk * PV, gts = (size_t)S.ldk * PV;
        // per-walker emission of one block: the operands of `outer` (X null: a row of ones); pair: the pair layout of k_two_bwd
        auto emit = [&](const T* X, size_t xg, size_t xt, int ldx, const T* Z, size_t zg, size_t zt, int ldz, int nt, int K, int Nc,
                        size_t off, bool pair) {
            const unsigned nblk = (unsigned)(((K + 31) / 32) * ((Nc + 63) / 64));
            hipLaunchKernelGGL((ds::k_jac_outer<T>), dim3(nblk, (unsigned)Bc), dim3(256), 0, st, X, xg, xt, ldx, Z, zg, zt, ldz, nt, K, Nc,
                               pair ? S.NP : 0, S.N * S.N, (long)Bc, js->rows, js->ld, off);
        };
        auto outer = [&](const T* X, size_t xg, size_t xt, int ldx, const T* Z, size_t zg, size_t zt, int ldz, int nt, int J, int K,
                         int Nc, size_t off, int nsplit = 1) {
            if (is) return;
            if (js) { emit(X, xg, xt, ldx, Z, zg, zt, ldz, nt, K, Nc, off, nsplit > 1); return; }      // (only the pair layers split)
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
            if (S.bias_orb && js)
                hipLaunchKernelGGL((ds::k_jac_orb_bias<T>), dim3((unsigned)Bc), dim3(256), 0, st, PB[sp], pgs, ns, OC, S.nparam[sp], (long)Bc,
                                   js->rows, js->ld, boff(s->i_borb[sp]));
            else if (S.bias_orb && !is)
                hipLaunchKernelGGL((ds::k_orb_bias_grad<T>), dim3(2 * S.nparam[sp], (unsigned)ng), dim3(256), 0, st, PB[sp], pgs, ns, OC,
                                   S.nparam[sp], PART + boff(s->i_borb[sp]), np);
            const int Kop = gp.korb_pad;
            dim3 block; unsigned gz;
            gemm_geom(Kop, 4, &block, &gz);
            launch_gemm_plain<T>(dim3(ns, (unsigned)ng, gz), block, st, PB[sp], pgs, (size_t)OC * PV,
                               WT + gp.worbT[sp], OC, (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, ns, GBAR + (size_t)i0 * Kop * PV,
                               (size_t)S.N * Kop * PV, (size_t)0, Kop, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            if (s->use_last) {
                // shared term of the orbital head (network.py:535): S_orb = W_sh^T mean_i h_i, one per spin channel
                const int Ksh = S.nch * Kl;
                if (sp == 0 && !is)
                    launch_spin_mean<T>(dim3((unsigned)((Ksh * PV + 255) / 256), (unsigned)ng), st, S, vb.Gl[L], Kl, MEANL);
                hipLaunchKernelGGL((ds::k_sum_tiles<T>), dim3((unsigned)((OC * PV + 255) / 256), (unsigned)ng), dim3(256), 0, st, PB[sp], pgs, ns,
                                   OC * PV, SBAR);
                outer(MEANL, (size_t)Ksh * PV, 0, PV, SBAR, (size_t)OC * PV, 0, PV, 1, PV, Ksh, OC, boff(s->i_wsh_orb[sp]));
                gemm_geom(Ksh, 4, &block, &gz);
                launch_gemm_plain<T>(dim3(1, (unsigned)ng, gz), block, st, (const T*)nullptr, (size_t)0, (size_t)0,
                                   (const T*)nullptr, 0, SBAR, (size_t)OC * PV, WT + gp.wshorbT[sp], OC, 0, sp == 0 ? MEANBAR : MEANBAR2,
                                   (size_t)Ksh * PV, (size_t)0, Ksh, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            }
        }
        if (js)
            hipLaunchKernelGGL((ds::k_jac_env<T>), dim3((unsigned)Bc, S.nch), dim3(256), 0, st, S, x, (long)Bc, vb.Gl[0], QBAR,
                               blk(s->i_pi[0]), blk(s->i_sg[0]), blk(s->i_pi[S.nch - 1]), blk(s->i_sg[S.nch - 1]), js->rows, js->ld,
                               (long)boff(s->i_pi[0]), (long)boff(s->i_sg[0]), (long)boff(s->i_pi[S.nch - 1]), (long)boff(s->i_sg[S.nch - 1]));
        else if (!is)
            hipLaunchKernelGGL((ds::k_env_grad<T>), dim3((unsigned)ng, S.nch), dim3(256), 0, st, S, x, (long)Bc, vb.Gl[0], QBAR,
                               blk(s->i_pi[0]), blk(s->i_sg[0]), blk(s->i_pi[S.nch - 1]), blk(s->i_sg[S.nch - 1]), PART, np,
                               (long)boff(s->i_pi[0]), (long)boff(s->i_sg[0]), (long)boff(s->i_pi[S.nch - 1]), (long)boff(s->i_sg[S.nch - 1]));
        // ---- layers, last to first
        const T* D1 = GBAR; int ld1 = gp.korb_pad; const T* MB = s->use_last ? MEANBAR : nullptr; const T* CARRY = nullptr;
        const T* MB2 = s->use_last && S.nch > 1 ? MEANBAR2 : nullptr;
        int hbi = 0, h2i = 0;
        if (s->use_last && !is)       // the last level of the pair stream feeds the orbital head only
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
            if (is && l == 0) {
                const T* carry = res ? (const T*)HBc : (const T*)nullptr;
                const dim3 igrid((unsigned)S.A, (unsigned)ng), iblock(4 * PV);
#define DS_IONG(NF) hipLaunchKernelGGL((ds::k_ion_grad<T, NF>), igrid, iblock, 0, st, S, x, (long)Bc, (const T*)ZBAR, (const T*)SBAR, carry, Nout, \
                                       blk(s->i_wloc[0]), blk(s->i_wsh[0]), (const T*)QBAR, blk(s->i_pi[0]), blk(s->i_sg[0]), blk(s->i_pi[S.nch - 1]),    \
                                       blk(s->i_sg[S.nch - 1]), is->out)
                if (S.nf == 4) DS_IONG(4); else DS_IONG(7);
#undef DS_IONG
                break;
            }
            if (js)      // b[l]: the walker's row sums of ZBAR over the electrons
                emit(nullptr, 0, 0, 0, ZBAR, (size_t)S.N * Nout * PV, (size_t)Nout * PV, PV, S.N, 1, Nout, boff(s->i_b[l]), false);
            outer(vb.Gl[l], gws, gts, PV, ZBAR, (size_t)S.N * Nout * PV, (size_t)Nout * PV, PV, S.N, PV, Kloc, Nout, boff(s->i_wloc[l]));
            if (ks) {
                KfacOperands<T> o;
                o.X = walker_tiles<T>(vb.Gl[l], gws, gts, S.N);
                o.Z = walker_tiles<T>(ZBAR, (size_t)S.N * Nout * PV, (size_t)Nout * PV, S.N);
                o.Gaux = vb.Gl[l]; o.e0 = 0; o.ne = S.N;
                kfac_emit<T>(s, *ks, ks->kp->blocks[l], o, 1, Bc, st);
            }
            const T* MEANl = vb.MEAN0;
            if (l > 0 && !is) {
                launch_spin_mean<T>(dim3((unsigned)((S.nch * Kh * PV + 255) / 256), (unsigned)ng), st, S, vb.Gl[l], Kh, MEANL);
                MEANl = MEANL;
            }
            outer(MEANl, (size_t)Ksh * PV, 0, PV, SBAR, (size_t)Nout * PV, 0, PV, 1, PV, Ksh, Nout, boff(s->i_wsh[l]));
            const int Kpad = gp.kpad[l];
            if (l > 0) {
                dim3 block; unsigned gz;
                gemm_geom(Kpad, 4, &block, &gz);
                launch_gemm_plain<T>(dim3(S.N, (unsigned)ng, gz), block, st, ZBAR, (size_t)S.N * Nout * PV,
                                   (size_t)Nout * PV, WT + gp.wlocT[l], Nout, (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, S.N, GBAR,
                                   (size_t)S.N * Kpad * PV, (size_t)0, Kpad, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
                gemm_geom(Ksh, 4, &block, &gz);
                launch_gemm_plain<T>(dim3(1, (unsigned)ng, gz), block, st, (const T*)nullptr, (size_t)0,
                                   (size_t)0, (const T*)nullptr, 0, SBAR, (size_t)Nout * PV, WT + gp.wshT[l], Nout, 0, MEANBAR,
                                   (size_t)Ksh * PV, (size_t)0, Ksh, PV, (const T*)nullptr, (const T*)nullptr, ds::OrbEpi<T>{});
            }
            // pair stream
            const dim3 pgrid((S.NP / 16 + 3) / 4, (unsigned)(ng * (PV / 5)));
            if (is) {
                // (no pair-stream backward)
            } else if (l == S.n_double) {
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
                if (js)  // b2[l]: the walker's row sums of Z2BAR over its pairs
                    emit(nullptr, 0, 0, 0, Z2BAR, (size_t)(PV / 5) * K2o * J, (size_t)K2o * J, J, PV / 5, 1, K2o, boff(s->i_b2[l]), true);
                else
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
GradWs<T> carve_grad_pass(const ds_system* s, const GradPlan& gp, const KfacPlan* kp, bool dets, Arena<T>& a, int64_t ng,
                          bool seedbuf = false) {
    GradWs<T> w{};
    w.WT = a.take(gp.wt_total);
    w.gb = carve_grad<T>(s, gp, a, ng);
    if (seedbuf && !kp) w.cot = a.take((size_t)2 * ds::PV * ng);      // the Jacobian pass: its one-hot seeds
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

inline PassSize grad_pass_size(const ds_system* s, const GradPlan& gp, const KfacPlan* kp, bool seedbuf = false) {
    auto extent = [&](int64_t ng) { return measure([&](Arena<double>& a) { carve_grad_pass<double>(s, gp, kp, true, a, ng, seedbuf); }); };
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

// The ion pass (ds_logpsi_ion_vjp, ds_iongrad.h): the value chain and the seed of ds_logpsi_vjp, then the sweep with the ion sink.
// Its workspace is that of a gradient pass without the pair-stream cotangents: [transposed weights | ng groups of carve_grad].
template <typename T> GradWs<T> carve_ion_pass(const ds_system* s, const GradPlan& gp, Arena<T>& a, int64_t ng) {
    GradWs<T> w{};
    w.WT = a.take(gp.wt_total);
    w.gb = carve_grad<T>(s, gp, a, ng, false);
    return w;
}

inline PassSize ion_pass_size(const ds_system* s, const GradPlan& gp) {
    auto extent = [&](int64_t ng) { return measure([&](Arena<double>& a) { carve_ion_pass<double>(s, gp, a, ng); }); };
    return PassSize{extent(0), extent(1) - extent(0)};
}

int64_t ion_pass_bytes(const ds_system* s, int64_t B) {
    GradPlan gp;
    if (grad_plan(s, &gp)) return -1;
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    const int64_t groups = groups_per_pass(B, esz, ion_pass_size(s, gp), (int64_t)32 << 30);
    return (int64_t)measure([&](Arena<double>& a) { carve_ion_pass<double>(s, gp, a, groups); }) * esz + 256;
}

// groups of the ion pass that fit ws_bytes (< 1: refused by the entry point before any launch)
int64_t ion_pass_groups(const ds_system* s, int64_t ws_bytes) {
    GradPlan gp;
    if (grad_plan(s, &gp)) return -1;
    return groups_that_fit(ws_bytes, s->dtype == 0 ? 8 : 4, ion_pass_size(s, gp));
}

template <typename T>
int logpsi_ion_vjp_impl(ds_system* s, const void* params_, const void* x_, int64_t B, const void* cot_, double* out, void* out_logabs_,
                        void* out_phase_, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int PV = ds::PV;
    const T *params = (const T*)params_, *cot = (const T*)cot_;
    T *out_logabs = (T*)out_logabs_, *out_phase = (T*)out_phase_;
    GradPlan gp;
    if (int rc = grad_plan(s, &gp)) return rc;
    const int64_t cg = groups_that_fit(ws_bytes, sizeof(T), ion_pass_size(s, gp));
    if (cg < 1) return fail("workspace too small for ds_logpsi_ion_vjp: %lld bytes", (long long)ws_bytes);
    bool first = true;
    for (int64_t b0 = 0; b0 < B; b0 += cg * PV) {
        const int64_t Bc = std::min<int64_t>(cg * PV, B - b0);
        const T* x = (const T*)x_ + b0 * 3 * S.N;
        Arena<T> a = arena_of<T>(ws, ws_bytes);
        const GradWs<T> w = carve_ion_pass<T>(s, gp, a, (Bc + PV - 1) / PV);
        if (!a.ok) return carve_fail("ds_logpsi_ion_vjp");
        ProfScope ps(s, DS_PROF_ION_VJP, st);
        if (first) grad_transposes<T>(s, gp, params, w.WT, st);
        if (int rc = run_value_chain<T>(s, params, x, Bc, w.gb.vb, st, out_logabs ? out_logabs + b0 : nullptr,
                                        out_phase ? out_phase + 2 * b0 : nullptr)) return rc;
        if (int rc = seed_logdet<T>(s, gp, w.gb, params, cot + 2 * b0, Bc, st)) return rc;
        const IonSink is{out + (size_t)b0 * S.A * 3};
        if (int rc = sweep_from_seed<T>(s, gp, w.gb, params, w.WT, x, Bc, true, (T*)nullptr, st, nullptr, nullptr, &is)) return rc;
        first = false;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// Per-walker Jacobian (ds_jac.h): per chunk the value chain once, then two reverse sweeps with the per-walker sink -- the seed
// (1, 0) on every walker fills the rows b (d log|psi_b|), the seed (0, 1) the rows B + b (d arg psi_b).  The sweep writes only
// its own cotangent buffers (and MEANL, the value chain's scratch): every activation the second sweep reads is still what the
// value chain left, so the chain is not rerun.  A chunk holds at most JAC_MAX_GROUPS groups (its walkers are a grid dimension).
constexpr int64_t JAC_MAX_GROUPS = 512;

int64_t jacobian_bytes(const ds_system* s, int64_t B) {
    GradPlan gp;
    if (grad_plan(s, &gp)) return -1;
    const int64_t esz = s->dtype == 0 ? 8 : 4;
    const int64_t groups = groups_per_pass(B, esz, grad_pass_size(s, gp, nullptr, true), (int64_t)32 << 30);
    return (int64_t)measure([&](Arena<double>& a) { carve_grad_pass<double>(s, gp, nullptr, true, a, groups, true); }) * esz + 256;
}

template <typename T>
int logpsi_jacobian_impl(ds_system* s, const void* params_, const void* x_, int64_t B, void* jac_, int64_t ld, void* out_logabs_,
                         void* out_phase_, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int PV = ds::PV;
    const T* params = (const T*)params_;
    T *jac = (T*)jac_, *out_logabs = (T*)out_logabs_, *out_phase = (T*)out_phase_;
    GradPlan gp;
    if (int rc = grad_plan(s, &gp)) return rc;
    int64_t cg = groups_that_fit(ws_bytes, sizeof(T), grad_pass_size(s, gp, nullptr, true));
    if (cg < 1) return fail("workspace too small for the per-walker Jacobian: %lld bytes", (long long)ws_bytes);
    cg = std::min(cg, JAC_MAX_GROUPS);
    bool first = true;
    for (int64_t b0 = 0; b0 < B; b0 += cg * PV) {
        const int64_t Bc = std::min<int64_t>(cg * PV, B - b0);
        const T* x = (const T*)x_ + b0 * 3 * S.N;
        Arena<T> a = arena_of<T>(ws, ws_bytes);
        const GradWs<T> w = carve_grad_pass<T>(s, gp, nullptr, true, a, (Bc + PV - 1) / PV, true);
        if (!a.ok) return carve_fail("the per-walker Jacobian");
        if (first) grad_transposes<T>(s, gp, params, w.WT, st);
        if (int rc = run_value_chain<T>(s, params, x, Bc, w.gb.vb, st, out_logabs ? out_logabs + b0 : nullptr,
                                        out_phase ? out_phase + 2 * b0 : nullptr)) return rc;
        for (int half = 0; half < 2; ++half) {
            T* rows = jac + (size_t)(half * B + b0) * (size_t)ld;
            hipLaunchKernelGGL((ds::k_jac_zero<T>), dim3((unsigned)((s->nparams + 255) / 256), (unsigned)Bc), dim3(256), 0, st, rows, (size_t)ld,
                               (long)s->nparams, (long)Bc);
            hipLaunchKernelGGL((ds::k_jac_seed<T>), dim3((unsigned)((Bc + 255) / 256)), dim3(256), 0, st, w.cot, (long)Bc, half);
            if (int rc = seed_logdet<T>(s, gp, w.gb, params, w.cot, Bc, st)) return rc;
            const JacSink<T> js{rows, (size_t)ld};
            if (int rc = sweep_from_seed<T>(s, gp, w.gb, params, w.WT, x, Bc, true, (T*)nullptr, st, nullptr, &js)) return rc;
        }
        first = false;
    }
    HIP_OK(hipGetLastError());
    return 0;
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

// ------------------------------------------------------------------ KFAC step (ds_kfac.h): damped inverses, preconditioner
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
    double* Tm = base + sp.o_t;                    // A^- V, float64 for either element type (o_t holds vtotal doubles)
    double* part = base + sp.o_part;
    const dim3 grid((unsigned)((sp.tiles_max + 3) / 4), (unsigned)sp.M.nb);
    hipLaunchKernelGGL((ds::k_kprec_gemm<T, 1>), grid, dim3(256), 0, st, sp.M, (const T*)inverses, (const T*)v, Tm, (const T*)v, part);
    hipLaunchKernelGGL((ds::k_kprec_gemm<T, 2>), grid, dim3(256), 0, st, sp.M, (const T*)inverses, (const double*)Tm, (T*)out, (const T*)v, part);
    hipLaunchKernelGGL(ds::k_kprec_final, dim3((unsigned)sp.M.nb), dim3(64), 0, st, sp.M, (const double*)part, sq);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

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
    return DS_BY_DTYPE(s->dtype, logpsi_vjp_impl, s, params, x, B, cot, grad, out_logabs, out_phase, ws, ws_bytes, st);
}

int64_t ds_ion_vjp_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s) return -1;
    return ion_pass_bytes(s, B);
}

int ds_logpsi_ion_vjp(ds_system* s, const void* params, const void* x, int64_t B, const void* cot, double* out, void* out_logabs,
                      void* out_phase, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !ws) return fail("ds_logpsi_ion_vjp: null argument");
    if (!x) return fail("ds_logpsi_ion_vjp: x is null");
    if (!cot) return fail("ds_logpsi_ion_vjp: cot is null");
    if (!out) return fail("ds_logpsi_ion_vjp: out is null");
    if (B < 1) return fail("ds_logpsi_ion_vjp: B must be >= 1 (got %lld)", (long long)B);
    const int64_t cg = ion_pass_groups(s, ws_bytes);
    if (cg < 1)
        return fail("workspace too small for ds_logpsi_ion_vjp: %lld bytes < %lld for one group of %d walkers (see ds_ion_vjp_workspace_bytes)",
                    (long long)ws_bytes, (long long)ion_pass_bytes(s, 1), ds::PV);
    return DS_BY_DTYPE(s->dtype, logpsi_ion_vjp_impl, s, params, x, B, cot, out, out_logabs, out_phase, ws, ws_bytes, (hipStream_t)stream);
}

int64_t ds_jacobian_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s) return -1;
    return jacobian_bytes(s, B);
}

int ds_logpsi_jacobian(ds_system* s, const void* params, const void* x, int64_t B, void* jac, int64_t ld, void* out_logabs,
                       void* out_phase, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params) return fail("null argument");
    if (B <= 0) return 0;                               // the empty batch has no rows
    if (!x || !jac || !ws) return fail("null argument");
    if (ld < s->nparams) return fail("ds_logpsi_jacobian: ld = %lld is smaller than the parameter count %lld", (long long)ld, (long long)s->nparams);
    return DS_BY_DTYPE(s->dtype, logpsi_jacobian_impl, s, params, x, B, jac, ld, out_logabs, out_phase, ws, ws_bytes, (hipStream_t)stream);
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
    return DS_BY_DTYPE(s->dtype, kfac_factors_impl, s, params, x, B, factors, grad_seed, ws, ws_bytes, st);
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
    return DS_BY_DTYPE(s->dtype, kfac_inverses_run, sp, factors, ema_weight, damping, inverses, ws, ws_bytes, (hipStream_t)stream);
}

int ds_kfac_precondition(ds_system* s, const void* inverses, const void* v, void* out, double* sq_norm, void* ws, int64_t ws_bytes,
                         void* stream) {
    if (!s || !inverses || !v || !out || !sq_norm || !ws) return fail("null argument");
    KfacStepPlan sp;
    if (int rc = kfac_step_plan(s, &sp, true)) return rc;
    return DS_BY_DTYPE(s->dtype, kfac_precondition_run, sp, inverses, v, out, sq_norm, ws, ws_bytes, (hipStream_t)stream);
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
    return DS_BY_DTYPE(dtype, kfac_inverses_run, sp, factors, ema_weight, damping, inverses, ws, ws_bytes, (hipStream_t)stream);
}

int64_t ds_pretrain_workspace_bytes(const ds_system* s, int64_t B) { return ds_vjp_workspace_bytes(s, B); }

int ds_pretrain_loss_vjp(ds_system* s, const void* params, const void* x, int64_t B, const void* target_up, const void* target_dn,
                         void* out_loss, void* grad, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !out_loss || !grad || !ws || (B > 0 && !x)) return fail("null argument");
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, pretrain_loss_vjp_impl, s, params, x, B, target_up, target_dn, out_loss, grad, ws, ws_bytes, st);
}

}  // extern "C"
