// ds_chain.hip -- the forward-Laplacian (energy) chain: its plan, ds_local_energy, the walker gradient ds_logpsi_grad, the stage
// dumps and ds_ewald.
#include "ds_host.h"
#include "ds_tiles.h"

namespace ds {
namespace host {

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
    bool recompute_prev;                      // k_two_layer_expand<.., PREV>: the layer runs layer l - 1 in registers; that layer's output is not written
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
    // k_two_layer_expand's geometry for a pair layer of K2o output features, from whether it has a residual and whether its output is written
    auto pair_geom = [&](PairPlan& pp, int K2o) {
        pp.xz = (!pp.res && K2o == 32) ? 2 : 1;       // (a residual layer keeps its operands: all features in one workgroup)
        // two electrons per workgroup where the output is written and a single electron's pairs would end in the middle of a 128-byte line
        pp.EW = (pp.write_out && S.N % 16 == 8 && pp.xz == 2) ? 2 : 1;
        pp.NW = (pp.EW * S.N + 15) / 16;
        pp.xlds = ((size_t)(K2o / pp.xz) * 5 * pp.EW * S.N + (size_t)pp.EW * S.nch * (K2o / pp.xz) * 5) * sizeof(T);
    };
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
            pp.write_out = l + 1 < S.n_double || s->use_last;
            pair_geom(pp, K2o);
            // the layer and the spin means of its output in one kernel (a workgroup per electron) when the output jets of an electron's
            // pairs fit the LDS: the next level's rows land in the buffer the one-electron layer below writes its output to
            pp.expand = !dump && s->use_pair_expand && !pp.res_sep && l + 1 < S.n_layers && pp.NW <= 8 && pp.xlds <= 150 * 1024;
            // A float64 residual layer behind a layer without residual on at most two k-steps of input features (layer 1 behind layer 0:
            // 4 'nu' or 8 'tri' features) runs that layer itself and keeps its output as operands; the layer in front then writes the
            // pair-mean rows only (one electron per workgroup, which its LDS test above already passed with more).
            if (l >= 1) {
                PairPlan& prev = p->layer[l - 1].pair;
                pp.recompute_prev = sizeof(T) == 8 && !dump && s->use_pair_recompute && pp.res && pp.expand && S.h2[l - 1] <= 8 &&
                                    !prev.res && !prev.res_sep && prev.expand;
                if (pp.recompute_prev) {
                    prev.write_out = false;
                    pair_geom(prev, K2);
                }
            }
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
        } else if (int8_energy_layer(s, l)) {
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
                // (recompute_prev: layer l - 1 left c.H2[hi] unwritten -- its input is still in the other buffer, and an output goes
                //  to c.H2[hi] itself: the walkers of the input buffer are Kin, not K2o, features apart)
#define DS_TWOXP(NT2) hipLaunchKernelGGL((ds::k_two_layer_expand<T, NT2, true, true>), dim3(S.N / pp.EW, (unsigned)Bc, pp.xz), dim3(64 * pp.NW), pp.xlds, st, S, c.H2[hi ^ 1], S.h2[l - 1], W2, b2, \
                                         pp.write_out ? c.H2[hi] : (T*)nullptr, c.G[gi ^ 1], S.h1[l + 1], S.ldk, plan.layer[l + 1].pm_unwritten ? 1 : 0, pp.EW,               \
                                         blk(s->i_w2[l - 1]), blk(s->i_b2[l - 1]))
                if (pp.recompute_prev) {
                    if constexpr (sizeof(T) == 8) { if (K2o == 32) DS_TWOXP(2); else DS_TWOXP(1); }      // (plan_chain: float64 only)
                } else if (K2o == 32 && pp.res) DS_TWOX(2, true);
                else if (pp.res) DS_TWOX(1, true);
                else DS_TWOX(1, false);
#undef DS_TWOXP
#undef DS_TWOX
            } else {
                const dim3 grid((S.NP / 16 + 3) / 4, (unsigned)Bc);
#define DS_TWO(NT2, RES) hipLaunchKernelGGL((ds::k_two_layer<T, NT2, RES, false>), grid, dim3(256), 0, st, S, c.H2[hi], K2, W2, b2, c.H2[hi ^ 1])
                if (K2o == 32) { if (pp.res) DS_TWO(2, true); else DS_TWO(2, false); }
                else { if (pp.res) DS_TWO(1, true); else DS_TWO(1, false); }
#undef DS_TWO
            }
            if (pp.res_sep)
                launch_pair_res_add<T>(dim3((unsigned)(((size_t)K2o * 5 * S.NP + 255) / 256), (unsigned)Bc), st, c.H2[hi], K2, c.H2[hi ^ 1], K2o, S.nf, S.NP);
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
                launch_layer_i8(s, l, false, (const double*)blk(s->i_wloc[l]), Kloc, Nout, (const double*)c.G[gi], gts, (const double*)Sl,
                                (double*)c.G[gi ^ 1], (int)(Bc * S.N), st);
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
                    launch_layer_res_add<T>(dim3(S.N, (unsigned)Bc), st, Xin, xws, xts, c.G[gi ^ 1], gws, gts, S.nf * S.A, Nout, S.P);
                break;
            }
        }
        gi ^= 1;
        if (l < S.n_double) {
            if (!lp.pair.recompute_prev) hi ^= 1;      // (such a layer wrote, if at all, into the buffer the layer in front left unwritten)
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
// One pass with BOTH outputs of k_combine, plus the Ewald triple (the DMC step, ds_dmc.hip): ke (B,2), grad (B,3N,2), log|psi|,
// phase and ew3 (B,3), chunked by ws_bytes as the two functions above chunk it.
template <typename T>
int energy_grad_impl(ds_system* s, const void* params, const void* x, int64_t B, void* out_ke, void* out_ew3, void* out_logabs,
                     void* out_phase, void* out_grad, void* ws, int64_t ws_bytes, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int64_t chunk = std::min<int64_t>(ws_bytes / (int64_t)(s->ws.per_walker * sizeof(T)), 65535);
    if (chunk < 1) return fail("workspace too small: %lld bytes < %zu per walker", (long long)ws_bytes, s->ws.per_walker * sizeof(T));
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t Bc = std::min(chunk, B - b0);
        int rc = run_chain<T>(s, (const T*)params, (const T*)x + b0 * 3 * S.N, Bc, arena_of<T>(ws, ws_bytes), st, (T*)out_ke + 2 * b0,
                              (T*)out_logabs + b0, (T*)out_phase + 2 * b0, nullptr, (T*)out_grad + b0 * 3 * S.N * 2);
        if (rc) return rc;
    }
    {
        ProfScope ps(s, DS_PROF_EWALD, st);
        hipLaunchKernelGGL((ds::k_ewald<T>), dim3((unsigned)B), dim3(256), ds::ewald_lds_bytes(S), st, S, (const T*)x, (T*)out_ew3);
    }
    HIP_OK(hipGetLastError());
    return 0;
}
int energy_grad_forward(ds_system* s, const void* params, const void* x, int64_t B, void* out_ke, void* out_ew3, void* out_logabs,
                        void* out_phase, void* out_grad, void* ws, int64_t ws_bytes, hipStream_t st) {
    return DS_BY_DTYPE(s->dtype, energy_grad_impl, s, params, x, B, out_ke, out_ew3, out_logabs, out_phase, out_grad, ws, ws_bytes, st);
}

// the Ewald triple (ee, ei, ii) per walker: out (B, 3)
template <typename T> void ewald_triple(ds_system* s, const void* x, int64_t B, void* out, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    size_t sh = ds::ewald_lds_bytes(S);
    hipLaunchKernelGGL((ds::k_ewald<T>), dim3((unsigned)B), dim3(256), sh, st, S, (const T*)x, (T*)out);
}

// the chain up to stage `stop` on the whole batch: elements written to `out`, or -1
template <typename T>
int64_t debug_stage_impl(ds_system* s, const void* params, const void* x, int64_t B, int stop, void* out, int64_t out_elems, void* ws,
                         int64_t ws_bytes, hipStream_t st) {
    DumpReq<T> dr{stop, (T*)out, out_elems, 0};
    const int rc = run_chain<T>(s, (const T*)params, (const T*)x, B, arena_of<T>(ws, ws_bytes), st, nullptr, nullptr, nullptr, &dr);
    return rc ? -1 : dr.written;
}

int logpsi_grad_forward(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* out_grad,
                        void* ws, int64_t ws_bytes, hipStream_t st) {
    return DS_BY_DTYPE(s->dtype, logpsi_grad_impl, s, params, x, B, out_logabs, out_phase, out_grad, ws, ws_bytes, st);
}

// layers of the energy chain that run as an int8 split (dump: in a stage dump, which has no low-rank layer 1)
int int8_energy_layers(const ds_system* s, bool dump) {
    ChainPlan<double> plan;
    return plan_chain<double>(s, dump, &plan) == 0 ? plan.count(LayerKind::Int8, s->sd.n_layers) : 0;
}

// pair layers of the handle's energy chain that run the layer in front of them in registers (PairPlan::recompute_prev)
template <typename T> int pair_recompute_count(const ds_system* s, bool dump) {
    ChainPlan<T> plan;
    if (plan_chain<T>(s, dump, &plan)) return 0;
    int n = 0;
    for (int l = 0; l < s->sd.n_double && l < s->sd.n_layers; ++l) n += plan.layer[l].pair.recompute_prev ? 1 : 0;
    return n;
}

template <typename T> void launch_pair_res_add(dim3 grid, hipStream_t st, const T* Hin, int Kin, T* Hout, int Kout, int n_res, int NP) {
    hipLaunchKernelGGL((ds::k_pair_res_add<T>), grid, dim3(256), 0, st, Hin, Kin, Hout, Kout, n_res, NP);
}

template <typename T>
void launch_layer_res_add(dim3 grid, hipStream_t st, const T* Xin, size_t x_ws, size_t x_ts, T* Gout, size_t g_ws, size_t g_ts, int n_res,
                          int Nout, int P) {
    hipLaunchKernelGGL((ds::k_layer_res_add<T>), grid, dim3(256), 0, st, Xin, x_ws, x_ts, Gout, g_ws, g_ts, n_res, Nout, P);
}

#define DS_INST(T)                                                                                      \
    template void launch_pair_res_add<T>(dim3, hipStream_t, const T*, int, T*, int, int, int);          \
    template void launch_layer_res_add<T>(dim3, hipStream_t, const T*, size_t, size_t, T*, size_t, size_t, int, int, int);
DS_INST(double) DS_INST(float)
#undef DS_INST

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

int ds_int8_layers(const ds_system* s) {
    if (!s) return -1;
    return int8_energy_layers(s, false);
}

int ds_pair_recompute_layers(const ds_system* s, int dump) {
    if (!s) return -1;
    return s->dtype == 0 ? pair_recompute_count<double>(s, dump != 0) : pair_recompute_count<float>(s, dump != 0);
}

int ds_local_energy(ds_system* s, const void* params, const void* x, int64_t B, void* out_ke, void* out_ewald, void* out_logabs,
                    void* out_phase, void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, local_energy_impl, s, params, x, B, out_ke, out_ewald, out_logabs, out_phase, ws, ws_bytes, st);
}

int ds_logpsi_grad(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* out_grad,
                   void* ws, int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws || !out_grad) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return logpsi_grad_forward(s, params, x, B, out_logabs, out_phase, out_grad, ws, ws_bytes, st);
}

int ds_ewald(ds_system* s, const void* x, int64_t B, void* out, void* stream) {
    if (!s || !x || !out) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    DS_BY_DTYPE(s->dtype, ewald_triple, s, x, B, out, st);
    HIP_OK(hipGetLastError());
    return 0;
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
    return DS_BY_DTYPE(s->dtype, debug_stage_impl, s, params, x, B, stop, out, out_elems, ws, ws_bytes, st);
}

}  // extern "C"
