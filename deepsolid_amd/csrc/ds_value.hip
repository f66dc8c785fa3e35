// ds_value.hip -- the value chain (log psi and the orbital matrices, ds_value.h) on groups of PV walkers: ds_logpsi, ds_orbitals, the
// forward of the samplers and of the gradient passes.  The int8 split of ds_i8.h lives here for both chains.
#include "ds_host.h"
#include "ds_i8.h"

namespace ds {
namespace host {

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

// ---------------------------------------------------------------- the int8 split (ds_i8.h), for both chains
// A dense residual hidden layer l with the shape of the int8 split (ds_i8.h: float64, 256 features from K = 320 rows).
inline bool i8_shape(const ds_system* s, int l) {
    const ds::SysDev<double>& S = s->sd;
    return s->dtype == 0 && l >= 1 && s->res1[l] && S.h1[l + 1] == ds::i8::NOUT && S.h1[l] + S.nch * S.h2[l] == 320;
}
// The slot axis and the switch are the caller's: the energy chain (plan_chain: 5 slot tiles) ...
bool int8_energy_layer(const ds_system* s, int l) { return s->use_i8 && s->sd.P == ds::i8::P && i8_shape(s, l); }
// ... and the value chain (its column axis is 80 walkers whatever the electron count: any float64 cell with such a layer; whether a
// call takes it depends on its batch)
bool int8_value_layer(const ds_system* s, int l) { return s->use_i8_val && ds::PV == ds::i8::P && i8_shape(s, l); }

// digit planes + column scales of layer l's per-electron weights: prepared by the first launch of a C-ABI call that needs them (the
// 20 forwards of an mcmc_step, the chunks of a local-energy batch and the value / energy chains of one call share them)
inline size_t i8_slot_bytes() { return ds::i8::wp_bytes(64 * 5) + ds::i8::NOUT * sizeof(double); }
inline void i8_prepare(ds_system* s, int l, const double* Wloc, int Kloc, int Nout, hipStream_t st, uint8_t** wp, double** sw) {
    *wp = (uint8_t*)s->i8_wp + (size_t)l * i8_slot_bytes();
    *sw = (double*)(*wp + ds::i8::wp_bytes(64 * 5));
    if (s->i8_prepped[l] != s->call_seq) {
        hipLaunchKernelGGL(ds::i8::k_i8_prep_w, dim3(ds::i8::NOUT / 16), dim3(256), 0, st, Wloc, Kloc, Nout, *wp, *sw);
        s->i8_prepped[l] = s->call_seq;
    }
}

size_t i8_planes_bytes(const ds_system* s) {
    // (the energy chain has the most int8 layers in a stage dump)
    bool need = int8_energy_layers(s, true) > 0;
    for (int l = 1; l < s->sd.n_layers; ++l) need = need || int8_value_layer(s, l);
    return need ? (size_t)DS_MAX_LAYERS * i8_slot_bytes() : 0;
}

// A layer as an int8 split: the energy chain's epilogue (value_epilogue false, tiles = (walker, electron)) or the value chain's
// (tiles = (80-walker group, electron)); one persistent workgroup per CU
void launch_layer_i8(ds_system* s, int l, bool value_epilogue, const double* Wloc, int Kloc, int Nout, const double* Gin, size_t tile_stride,
                     const double* Sb, double* Gout, int ntiles, hipStream_t st) {
    uint8_t* wp; double* sw;
    i8_prepare(s, l, Wloc, Kloc, Nout, st, &wp, &sw);
    const dim3 grid((unsigned)std::min<int64_t>(ntiles, s->n_cu));
    if (value_epilogue)
        hipLaunchKernelGGL((ds::i8::k_layer_i8<5, 4>), grid, dim3(512), ds::i8::lds_bytes(), st, Gin, tile_stride, (const uint4*)wp, sw, Sb, s->sd.N,
                           Gout, ntiles);
    else
        hipLaunchKernelGGL((ds::i8::k_layer_i8<5, 2>), grid, dim3(512), ds::i8::lds_bytes(), st, Gin, tile_stride, (const uint4*)wp, sw, Sb, s->sd.N,
                           Gout, ntiles);
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
                launch_pair_res_add<T>(dim3((unsigned)(((size_t)K2o * 5 * S.NP + 255) / 256), (unsigned)(ng * (PV / 5))), st, Hin, K2, Hnext, K2o, S.nf, S.NP);
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
            launch_spin_mean<T>(dim3((unsigned)((Ksh * PV + 255) / 256), (unsigned)ng), st, S, Gin, Kh, vb.MEANS);
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
        const bool i8_tiles = s->val_i8_call ? s->val_i8_call > 0 : (int64_t)S.N * ng >= (int64_t)s->val_i8_min_tiles;
        if (sizeof(T) == 8 && int8_value_layer(s, l) && i8_tiles) {
            launch_layer_i8(s, l, true, (const double*)blk(s->i_wloc[l]), Kloc, Nout, (const double*)Gin, gts, (const double*)ZB, (double*)Gout,
                                  (int)(S.N * ng), st);
        } else if (s->res1[l] && !res_sep) {
            if (nbh == 4) DS_VHID(4) else if (nbh == 2) DS_VHID(2) else DS_VHID(1)
        } else {
#undef DS_VHID
            hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 3>), dim3(S.N, (unsigned)ng, gz), block, 0, st, Gin, gws, gts, blk(s->i_wloc[l]), Kloc,
                               (const T*)nullptr, (size_t)0, (const T*)nullptr, 0, S.N, Gout, gws, gts, Nout, PV, ZB, blk(s->i_b[l]), ds::OrbEpi<T>{});
            if (res_sep)
                launch_layer_res_add<T>(dim3(S.N, (unsigned)ng), st, (const T*)Gin, gws, gts, Gout, gws, gts, S.nf * S.A, Nout, PV);
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
            launch_gemm_plain<T>(dim3(ns, (unsigned)ng, ogz), oblock, st, Gl + (size_t)i0 * S.ldk * PV,
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
        launch_det_value<T>(s, S, vb, Bc, st);
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

int logpsi_forward(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* ws, int64_t ws_bytes,
                   hipStream_t st) {
    return DS_BY_DTYPE(s->dtype, logpsi_impl, s, params, x, B, out_logabs, out_phase, ws, ws_bytes, st);
}

template <typename T>
void launch_gemm_plain(dim3 grid, dim3 block, hipStream_t st, const T* X, size_t x_walker_stride, size_t x_tile_stride, const T* W, int K,
                       const T* X2, size_t x2_walker_stride, const T* W2, int K2, int n_tiles, T* Z, size_t z_walker_stride,
                       size_t z_tile_stride, int Nout, int P, const T* Sb, const T* bias, const ds::OrbEpi<T>& oe) {
    hipLaunchKernelGGL((ds::k_jet_gemm<T, 4, 5, 0>), grid, block, 0, st, X, x_walker_stride, x_tile_stride, W, K, X2, x2_walker_stride, W2, K2,
                       n_tiles, Z, z_walker_stride, z_tile_stride, Nout, P, Sb, bias, oe);
}

#define DS_INST(T)                                                                                                                   \
    template int run_value_chain<T>(ds_system*, const T*, const T*, int64_t, const ValBufs<T>&, hipStream_t, T*, T*);                    \
    template void launch_gemm_plain<T>(dim3, dim3, hipStream_t, const T*, size_t, size_t, const T*, int, const T*, size_t, const T*, int, \
                                       int, T*, size_t, size_t, int, int, const T*, const T*, const ds::OrbEpi<T>&);
DS_INST(double) DS_INST(float)
#undef DS_INST

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

int ds_logpsi(ds_system* s, const void* params, const void* x, int64_t B, void* out_logabs, void* out_phase, void* ws,
              int64_t ws_bytes, void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return logpsi_forward(s, params, x, B, out_logabs, out_phase, ws, ws_bytes, st);
}

int ds_orbitals(ds_system* s, const void* params, const void* x, int64_t B, void* out_up, void* out_dn, void* ws, int64_t ws_bytes,
                void* stream) {
    if (s) ++s->call_seq;
    if (!s || !params || !x || !ws || !out_up) return fail("null argument");
    if (B <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return DS_BY_DTYPE(s->dtype, orbitals_impl, s, params, x, B, out_up, out_dn, ws, ws_bytes, st);
}

}  // extern "C"
