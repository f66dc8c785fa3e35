// ds_det.hip -- the determinant stage of both chains: inverse, determinant and traces of the forward-Laplacian chain, log det (and
// the inverses of a gradient pass) of the value chain.  The unrolled one-lane-per-row inverses are in ds_det_inst.hip.
#include "ds_host.h"
#include "ds_tiles.h"

namespace ds {
namespace host {

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

// Value chain: log det of every determinant channel into DETS -- and, for a gradient pass (vb.MINV), the inverses by the
// Gauss-Jordan kernel
template <typename T>
void launch_det_value(const ds_system* s, const ds::SysDev<T>& S, const ValBufs<T>& vb, int64_t Bc, hipStream_t st) {
    const WsLayout& L = s->wsv;
    const int PV = ds::PV;
    T* MOUT = vb.MOUT; T* DETS = vb.DETS;
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
}

#define DS_INST(T)                                                                                                      \
    template void launch_det_inverse<T>(const ds_system*, const ds::SysDev<T>&, const Carve<T>&, int, int64_t, hipStream_t); \
    template int launch_det_trace<T>(const ds_system*, const ds::SysDev<T>&, const Carve<T>&, int, int64_t, hipStream_t);    \
    template void launch_det_value<T>(const ds_system*, const ds::SysDev<T>&, const ValBufs<T>&, int64_t, hipStream_t);
DS_INST(double) DS_INST(float)
#undef DS_INST

}  // namespace host
}  // namespace ds
