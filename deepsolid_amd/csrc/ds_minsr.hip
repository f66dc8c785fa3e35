// ds_minsr.hip -- host side of ds_minsr.h: Gram matrix, matrix-vector products and the damped centred solve on a per-walker
// Jacobian (ds_minsr_gram, ds_minsr_matvec, ds_minsr_solve).  No system handle.
#include "ds_host.h"
#include "ds_minsr.h"

namespace ds {
namespace host {

struct GramPlan {
    int nb = 0, tiles = 0, nsplit = 1;
    long pchunk = 0;
};

// the split of the P axis depends on the shape alone: 512 workgroups wanted, at least 1024 columns each
int gram_plan(int64_t R, int64_t P, GramPlan* g) {
    if (R < 1 || P < 1 || R > 46340) return fail("ds_minsr_gram: R must lie in [1, 46340] and P must be positive");
    g->nb = (int)((R + ds::MINSR_TM - 1) / ds::MINSR_TM);
    g->tiles = g->nb * (g->nb + 1) / 2;
    int64_t ns = std::max<int64_t>(1, 512 / g->tiles);
    ns = std::min<int64_t>(ns, std::max<int64_t>(1, P / 1024));
    g->pchunk = (long)rup((P + ns - 1) / ns, ds::MINSR_KC);
    g->nsplit = (int)((P + g->pchunk - 1) / g->pchunk);
    return 0;
}

template <typename T>
int gram_run(const GramPlan& g, const void* jac, int R, int64_t P, int64_t ld, double* G, void* ws, hipStream_t st) {
    const bool direct = g.nsplit == 1;
    hipLaunchKernelGGL((ds::k_minsr_gram<T>), dim3((unsigned)g.tiles, (unsigned)g.nsplit), dim3(256), 0, st, (const T*)jac, R, (long)P, (size_t)ld,
                       g.pchunk, direct ? G : (double*)ws, direct ? 1 : 0);
    if (!direct)
        hipLaunchKernelGGL(ds::k_minsr_gram_sum, dim3((unsigned)(((size_t)R * R + 255) / 256)), dim3(256), 0, st, (const double*)ws, g.nsplit, R, G);
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename T>
int matvec_run(int mode, const void* jac, int R, int64_t P, int64_t ld, const double* v, double* out, hipStream_t st) {
    if (mode == 0)
        hipLaunchKernelGGL((ds::k_minsr_jv<T>), dim3((unsigned)R), dim3(256), 0, st, (const T*)jac, (long)P, (size_t)ld, v, (const double*)nullptr, 1.0,
                           out);
    else
        hipLaunchKernelGGL((ds::k_minsr_jtv<T>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (const T*)jac, R, (long)P, (size_t)ld, v, out);
    HIP_OK(hipGetLastError());
    return 0;
}

// workspace of the solve, in doubles: work copy W | M0, then the refined inverse | residual, then A again | pivot inverse |
// saved column panel | row means | block means | zeta0 | r
struct SolvePlan {
    int64_t o_w = 0, o_m = 0, o_r = 0, o_p = 0, o_c = 0, o_m1 = 0, o_mm = 0, o_z = 0, o_res = 0, doubles = 0;
    int nblk = 0;
};

int solve_plan(int64_t R, int64_t block, SolvePlan* sp) {
    if (R < 1 || R > 46340) return fail("ds_minsr_solve: R must lie in [1, 46340]");
    if (block < 0 || (block > 0 && R % block != 0)) return fail("ds_minsr_solve: R = %lld is not a multiple of block = %lld", (long long)R, (long long)block);
    auto r8 = [](int64_t v) { return (v + 7) / 8 * 8; };
    sp->nblk = block > 0 ? (int)(R / block) : 0;
    if (sp->nblk > 65535) return fail("ds_minsr_solve: more than 65535 blocks");
    sp->o_w = 0;
    sp->o_m = sp->o_w + r8(R * R);
    sp->o_r = sp->o_m + r8(R * R);
    sp->o_p = sp->o_r + r8(R * R);
    sp->o_c = sp->o_p + 1024;
    sp->o_m1 = sp->o_c + r8(R * 32);
    sp->o_mm = sp->o_m1 + r8(R * sp->nblk);
    sp->o_z = sp->o_mm + r8((int64_t)sp->nblk * sp->nblk);
    sp->o_res = sp->o_z + r8(R);
    sp->doubles = sp->o_res + r8(R);
    return 0;
}

int solve_run(const SolvePlan& sp, int R, int block, double scale, double lambda, const double* G, const double* rhs, double* zeta, void* ws,
              hipStream_t st) {
    double* base = (double*)ws;
    double *W = base + sp.o_w, *M0 = base + sp.o_m, *Rb = base + sp.o_r, *Pv = base + sp.o_p, *C = base + sp.o_c, *M1 = base + sp.o_m1,
           *MM = base + sp.o_mm, *z0 = base + sp.o_z, *res = base + sp.o_res;
    const unsigned ge = (unsigned)(((size_t)R * R + 255) / 256);
    if (block > 0) {
        hipLaunchKernelGGL(ds::k_minsr_rowmeans, dim3((unsigned)R, (unsigned)sp.nblk), dim3(256), 0, st, G, R, block, M1);
        hipLaunchKernelGGL(ds::k_minsr_blockmeans, dim3((unsigned)sp.nblk, (unsigned)sp.nblk), dim3(256), 0, st, (const double*)M1, R, block, MM);
    }
    hipLaunchKernelGGL(ds::k_minsr_prep, dim3(ge), dim3(256), 0, st, G, R, block, scale, lambda, (const double*)M1, (const double*)MM, W, M0);
    // the blocked Gauss-Jordan inverse and the Newton step of ds_kfac.h on one matrix of order R
    ds::KfacMats M;
    std::memset(&M, 0, sizeof(M));
    M.nb = 1; M.n[0] = R; M.rep[0] = 1;
    const int nbm = (R + 31) / 32;
    for (int k = 0; k < nbm; ++k) {
        hipLaunchKernelGGL(ds::k_kinv_diag, dim3(1), dim3(256), 0, st, M, (const double*)W, Pv, k);
        if (nbm > 1) hipLaunchKernelGGL(ds::k_kinv_panel, dim3((unsigned)((nbm + 3) / 4), 1), dim3(256), 0, st, M, W, (const double*)Pv, C, k);
        hipLaunchKernelGGL(ds::k_kinv_update, dim3((unsigned)((nbm * nbm + 3) / 4), 1), dim3(256), 0, st, M, W, (const double*)Pv, (const double*)C, k);
    }
    const dim3 gr((unsigned)((nbm * nbm + 3) / 4), 1);
    hipLaunchKernelGGL((ds::k_kinv_refine<1>), gr, dim3(256), 0, st, M, (const double*)M0, (const double*)W, Rb);
    hipLaunchKernelGGL((ds::k_kinv_refine<2>), gr, dim3(256), 0, st, M, (const double*)W, (const double*)Rb, M0);
    // X = M0.  zeta0 = X rhs, then one step of iterative refinement against A (formed again where the residual matrix was):
    // r = rhs - A zeta0,  zeta = zeta0 + X r
    hipLaunchKernelGGL(ds::k_minsr_prep, dim3(ge), dim3(256), 0, st, G, R, block, scale, lambda, (const double*)M1, (const double*)MM, Rb,
                       (double*)nullptr);
    const double* none = nullptr;
    hipLaunchKernelGGL((ds::k_minsr_jv<double>), dim3((unsigned)R), dim3(256), 0, st, (const double*)M0, (long)R, (size_t)R, rhs, none, 1.0, z0);
    hipLaunchKernelGGL((ds::k_minsr_jv<double>), dim3((unsigned)R), dim3(256), 0, st, (const double*)Rb, (long)R, (size_t)R, (const double*)z0, rhs, -1.0,
                       res);
    hipLaunchKernelGGL((ds::k_minsr_jv<double>), dim3((unsigned)R), dim3(256), 0, st, (const double*)M0, (long)R, (size_t)R, (const double*)res,
                       (const double*)z0, 1.0, zeta);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

int64_t ds_minsr_gram_workspace_bytes(int64_t R, int64_t P) {
    GramPlan g;
    if (gram_plan(R, P, &g)) return -1;
    return g.nsplit > 1 ? (int64_t)g.nsplit * R * R * 8 : 0;
}

int ds_minsr_gram(int dtype, const void* jac, int64_t R, int64_t P, int64_t ld, double* G, void* ws, int64_t ws_bytes, void* stream) {
    if (dtype != 0 && dtype != 1) return fail("ds_minsr_gram: dtype must be 0 (float64) or 1 (float32)");
    GramPlan g;
    if (int rc = gram_plan(R, P, &g)) return rc;
    if (!jac || !G) return fail("null argument");
    if (ld < P) return fail("ds_minsr_gram: ld = %lld is smaller than P = %lld", (long long)ld, (long long)P);
    const int64_t need = g.nsplit > 1 ? (int64_t)g.nsplit * R * R * 8 : 0;
    if (need > 0 && (!ws || ws_bytes < need)) return fail("ds_minsr_gram: workspace too small (ds_minsr_gram_workspace_bytes)");
    return DS_BY_DTYPE(dtype, gram_run, g, jac, (int)R, P, ld, G, ws, (hipStream_t)stream);
}

int64_t ds_minsr_matvec_workspace_bytes(int mode, int64_t R, int64_t P) {
    if ((mode != 0 && mode != 1) || R < 1 || P < 1) return -1;
    return 0;
}

int ds_minsr_matvec(int dtype, int mode, const void* jac, int64_t R, int64_t P, int64_t ld, const double* v, double* out, void* ws,
                    int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    if (dtype != 0 && dtype != 1) return fail("ds_minsr_matvec: dtype must be 0 (float64) or 1 (float32)");
    if (mode != 0 && mode != 1) return fail("ds_minsr_matvec: mode must be 0 (J v) or 1 (J^T v)");
    if (R < 1 || P < 1 || R > 2147483647LL) return fail("ds_minsr_matvec: R and P must be positive");
    if (!jac || !v || !out) return fail("null argument");
    if (ld < P) return fail("ds_minsr_matvec: ld = %lld is smaller than P = %lld", (long long)ld, (long long)P);
    return DS_BY_DTYPE(dtype, matvec_run, mode, jac, (int)R, P, ld, v, out, (hipStream_t)stream);
}

int64_t ds_minsr_solve_workspace_bytes(int64_t R, int64_t block) {
    SolvePlan sp;
    if (solve_plan(R, block, &sp)) return -1;
    return sp.doubles * 8;
}

int ds_minsr_solve(int64_t R, int64_t block, double scale, double lambda, const double* G, const double* rhs, double* zeta, void* ws,
                   int64_t ws_bytes, void* stream) {
    SolvePlan sp;
    if (int rc = solve_plan(R, block, &sp)) return rc;
    if (!(lambda > 0.0)) return fail("ds_minsr_solve: lambda must be positive");
    if (!G || !rhs || !zeta || !ws) return fail("null argument");
    if (ws_bytes < sp.doubles * 8) return fail("ds_minsr_solve: workspace too small (ds_minsr_solve_workspace_bytes)");
    return solve_run(sp, (int)R, (int)block, scale, lambda, G, rhs, zeta, ws, (hipStream_t)stream);
}

}  // extern "C"
