// ds_observe.hip -- observables of a batch of walkers that need no wave function (ds_obs.h, ds_realspace.h): structure factor and
// polarization sums, electron density and pair-correlation counts; and forward walking for the DMC (ds_fw.h): ancestor tables, the
// counts with a weight and a source row per walker, weighted sums of per-walker values; and the ionic forces (ds_force.h), which need
// the handle's Ewald tables and the caller's drift but no forward of their own; and the strain derivative of the energy (ds_stress.h),
// which needs the same tables and the caller's walker gradient.
#include "ds_host.h"
#include "ds_obs.h"
#include "ds_realspace.h"
#include "ds_fw.h"
#include "ds_force.h"
#include "ds_stress.h"

namespace ds {
namespace host {

// observables (ds_obs.h): one kernel instance per number of q points per lane
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


template <typename T>
void realspace_counts(const ds::RealSpaceArgs& A, const void* x, size_t off, long long nb, int N, int64_t* dens, int64_t* pair, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_realspace_counts<T>), dim3((unsigned)ds::rs_groups(nb)), dim3(ds::RS_THREADS), 0, st, A, (const T*)x + off, nb, N,
                       (unsigned long long*)dens, (unsigned long long*)pair);
}

// what ds_realspace_counts and ds_realspace_counts_w check alike, and the kernel arguments they share
static int realspace_args(const char* who, const double* fold_inv, const int32_t* grid, const double* latvec, const double* latvec_inv,
                          double r_max, int n_r, int dtype, const void* x, int64_t B, int64_t n_elec, int64_t n_up, const int64_t* dens,
                          const int64_t* pair, ds::RealSpaceArgs& A) {
    if (!x) return fail("null argument");
    if (!dens && !pair) return fail("%s: dens and pair are both null, nothing to count", who);
    if (dtype != 0 && dtype != 1) return fail("dtype must be 0 or 1");
    if (B < 1) return fail("B must be >= 1 (got %lld)", (long long)B);
    if (n_elec < 1 || n_elec > ds::RS_MAX_N) return fail("n_elec must be in 1..%d (got %lld)", ds::RS_MAX_N, (long long)n_elec);
    if (n_up < 0 || n_up > n_elec) return fail("n_up must be in 0..n_elec = %lld (got %lld)", (long long)n_elec, (long long)n_up);
    std::memset(&A, 0, sizeof(A));
    A.n_up = (int)n_up;
    A.do_dens = dens != nullptr;
    A.do_pair = pair != nullptr;
    if (dens) {
        if (!fold_inv || !grid) return fail("%s: the density needs fold_inv and grid", who);
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
        if (!latvec || !latvec_inv) return fail("%s: the pair counts need latvec and latvec_inv", who);
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
    return 0;
}

template <typename T>
void realspace_counts_w(const ds::RealSpaceArgs& A, const void* x, long long nb, int N, long long B_src, const int32_t* index,
                        const double* weight, double scale, int64_t* dens, int64_t* pair, int64_t* q_sum, int64_t* n_bad, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_realspace_counts_w<T>), dim3((unsigned)ds::rs_groups(nb)), dim3(ds::RS_THREADS), 0, st, A, (const T*)x, nb, N,
                       B_src, (const int*)index, weight, scale, (unsigned long long*)dens, (unsigned long long*)pair, (unsigned long long*)q_sum,
                       (unsigned long long*)n_bad);
}

// the smallest distance between neighbouring lattice planes (estimator.plane_spacings)
static double min_plane_spacing(const double* a) {
    double inv[9], best = INFINITY;
    inv3(a, inv);
    for (int j = 0; j < 3; ++j) best = std::min(best, 1.0 / std::sqrt(inv[j] * inv[j] + inv[3 + j] * inv[3 + j] + inv[6 + j] * inv[6 + j]));
    return best;
}

// ionic forces (ds_force.h): the walkers [b0, b0 + nb) of the batch; rows: of this launch
template <typename T>
void ion_forces(ds_system* s, const void* x, const void* drift, int64_t b0, int64_t nb, double r_c, const double* ion_ion, double* out_hf,
                double* out_zv, double* rows, int64_t* n_bad, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int tables = ds::force_table_flags(S);      // (>= 0: checked by ds_ion_forces)
    const size_t n3 = 3 * (size_t)S.N, a3 = 3 * (size_t)S.As;
    hipLaunchKernelGGL((ds::k_ion_forces<T>), dim3((unsigned)nb), dim3(256), ds::force_lds_doubles(S, tables) * sizeof(double), st, S,
                       (const T*)x + b0 * n3, drift ? (const T*)drift + b0 * n3 : nullptr, r_c, 0.5 * min_plane_spacing(s->d.sim_a), ion_ion, tables,
                       out_hf ? out_hf + b0 * a3 : nullptr, out_zv ? out_zv + b0 * a3 : nullptr, rows, (unsigned long long*)n_bad);
}

// half the length of the shortest non-zero lattice vector with coefficients in -3..3 (estimator.wigner_seitz_radius)
static double wigner_seitz_radius(const double* a) {
    double best = INFINITY;
    for (int i = -3; i <= 3; ++i)
        for (int j = -3; j <= 3; ++j)
            for (int k = -3; k <= 3; ++k) {
                if (!i && !j && !k) continue;
                double v2 = 0;
                for (int c = 0; c < 3; ++c) {
                    const double v = i * a[c] + j * a[3 + c] + k * a[6 + c];
                    v2 += v * v;
                }
                best = std::min(best, v2);
            }
    return 0.5 * std::sqrt(best);
}

template <typename T> int force_tables(ds_system* s) { return ds::force_table_flags(dev<T>(s)); }

// doubles of workspace per group of FORCE_GROUP walkers: their rows and the group's partial sums
static int64_t force_group_doubles(const ds_system* s) { return (int64_t)ds::FORCE_GROUP * 6 * s->sd.As + 12 * s->sd.As + 1; }

static_assert(FORCE_SUM_GROUP == ds::FORCE_GROUP, "ds_host.h restates the group of k_force_part");
int force_sums(const double* rows, int64_t nw, int A, double* part, double* sums, hipStream_t st) {
    const int64_t groups = (nw + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP;
    const int K = 12 * A + 1;
    hipLaunchKernelGGL(ds::k_force_part, dim3((unsigned)groups), dim3(ds::FORCE_GROUP), 0, st, rows, (long long)nw, A, part);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(ds::k_force_final, dim3((K + 255) / 256), dim3(256), 0, st, (const double*)part, (long long)groups, K, sums);
    HIP_OK(hipGetLastError());
    return 0;
}

// strain derivatives (ds_stress.h): the walkers [b0, b0 + nb) of the batch; rows: of this launch
template <typename T>
void stress(ds_system* s, const void* x, const void* grad, int64_t b0, int64_t nb, const double* ion_ion, double* out, double* rows,
            int64_t* n_bad, hipStream_t st) {
    const ds::SysDev<T>& S = dev<T>(s);
    const int tables = ds::stress_table_flags(S);     // (>= 0: checked by ds_stress)
    const size_t n3 = 3 * (size_t)S.N;
    hipLaunchKernelGGL((ds::k_stress<T>), dim3((unsigned)nb), dim3(256), ds::stress_lds_doubles(S, tables != 0) * sizeof(double), st, S,
                       (const T*)x + b0 * n3, grad ? (const T*)grad + b0 * 2 * n3 : nullptr, ion_ion, tables,
                       out ? out + b0 * 6 * ds::STRESS_ROWS : nullptr, rows, (unsigned long long*)n_bad);
}

template <typename T> int stress_tables(ds_system* s) { return ds::stress_table_flags(dev<T>(s)); }

// doubles of workspace per group of FORCE_GROUP walkers: their rows and the group's partial sums
static int64_t stress_group_doubles() { return (int64_t)ds::FORCE_GROUP * 6 * ds::STRESS_ROWS + ds::STRESS_K; }

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

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
    DS_BY_DTYPE(dtype, obs_partial, A, x, B, (int)n_elec, G, part, st);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(ds::k_obs_final, dim3((K + 255) / 256), dim3(256), 0, st, (const double*)part, G, K, out_sums);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_realspace_counts(const double* fold_inv, const int32_t* grid, const double* latvec, const double* latvec_inv, double r_max,
                        int n_r, int dtype, const void* x, int64_t B, int64_t n_elec, int64_t n_up, int64_t* dens, int64_t* pair,
                        void* stream) {
    ds::RealSpaceArgs A;
    if (int rc = realspace_args("ds_realspace_counts", fold_inv, grid, latvec, latvec_inv, r_max, n_r, dtype, x, B, n_elec, n_up, dens, pair, A))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // pieces of at most RS_MAX_LAUNCH_WALKERS walkers: the bound behind the uint32 LDS bins (ds_realspace.h)
    for (int64_t b0 = 0; b0 < B; b0 += ds::RS_MAX_LAUNCH_WALKERS) {
        const long long nb = (long long)std::min<int64_t>(B - b0, ds::RS_MAX_LAUNCH_WALKERS);
        const size_t off = (size_t)b0 * 3 * (size_t)n_elec;
        DS_BY_DTYPE(dtype, realspace_counts, A, x, off, nb, (int)n_elec, dens, pair, st);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int ds_realspace_counts_w(const double* fold_inv, const int32_t* grid, const double* latvec, const double* latvec_inv, double r_max,
                          int n_r, int dtype, const void* x, int64_t B, int64_t n_elec, int64_t n_up, int64_t* dens, int64_t* pair,
                          int64_t B_src, const int32_t* index, const double* weight, double weight_scale, int64_t* q_sum,
                          int64_t* n_bad, void* stream) {
    ds::RealSpaceArgs A;
    if (int rc = realspace_args("ds_realspace_counts_w", fold_inv, grid, latvec, latvec_inv, r_max, n_r, dtype, x, B, n_elec, n_up, dens, pair, A))
        return rc;
    if (!q_sum || !n_bad) return fail("ds_realspace_counts_w: null q_sum or n_bad");
    if (B_src < 1 || B_src > INT32_MAX) return fail("ds_realspace_counts_w: B_src must be in 1..2^31 - 1 (got %lld)", (long long)B_src);
    if (!index && B > B_src) return fail("ds_realspace_counts_w: without an index B = %lld walkers need B_src >= B (got %lld)", (long long)B, (long long)B_src);
    if (weight && !(weight_scale > 0.0 && std::isfinite(weight_scale)))
        return fail("ds_realspace_counts_w: weight_scale must be positive and finite (got %g)", weight_scale);
    hipStream_t st = (hipStream_t)stream;
    // pieces of at most RS_MAX_LAUNCH_WALKERS walkers: the bound behind the LDS bins (ds_fw.h); the source rows are those of all of x.
    // Without an index walker w reads row w: the piece's rows then start at its own first walker.
    for (int64_t b0 = 0; b0 < B; b0 += ds::RS_MAX_LAUNCH_WALKERS) {
        const long long nb = (long long)std::min<int64_t>(B - b0, ds::RS_MAX_LAUNCH_WALKERS);
        const size_t off = index ? 0 : (size_t)b0 * 3 * (size_t)n_elec;
        const void* xp = dtype == 0 ? (const void*)((const double*)x + off) : (const void*)((const float*)x + off);
        DS_BY_DTYPE(dtype, realspace_counts_w, A, xp, nb, (int)n_elec, (long long)(index ? B_src : B_src - b0), index ? index + b0 : nullptr,
                    weight ? weight + b0 : nullptr, weight_scale, dens, pair, q_sum, n_bad, st);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int64_t ds_dmc_ancestry_workspace_bytes(int64_t B, int n_slots) {
    if (B < 1 || B > INT32_MAX || n_slots < 0) return -1;
    return (int64_t)sizeof(int32_t) * B * (1 + (int64_t)n_slots);
}

int ds_dmc_ancestry(int64_t B, int steps, const int32_t* parents, int n_slots, int32_t* anc, int32_t* out_block, void* ws, int64_t ws_bytes,
                    void* stream) {
    if (B < 1 || B > INT32_MAX) return fail("ds_dmc_ancestry: B must be in 1..2^31 - 1 (got %lld)", (long long)B);
    if (steps < 0 || n_slots < 0) return fail("ds_dmc_ancestry: steps and n_slots must be >= 0 (got %d, %d)", steps, n_slots);
    if (steps > 0 && !parents) return fail("ds_dmc_ancestry: null parents with steps = %d", steps);
    if (n_slots > 0 && !anc) return fail("ds_dmc_ancestry: null anc with n_slots = %d", n_slots);
    if (!ws) return fail("ds_dmc_ancestry: null workspace");
    const int64_t need = ds_dmc_ancestry_workspace_bytes(B, n_slots);
    if (ws_bytes < need)
        return fail("workspace too small for ds_dmc_ancestry: %lld bytes < %lld (see ds_dmc_ancestry_workspace_bytes)", (long long)ws_bytes,
                    (long long)need);
    hipStream_t st = (hipStream_t)stream;
    int* P = (int*)ws;
    int* old = P + B;
    const unsigned groups = (unsigned)((B + 255) / 256);
    hipLaunchKernelGGL(ds::k_fw_compose, dim3(groups), dim3(256), 0, st, (long long)B, steps, (const int*)parents, P);
    HIP_OK(hipGetLastError());
    if (n_slots > 0) {
        HIP_OK(hipMemcpyAsync(old, anc, sizeof(int32_t) * (size_t)B * (size_t)n_slots, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(ds::k_fw_apply, dim3(groups), dim3(256), 0, st, (long long)B, n_slots, (const int*)P, (const int*)old, (int*)anc);
        HIP_OK(hipGetLastError());
    }
    if (out_block) HIP_OK(hipMemcpyAsync(out_block, P, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToDevice, st));
    return 0;
}

int64_t ds_dmc_fw_sums_workspace_bytes(int64_t B, int K) {
    if (B < 1 || B > INT32_MAX || K < 1 || K > ds::FW_MAX_K) return -1;
    return (int64_t)sizeof(double) * 2 * K * ((B + ds::FW_GROUP - 1) / ds::FW_GROUP);
}

int ds_dmc_fw_sums(int64_t B, int K, const double* values, int64_t B_src, const int32_t* index, const double* weight, double* out,
                   int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream) {
    if (!values || !out || !n_bad || !ws) return fail("ds_dmc_fw_sums: null argument");
    if (B < 1 || B > INT32_MAX) return fail("ds_dmc_fw_sums: B must be in 1..2^31 - 1 (got %lld)", (long long)B);
    if (K < 1 || K > ds::FW_MAX_K) return fail("ds_dmc_fw_sums: K must be in 1..%d (got %d)", ds::FW_MAX_K, K);
    if (B_src < 1 || B_src > INT32_MAX) return fail("ds_dmc_fw_sums: B_src must be in 1..2^31 - 1 (got %lld)", (long long)B_src);
    if (!index && B > B_src) return fail("ds_dmc_fw_sums: without an index B = %lld walkers need B_src >= B (got %lld)", (long long)B, (long long)B_src);
    const int64_t need = ds_dmc_fw_sums_workspace_bytes(B, K);
    if (ws_bytes < need)
        return fail("workspace too small for ds_dmc_fw_sums: %lld bytes < %lld (see ds_dmc_fw_sums_workspace_bytes)", (long long)ws_bytes,
                    (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const long long groups = (B + ds::FW_GROUP - 1) / ds::FW_GROUP;
    hipLaunchKernelGGL(ds::k_fw_sums, dim3((unsigned)groups), dim3(ds::FW_GROUP), 0, st, (long long)B, K, values, (long long)B_src,
                       (const int*)index, weight, (double*)ws, (unsigned long long*)n_bad);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(ds::k_fw_sums_final, dim3(1), dim3(2 * ds::FW_MAX_K), 0, st, (const double*)ws, groups, K, out);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t ds_ion_forces_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s || B < 1) return -1;
    const int64_t per = force_group_doubles(s) * (int64_t)sizeof(double);
    const int64_t groups = (B + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP;
    return per * std::max<int64_t>(1, std::min<int64_t>(groups, workspace_budget() / per));
}

int ds_ion_forces(ds_system* s, const void* x, const void* drift, int64_t B, double r_c, const double* ion_ion, double* out_hf,
                  double* out_zv, double* sums, int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream) {
    if (!s || !x) return fail("ds_ion_forces: null argument");
    if (B < 1) return fail("ds_ion_forces: B must be >= 1 (got %lld)", (long long)B);
    if (!out_hf && !out_zv && !sums) return fail("ds_ion_forces: out_hf, out_zv and sums are all null, nothing to write");
    if ((out_zv || sums) && !drift) return fail("ds_ion_forces: out_zv and sums need the drift (got a null drift)");
    const double r_ws = wigner_seitz_radius(s->d.sim_a);
    if (!(r_c > 0.0) || !std::isfinite(r_c) || r_c > r_ws * (1.0 + 1e-12))
        return fail("ds_ion_forces: the cutoff r_c = %g must be positive and at most the Wigner-Seitz radius %.17g of the simulation cell", r_c, r_ws);
    // the nearest image of the zero-variance term is looked for one cell around the wrapped one (ds_force.h)
    if ((out_zv || sums) && !(r_c < min_plane_spacing(s->d.sim_a)))
        return fail("ds_ion_forces: the cutoff r_c = %g is not below the smallest plane spacing %g of the simulation cell: the lattice "
                    "vectors are too skewed for the nearest-image search (use a reduced cell or a smaller cutoff)", r_c, min_plane_spacing(s->d.sim_a));
    if (DS_BY_DTYPE(s->dtype, force_tables, s) < 0)
        return fail("ds_ion_forces: %d ions need more than %d KB of LDS per walker: not supported", s->sd.As, (int)(ds::FORCE_LDS_MAX / 1024));
    const int A = s->sd.As;
    const int64_t per = force_group_doubles(s) * (int64_t)sizeof(double);
    int64_t fit = 0;
    if (sums) {
        fit = ws ? ws_bytes / per : 0;
        if (fit < 1)
            return fail("workspace too small for ds_ion_forces: %lld bytes < %lld for one group of %d walkers (see ds_ion_forces_workspace_bytes)",
                        (long long)(ws ? ws_bytes : 0), (long long)per, ds::FORCE_GROUP);
    }
    hipStream_t st = (hipStream_t)stream;
    if (!sums) {
        DS_BY_DTYPE(s->dtype, ion_forces, s, x, drift, (int64_t)0, B, r_c, ion_ion, out_hf, out_zv, (double*)nullptr, n_bad, st);
        HIP_OK(hipGetLastError());
        return 0;
    }
    // passes of `fit` groups: a pass starts at a multiple of FORCE_GROUP walkers of the batch, so the groups -- and with them the
    // order of every addition -- are those of one pass over everything
    const int K = 12 * A + 1;
    fit = std::min<int64_t>(fit, (B + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP);
    double* rows = (double*)ws;
    double* part = rows + (size_t)fit * ds::FORCE_GROUP * 6 * A;
    for (int64_t b0 = 0; b0 < B; b0 += fit * ds::FORCE_GROUP) {
        const int64_t nb = std::min<int64_t>(B - b0, fit * ds::FORCE_GROUP);
        const int64_t groups = (nb + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP;
        DS_BY_DTYPE(s->dtype, ion_forces, s, x, drift, b0, nb, r_c, ion_ion, out_hf, out_zv, rows, n_bad, st);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(ds::k_force_part, dim3((unsigned)groups), dim3(ds::FORCE_GROUP), 0, st, (const double*)rows, (long long)nb, A, part);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(ds::k_force_final, dim3((K + 255) / 256), dim3(256), 0, st, (const double*)part, (long long)groups, K, sums);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int64_t ds_stress_workspace_bytes(const ds_system* s, int64_t B) {
    if (!s || B < 1) return -1;
    const int64_t per = stress_group_doubles() * (int64_t)sizeof(double);
    const int64_t groups = (B + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP;
    return per * std::max<int64_t>(1, std::min<int64_t>(groups, workspace_budget() / per));
}

int ds_stress(ds_system* s, const void* x, const void* grad, int64_t B, const double* ion_ion, double* out, double* sums, int64_t* n_bad,
              void* ws, int64_t ws_bytes, void* stream) {
    if (!s || !x) return fail("ds_stress: null argument");
    if (B < 1) return fail("ds_stress: B must be >= 1 (got %lld)", (long long)B);
    if (!out && !sums) return fail("ds_stress: out and sums are both null, nothing to write");
    if (sums && !grad) return fail("ds_stress: sums hold the kinetic rows too: they need the gradient (got a null grad)");
    if (DS_BY_DTYPE(s->dtype, stress_tables, s) < 0)
        return fail("ds_stress: %d electrons need more than %d KB of LDS per walker: not supported", s->sd.N, (int)(ds::FORCE_LDS_MAX / 1024));
    const int64_t per = stress_group_doubles() * (int64_t)sizeof(double);
    int64_t fit = 0;
    if (sums) {
        fit = ws ? ws_bytes / per : 0;
        if (fit < 1)
            return fail("workspace too small for ds_stress: %lld bytes < %lld for one group of %d walkers (see ds_stress_workspace_bytes)",
                        (long long)(ws ? ws_bytes : 0), (long long)per, ds::FORCE_GROUP);
    }
    hipStream_t st = (hipStream_t)stream;
    if (!sums) {
        DS_BY_DTYPE(s->dtype, stress, s, x, grad, (int64_t)0, B, ion_ion, out, (double*)nullptr, n_bad, st);
        HIP_OK(hipGetLastError());
        return 0;
    }
    // passes of `fit` groups, cut at multiples of FORCE_GROUP walkers of the batch as in ds_ion_forces: the same additions in the
    // same order for any workspace
    fit = std::min<int64_t>(fit, (B + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP);
    double* rows = (double*)ws;
    double* part = rows + (size_t)fit * ds::FORCE_GROUP * 6 * ds::STRESS_ROWS;
    for (int64_t b0 = 0; b0 < B; b0 += fit * ds::FORCE_GROUP) {
        const int64_t nb = std::min<int64_t>(B - b0, fit * ds::FORCE_GROUP);
        const int64_t groups = (nb + ds::FORCE_GROUP - 1) / ds::FORCE_GROUP;
        DS_BY_DTYPE(s->dtype, stress, s, x, grad, b0, nb, ion_ion, out, rows, n_bad, st);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(ds::k_stress_part, dim3((unsigned)groups), dim3(ds::FORCE_GROUP), 0, st, (const double*)rows, (long long)nb, part);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(ds::k_force_final, dim3((ds::STRESS_K + 255) / 256), dim3(256), 0, st, (const double*)part, (long long)groups,
                           ds::STRESS_K, sums);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
