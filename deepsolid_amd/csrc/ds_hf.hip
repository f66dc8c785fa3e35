// ds_hf.hip -- host side of the Hartree-Fock orbital provider (ds_hf_create / ds_hf_destroy / ds_hf_orbitals / ds_hf_orbitals_at;
// kernels: ds_hf.h) and of the one-body density matrix in such a basis (ds_obdm_workspace_bytes / ds_obdm_accumulate; ds_obdm.h)
#include "ds_base.h"
#include "ds_hf.h"
#include "ds_obdm.h"

struct ds_hf {
    ds::HfArgs A;
    int nt;                                 // column tiles of 16 AOs the kernel is instantiated for: 1, 2, 4 or 8
    int n_kgroups;
    std::vector<void*> dev;                 // every device allocation, freed by ds_hf_destroy
};

namespace ds {
namespace host {

template <typename V>
int hf_upload(ds_hf* h, const std::vector<V>& host, const V** out) {
    void* d = nullptr;
    const size_t bytes = (host.empty() ? 1 : host.size()) * sizeof(V);
    HIP_OK(hipMalloc(&d, bytes));
    h->dev.push_back(d);
    if (!host.empty()) HIP_OK(hipMemcpy(d, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice));
    *out = (const V*)d;
    return 0;
}

template <typename T, int NT, int CH>
void hf_launch(const ds_hf* h, const void* x, long long np, void* up, void* dn, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_hf_orbitals<T, NT, CH>), dim3((unsigned)np, (unsigned)h->n_kgroups), dim3(64), 0, st, h->A, (const T*)x, np,
                       (double*)up, (double*)dn);
}

template <typename T>
void hf_dispatch(const ds_hf* h, const void* x, long long np, void* up, void* dn, hipStream_t st) {
    switch (h->nt) {
        case 1: hf_launch<T, 1, 64>(h, x, np, up, dn, st); break;
        case 2: hf_launch<T, 2, 64>(h, x, np, up, dn, st); break;
        case 4: hf_launch<T, 4, 64>(h, x, np, up, dn, st); break;
        default: hf_launch<T, 8, 32>(h, x, np, up, dn, st); break;      // 32-image chunks keep the LDS tile at 33 KB
    }
}

template <typename T, int NT, int CH>
void hf_at_launch(const ds_hf* h, const void* pts, long long np, int sp, void* out, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_hf_orbitals_at<T, NT, CH>), dim3((unsigned)np, (unsigned)h->n_kgroups), dim3(64), 0, st, h->A, (const T*)pts,
                       np, sp, (double*)out);
}

template <typename T>
void hf_at_dispatch(const ds_hf* h, const void* pts, long long np, int sp, void* out, hipStream_t st) {
    switch (h->nt) {
        case 1: hf_at_launch<T, 1, 64>(h, pts, np, sp, out, st); break;
        case 2: hf_at_launch<T, 2, 64>(h, pts, np, sp, out, st); break;
        case 4: hf_at_launch<T, 4, 64>(h, pts, np, sp, out, st); break;
        default: hf_at_launch<T, 8, 32>(h, pts, np, sp, out, st); break;
    }
}

// ------------------------------------------------------------------ one-body density matrix, ds_obdm.h
// Workspace of ds_obdm_accumulate for chunks of ng groups of OBDM_GROUP samples, in float64.  Shared by all chunks: the call's
// running sums (one partial row).  Per chunk: one partial row per group and the basis values at r_e and r' of every sample.
struct ObdmWs { double *ACC, *PART, *PHI; };
inline ObdmWs carve_obdm(Arena<double>& a, int Mb, int64_t ng) {
    const size_t row = (size_t)ds::obdm_row(Mb);
    ObdmWs w{};
    w.ACC = a.take(row);
    w.PART = a.take((size_t)ng * row);
    w.PHI = a.take((size_t)ng * ds::OBDM_GROUP * 2 * 2 * (size_t)Mb);
    return w;
}
inline int64_t obdm_bytes(int Mb, int64_t ng) {
    return (int64_t)measure([&](Arena<double>& a) { carve_obdm(a, Mb, ng); }) * 8;
}
constexpr int64_t OBDM_MAX_GROUPS = 1 << 22;             // 2 n blocks of k_obdm_basis stay below 2^31
constexpr int64_t OBDM_WS_BUDGET = 256LL << 20;          // what ds_obdm_workspace_bytes asks for at most (one group at least)

template <typename T, int NT, int CH>
void obdm_basis_launch(const ds_hf* h, const ds::ObdmArgs& O, const void* x, const void* shift, double* phi, hipStream_t st) {
    hipLaunchKernelGGL((ds::k_obdm_basis<T, NT, CH>), dim3((unsigned)(2 * O.n), (unsigned)h->n_kgroups), dim3(64), 0, st, h->A, O,
                       (const T*)x, (const T*)shift, phi);
}

template <typename T>
int obdm_impl(ds_hf* h, const void* x, int64_t B, int N, int n_up, int M, int first, const void* ratio, const void* shift,
              const double* weight, double* dm, double* ov, int64_t* n_bad, void* ws, int64_t ws_bytes, hipStream_t st) {
    const int M_up = h->A.n_up, M_dn = h->A.n_dn, Mb = std::max(M_up, M_dn);
    const int64_t total = B * (int64_t)M, groups_all = (total + ds::OBDM_GROUP - 1) / ds::OBDM_GROUP;
    // the chunk length follows from the workspace: the largest number of groups whose layout fits
    const int64_t fixed = obdm_bytes(Mb, 0), per = obdm_bytes(Mb, 1) - fixed;
    const int64_t ng = std::min<int64_t>({(ws_bytes - fixed) / per, OBDM_MAX_GROUPS, groups_all});
    if (!ws || ng < 1) return fail("workspace too small for ds_obdm_accumulate: %lld bytes < %lld for one group of %d samples",
                                   (long long)(ws ? ws_bytes : 0), (long long)obdm_bytes(Mb, 1), ds::OBDM_GROUP);
    Arena<double> a = arena_of<double>(ws, ws_bytes);
    const ObdmWs w = carve_obdm(a, Mb, ng);
    if (!a.ok) return carve_fail("one-body density matrix");
    ds::ObdmArgs O;
    O.M = M; O.N = N; O.n_up = n_up; O.first = first; O.Mb = Mb;
    const long long row = ds::obdm_row(Mb);
    const int64_t chunk = ng * ds::OBDM_GROUP;
    for (int64_t g0 = 0; g0 < total; g0 += chunk) {
        O.g0 = g0; O.n = std::min(chunk, total - g0);
        const int64_t groups = (O.n + ds::OBDM_GROUP - 1) / ds::OBDM_GROUP;
        switch (h->nt) {
            case 1: obdm_basis_launch<T, 1, 64>(h, O, x, shift, w.PHI, st); break;
            case 2: obdm_basis_launch<T, 2, 64>(h, O, x, shift, w.PHI, st); break;
            case 4: obdm_basis_launch<T, 4, 64>(h, O, x, shift, w.PHI, st); break;
            default: obdm_basis_launch<T, 8, 32>(h, O, x, shift, w.PHI, st); break;
        }
        hipLaunchKernelGGL((ds::k_obdm_accumulate<T>), dim3((unsigned)groups), dim3(64 * ds::OBDM_WAVES), 0, st, O, M_up, M_dn,
                           (const T*)ratio, weight, (const double*)w.PHI, w.PART);
        hipLaunchKernelGGL(ds::k_obdm_final, dim3((unsigned)((row + 255) / 256)), dim3(256), 0, st, (const double*)w.PART,
                           (long long)groups, Mb, M_up, M_dn, g0 == 0 ? 1 : 0, g0 + chunk >= total ? 1 : 0, w.ACC, dm, ov,
                           (long long*)n_bad);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace host
}  // namespace ds

using namespace ds::host;

extern "C" {

void ds_hf_destroy(ds_hf* h) {
    if (!h) return;
    for (void* d : h->dev) (void)hipFree(d);
    delete h;
}

int ds_hf_create(const ds_hf_desc* d, ds_hf** out) {
    if (!d || !out) return fail("null argument");
    *out = nullptr;
    if (!d->atoms || !d->shell_atom || !d->shell_l || !d->shell_nprim || !d->exps || !d->coefs || !d->kpts || !d->images ||
        !d->nocc_up || !d->nocc_dn)
        return fail("ds_hf_create: null array in the descriptor");
    if (d->n_atoms < 1) return fail("ds_hf_create: no atoms");
    if (d->n_shells < 1) return fail("ds_hf_create: no shells");
    if (d->n_k < 1 || d->n_k > ds::HF_MAX_K) return fail("ds_hf_create: n_k must be in 1..%d (got %d)", ds::HF_MAX_K, d->n_k);
    if (d->n_images < 1) return fail("ds_hf_create: no lattice images");
    if (d->n_up < 0 || d->n_dn < 0 || d->n_up > ds::HF_MAX_ORB || d->n_dn > ds::HF_MAX_ORB || d->n_up + d->n_dn < 1)
        return fail("ds_hf_create: electrons per spin must be in 0..%d, one at least (got %d, %d)", ds::HF_MAX_ORB, d->n_up, d->n_dn);
    if ((d->n_up > 0 && !d->mo_up) || (d->n_dn > 0 && !d->mo_dn)) return fail("ds_hf_create: null MO coefficients");
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(d->a[i])) return fail("ds_hf_create: lattice entry %d is not finite", i);
    const struct { const char* name; const double* v; long long n; } coords[] = {
        {"atoms", d->atoms, 3LL * d->n_atoms}, {"kpts", d->kpts, 3LL * d->n_k}, {"images", d->images, 3LL * d->n_images}};
    for (const auto& c : coords)
        for (long long i = 0; i < c.n; ++i)
            if (!std::isfinite(c.v[i])) return fail("ds_hf_create: %s[%lld][%lld] is not finite", c.name, i / 3, i % 3);

    std::vector<ds::HfShell> shells(d->n_shells);
    std::vector<double> exps, coefs;
    int nao = 0, np = 0;
    double amin = 1e300;
    for (int s = 0; s < d->n_shells; ++s) {
        const int at = d->shell_atom[s], l = d->shell_l[s], n = d->shell_nprim[s];
        if (at < 0 || at >= d->n_atoms) return fail("ds_hf_create: shell %d names atom %d of %d", s, at, d->n_atoms);
        if (l < 0 || l > 2) return fail("ds_hf_create: shell %d has l = %d; only s, p and d shells are provided", s, l);
        if (n < 1) return fail("ds_hf_create: shell %d has no primitives", s);
        for (int c = 0; c < 3; ++c) shells[s].R[c] = d->atoms[3 * at + c];
        shells[s].l = l;
        shells[s].nprim = n;
        shells[s].prim0 = np;
        shells[s].ao0 = nao;
        for (int j = 0; j < n; ++j) {
            const double al = d->exps[np + j], c = d->coefs[np + j];
            if (!(al > 0.0) || !std::isfinite(al) || !std::isfinite(c)) return fail("ds_hf_create: shell %d primitive %d is not a positive finite exponent with a finite coefficient", s, j);
            exps.push_back(al);
            coefs.push_back(c);
            amin = std::min(amin, al);
        }
        np += n;
        nao += 2 * l + 1;
    }
    if (nao > ds::HF_MAX_AO) return fail("ds_hf_create: %d atomic orbitals; at most %d are provided", nao, ds::HF_MAX_AO);

    ds_hf* h = new ds_hf();
    ds::HfArgs& A = h->A;
    for (int i = 0; i < 9; ++i) A.a[i] = d->a[i];
    inv3(d->a, A.ainv);
    A.n_up = d->n_up; A.n_dn = d->n_dn; A.n_k = d->n_k; A.nao = nao; A.n_shells = d->n_shells; A.n_atoms = d->n_atoms;
    A.alpha_min = amin;
    const int tiles = (nao + 15) / 16;
    h->nt = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 8;
    h->n_kgroups = (d->n_k + 7) / 8;
    const int nL = d->n_images, nLp = (nL + 63) / 64 * 64;
    A.n_img_pad = nLp;

    // occupation -> k point of every orbital (orbitals ordered by k, then band)
    std::vector<int> orbk[2];
    const int32_t* nocc[2] = {d->nocc_up, d->nocc_dn};
    const int ns[2] = {d->n_up, d->n_dn};
    for (int s = 0; s < 2; ++s) {
        for (int k = 0; k < d->n_k; ++k) {
            if (nocc[s][k] < 0) { ds_hf_destroy(h); return fail("ds_hf_create: negative occupation at k point %d", k); }
            for (int j = 0; j < nocc[s][k]; ++j) orbk[s].push_back(k);
        }
        if ((int)orbk[s].size() != ns[s]) {
            const int got = (int)orbk[s].size();
            ds_hf_destroy(h);
            return fail("ds_hf_create: spin %d has %d occupied orbitals over the k points but %d electrons", s, got, ns[s]);
        }
    }
    std::vector<double> images((size_t)nLp * 3, 0.0), phase((size_t)h->n_kgroups * nLp * 16, 0.0);
    for (int i = 0; i < 3 * nL; ++i) images[i] = d->images[i];
    for (int k = 0; k < d->n_k; ++k)
        for (int L = 0; L < nL; ++L) {
            const double ang = d->kpts[3 * k] * d->images[3 * L] + d->kpts[3 * k + 1] * d->images[3 * L + 1] + d->kpts[3 * k + 2] * d->images[3 * L + 2];
            double* row = &phase[((size_t)(k >> 3) * nLp + L) * 16 + 2 * (k & 7)];
            row[0] = std::cos(ang);
            row[1] = std::sin(ang);
        }
    std::vector<double> atoms(d->atoms, d->atoms + 3 * d->n_atoms), kpts(d->kpts, d->kpts + 3 * d->n_k);
    int rc = hf_upload(h, shells, &A.shells) || hf_upload(h, atoms, &A.atoms) || hf_upload(h, exps, &A.exps) ||
             hf_upload(h, coefs, &A.coefs) || hf_upload(h, kpts, &A.kpts) || hf_upload(h, images, &A.images) ||
             hf_upload(h, phase, &A.phase);
    const double* mo[2] = {d->mo_up, d->mo_dn};
    for (int s = 0; s < 2 && !rc; ++s) {
        std::vector<double> c(mo[s] ? (size_t)2 * nao * ns[s] : 0);
        for (size_t i = 0; i < c.size(); ++i) {
            if (!std::isfinite(mo[s][i])) { ds_hf_destroy(h); return fail("ds_hf_create: MO coefficient %zu of spin %d is not finite", i, s); }
            c[i] = mo[s][i];
        }
        rc = hf_upload(h, c, &A.mo[s]) || hf_upload(h, orbk[s], &A.orb_k[s]);
    }
    if (rc) { ds_hf_destroy(h); return 1; }
    *out = h;
    return 0;
}

int ds_hf_orbitals(ds_hf* h, int dtype, const void* x, int64_t B, void* out_up, void* out_dn, void* stream) {
    if (!h || !x) return fail("null argument");
    if (dtype != 0 && dtype != 1) return fail("dtype must be 0 or 1");
    if ((h->A.n_up > 0 && !out_up) || (h->A.n_dn > 0 && !out_dn)) return fail("ds_hf_orbitals: null output for a spin with electrons");
    if (B <= 0) return 0;
    const long long np = (long long)B * (h->A.n_up + h->A.n_dn);
    if (np > 2147483647LL) return fail("ds_hf_orbitals: %lld electron positions in one call; at most 2^31 - 1", np);
    hipStream_t st = (hipStream_t)stream;
    DS_BY_DTYPE(dtype, hf_dispatch, h, x, np, out_up, out_dn, st);
    HIP_OK(hipGetLastError());
    return 0;
}

int ds_hf_orbitals_at(ds_hf* h, int spin, int dtype, const void* points, int64_t P, void* out, void* stream) {
    if (!h) return fail("ds_hf_orbitals_at: null handle");
    if (spin != 0 && spin != 1) return fail("ds_hf_orbitals_at: spin must be 0 or 1 (got %d)", spin);
    if (dtype != 0 && dtype != 1) return fail("dtype must be 0 or 1");
    if (P < 0) return fail("ds_hf_orbitals_at: P must be >= 0 (got %lld)", (long long)P);
    if ((spin ? h->A.n_dn : h->A.n_up) == 0 || P == 0) return 0;
    if (!points || !out) return fail("ds_hf_orbitals_at: null points or output");
    if (P > 2147483647LL) return fail("ds_hf_orbitals_at: %lld points in one call; at most 2^31 - 1", (long long)P);
    hipStream_t st = (hipStream_t)stream;
    DS_BY_DTYPE(dtype, hf_at_dispatch, h, points, (long long)P, spin, out, st);
    HIP_OK(hipGetLastError());
    return 0;
}

int64_t ds_obdm_workspace_bytes(const ds_hf* h, int64_t B, int n_samples) {
    if (!h || B < 1 || n_samples < 1) return -1;
    const int Mb = std::max(h->A.n_up, h->A.n_dn);
    const int64_t groups = (B * (int64_t)n_samples + ds::OBDM_GROUP - 1) / ds::OBDM_GROUP;
    const int64_t fixed = obdm_bytes(Mb, 0), per = obdm_bytes(Mb, 1) - fixed;
    return obdm_bytes(Mb, std::min<int64_t>({groups, OBDM_MAX_GROUPS, std::max<int64_t>(1, (OBDM_WS_BUDGET - fixed) / per)}));
}

int ds_obdm_accumulate(ds_hf* h, int dtype, const void* x, int64_t B, int n_elec, int n_up, int n_samples, int first_electron,
                       const void* ratio, const void* shift, const double* weight, double* dm_sums, double* ov_sums, int64_t* n_bad,
                       void* ws, int64_t ws_bytes, void* stream) {
    if (!h || !x || !ratio || !shift) return fail("ds_obdm_accumulate: null basis, x, ratio or shift");
    if (!dm_sums && !ov_sums) return fail("ds_obdm_accumulate: dm_sums and ov_sums are both null, nothing to write");
    if (dtype != 0 && dtype != 1) return fail("ds_obdm_accumulate: dtype must be 0 or 1 (got %d)", dtype);
    if (B < 1) return fail("ds_obdm_accumulate: B must be >= 1 (got %lld)", (long long)B);
    if (n_samples < 1) return fail("ds_obdm_accumulate: n_samples must be >= 1 (got %d)", n_samples);
    if (n_elec < 1) return fail("ds_obdm_accumulate: n_elec must be >= 1 (got %d)", n_elec);
    if (n_up < 0 || n_up > n_elec) return fail("ds_obdm_accumulate: n_up must be in 0..%d (got %d)", n_elec, n_up);
    if (first_electron < 0 || first_electron >= n_elec)
        return fail("ds_obdm_accumulate: first_electron must be in 0..%d (got %d)", n_elec - 1, first_electron);
    if (B > 2147483647LL / n_samples)
        return fail("ds_obdm_accumulate: %lld x %d samples in one call; at most 2^31 - 1", (long long)B, n_samples);
    return DS_BY_DTYPE(dtype, obdm_impl, h, x, B, n_elec, n_up, n_samples, first_electron, ratio, shift, weight, dm_sums, ov_sums, n_bad,
                       ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
