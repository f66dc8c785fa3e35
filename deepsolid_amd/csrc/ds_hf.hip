// ds_hf.hip -- host side of the Hartree-Fock orbital provider (ds_hf_create / ds_hf_destroy / ds_hf_orbitals); kernel: ds_hf.h
#include "ds_base.h"
#include "ds_hf.h"

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

}  // extern "C"
