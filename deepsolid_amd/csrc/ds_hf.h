// ds_hf.h -- Hartree-Fock crystalline orbitals of a Gaussian basis at a batch of walkers or at arbitrary points.
//
// Reference: DeepSolid/hf.py:106-153 (`eval_orbitals_pbc`, `eval_mos_pbc`, `eval_orb_mat`), which calls PySCF's
// `PBCGTOval_sph` on the host.  Conventions:
//   ao_k,mu(r) = sum_L exp(i k.L) R_mu(|d|) S_lm(d),   d = r - R_atom(mu) - L,   R(|d|) = sum_p c_p exp(-alpha_p |d|^2)
//   S_lm: real solid harmonics orthonormal on the sphere; l = 1 in the order x, y, z; l = 2 in the order xy, yz, z^2, xz, x^2-y^2
//   the walker is wrapped into the primitive cell first and the AO is multiplied by exp(i k.(wrap a))        (hf.py:113-120)
//   orbital o of spin s belongs to one k point (orbitals ordered by k, then band); out[b][e][o] = sum_mu ao_k(o),mu(r_be) C[mu][o]
//
// One wave (one workgroup of 64 lanes) per (electron, group of 8 k points):
//   1. wrap the position (float64; a float32 walker is widened on load);
//   2. per chunk of CH images: lane = image; every shell's radial sum and its 1, 3 or 5 angular factors go to the LDS tile
//      chi[image][mu]; a chunk is skipped when alpha_min |r - R - L|^2 > 90 for every lane and every atom (terms below e^-90);
//   3. AO[(k, re/im)][mu] += phase[(k, re/im)][L] chi[L][mu] on v_mfma_f64_16x16x4_f64: 16 rows = 8 k points x (re, im),
//      NT column tiles of 16 AOs, 4 images per instruction, images in table order;
//   4. the 16 x nao AO tile goes back to LDS; lane o contracts it with the MO coefficients of orbital o over mu in index order,
//      applies the wrap phase and stores one complex128.
// No atomics, no cross-wave reduction: the bits of one electron's row depend on its position alone.
// Steps 1-4 are the device function hf_orbital_row; k_hf_orbitals (the electrons of a batch of walkers: the spin follows from the
// electron index), k_hf_orbitals_at (arbitrary points, the spin is an argument) and k_obdm_basis (ds_obdm.h) only say where the
// point comes from and where the row goes.
// Beyond 8 k points every k group is a workgroup of its own that evaluates the chi tiles again: the exponentials, which bound the
// kernel at n_k = 8 (EXPERIMENTS.md), are paid ceil(n_k / 8) times per electron.
#pragma once
#include <hip/hip_runtime.h>

#include "ds_device.h"

namespace ds {

constexpr int HF_MAX_AO = 128;
constexpr int HF_MAX_K = 64;
constexpr int HF_MAX_ORB = 64;         // electrons (= orbitals) per spin
constexpr double HF_SCREEN = 90.0;

struct HfShell {
    double R[3];                       // centre
    int l, nprim, prim0, ao0;          // angular momentum, primitives [prim0, prim0 + nprim), first AO column
};

struct HfArgs {
    double a[9], ainv[9];              // primitive cell (rows = lattice vectors) and its inverse
    int n_up, n_dn, n_k, nao, n_shells, n_atoms, n_img_pad;
    double alpha_min;
    const HfShell* shells;
    const double* atoms;               // (n_atoms, 3)
    const double* exps;                // concatenated primitives
    const double* coefs;
    const double* kpts;                // (n_k, 3)
    const double* images;              // (n_img_pad, 3), padded rows are zero vectors with phase 0
    const double* phase;               // [k group][image][16]: row 2 kl = cos(k.L), row 2 kl + 1 = sin(k.L)
    const double* mo[2];               // per spin [mu][o] interleaved (re, im)
    const int* orb_k[2];               // per spin: k point of orbital o
};

// S_lm factors (orthonormal on the sphere)
constexpr double HF_S0 = 0.28209479177387814;      // 1 / (2 sqrt(pi))
constexpr double HF_S1 = 0.48860251190291992;      // sqrt(3 / 4 pi)
constexpr double HF_D_XY = 1.0925484305920792;     // sqrt(15 / 4 pi)
constexpr double HF_D_Z2 = 0.31539156525252005;    // sqrt(5 / 16 pi)
constexpr double HF_D_X2Y2 = 0.54627421529603959;  // sqrt(15 / 16 pi)

// The orbitals of spin `sp` at ONE point r (float64), by one wave: steps 1-4 of the head of the file for the k group `kg`.  Lane o
// (o < orbitals of the spin, k point of o in the group) stores orbital o at row[2 o], row[2 o + 1].  Every kernel that evaluates
// orbitals goes through this function, so a point's bits depend on (r, sp) alone, whichever kernel asks.
template <int NT, int CH>
__device__ __forceinline__ void hf_orbital_row(const HfArgs& A, const double r[3], int sp, int kg, double* __restrict__ row_out) {
    constexpr int LD = 16 * NT + 1;
    __shared__ double chi[CH * LD];
    const int lane = threadIdx.x;

    // 1. wrap into the primitive cell
    double rp[3], wr[3];
    wrap_point<double>(r, A.a, A.ainv, rp, wr);

    typedef Acc4<double>::type acc_t;
    acc_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = acc_t{0, 0, 0, 0};
    for (int i = lane; i < CH * LD; i += 64) chi[i] = 0.0;
    __syncthreads();

    const double* ph = A.phase + (long long)kg * A.n_img_pad * 16;
    for (int L0 = 0; L0 < A.n_img_pad; L0 += CH) {
        // 2. this lane's image
        const bool active = lane < CH;
        const int li = L0 + (active ? lane : 0);
        const double q0 = rp[0] - A.images[3 * li], q1 = rp[1] - A.images[3 * li + 1], q2 = rp[2] - A.images[3 * li + 2];
        double dmin = 1e300;
        for (int at = 0; at < A.n_atoms; ++at) {
            const double d0 = q0 - A.atoms[3 * at], d1 = q1 - A.atoms[3 * at + 1], d2 = q2 - A.atoms[3 * at + 2];
            const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
            dmin = r2 < dmin ? r2 : dmin;
        }
        if (__all(!active || A.alpha_min * dmin > HF_SCREEN)) continue;    // wave-uniform: every image of the chunk is below e^-90
        if (active) {
            double* row = chi + lane * LD;
            for (int s = 0; s < A.n_shells; ++s) {
                const HfShell sh = A.shells[s];
                const double d0 = q0 - sh.R[0], d1 = q1 - sh.R[1], d2 = q2 - sh.R[2];
                const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                double rad = 0.0;
                for (int j = 0; j < sh.nprim; ++j) rad += A.coefs[sh.prim0 + j] * exp(-A.exps[sh.prim0 + j] * r2);
                if (sh.l == 0) {
                    row[sh.ao0] = HF_S0 * rad;
                } else if (sh.l == 1) {
                    const double f = HF_S1 * rad;
                    row[sh.ao0] = f * d0;
                    row[sh.ao0 + 1] = f * d1;
                    row[sh.ao0 + 2] = f * d2;
                } else {
                    row[sh.ao0] = HF_D_XY * rad * (d0 * d1);
                    row[sh.ao0 + 1] = HF_D_XY * rad * (d1 * d2);
                    row[sh.ao0 + 2] = HF_D_Z2 * rad * (3.0 * d2 * d2 - r2);
                    row[sh.ao0 + 3] = HF_D_XY * rad * (d0 * d2);
                    row[sh.ao0 + 4] = HF_D_X2Y2 * rad * (d0 * d0 - d1 * d1);
                }
            }
        }
        __syncthreads();
        // 3. AO tile += phase (16 x CH) . chi (CH x 16 NT), four images per instruction
        const int kk = lane >> 4, col = lane & 15;
#pragma unroll 4
        for (int j = 0; j < CH; j += 4) {
            const double av = ph[(long long)(L0 + j) * 16 + lane];      // [image L0 + j + kk][row col]
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma16(av, chi[(j + kk) * LD + 16 * t + col], acc[t]);
        }
        __syncthreads();
    }

    // 4. AO tile -> LDS as ao[row][mu] (row = 2 k_local + re/im), then lane o contracts orbital o
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) chi[acc_row<double>(lane, g) * LD + 16 * t + (lane & 15)] = acc[t][g];
    __syncthreads();

    const int ns = sp ? A.n_dn : A.n_up;
    if (lane >= ns) return;
    const int k = A.orb_k[sp][lane];
    if ((k >> 3) != kg) return;
    const double* are = chi + (2 * (k & 7)) * LD;
    const double* aim = are + LD;
    const double* C = A.mo[sp];
    double ore = 0.0, oim = 0.0;
    for (int mu = 0; mu < A.nao; ++mu) {
        const double cr = C[2 * ((long long)mu * ns + lane)], ci = C[2 * ((long long)mu * ns + lane) + 1];
        ore += are[mu] * cr - aim[mu] * ci;
        oim += are[mu] * ci + aim[mu] * cr;
    }
    // wrap phase exp(i k . (wrap a))
    double t3[3];
    for (int c = 0; c < 3; ++c) t3[c] = wr[0] * A.a[c] + wr[1] * A.a[3 + c] + wr[2] * A.a[6 + c];
    const double ang = A.kpts[3 * k] * t3[0] + A.kpts[3 * k + 1] * t3[1] + A.kpts[3 * k + 2] * t3[2];
    double sn, cs;
    sincos(ang, &sn, &cs);
    row_out[2 * lane] = ore * cs - oim * sn;
    row_out[2 * lane + 1] = ore * sn + oim * cs;
}

// out_s[b][electron of spin s][orbital of spin s] at the electrons of B walkers: the spin follows from the electron index
template <typename T, int NT, int CH>
__global__ __launch_bounds__(64) void k_hf_orbitals(HfArgs A, const T* __restrict__ x, long long n_points,
                                                    double* __restrict__ out_up, double* __restrict__ out_dn) {
    const long long p = blockIdx.x;
    if (p >= n_points) return;
    const int N = A.n_up + A.n_dn;
    const long long b = p / N;
    const int e = (int)(p - b * N);
    const int sp = e < A.n_up ? 0 : 1;
    const int ns = sp ? A.n_dn : A.n_up;
    const int el = sp ? e - A.n_up : e;
    double r[3];
    for (int c = 0; c < 3; ++c) r[c] = (double)x[p * 3 + c];
    hf_orbital_row<NT, CH>(A, r, sp, blockIdx.y, (sp ? out_dn : out_up) + 2 * ((b * ns + el) * (long long)ns));
}

// out[p][orbital of spin sp] at P arbitrary points (P, 3): the spin is the caller's
template <typename T, int NT, int CH>
__global__ __launch_bounds__(64) void k_hf_orbitals_at(HfArgs A, const T* __restrict__ pts, long long n_points, int sp,
                                                       double* __restrict__ out) {
    const long long p = blockIdx.x;
    if (p >= n_points) return;
    double r[3];
    for (int c = 0; c < 3; ++c) r[c] = (double)pts[p * 3 + c];
    hf_orbital_row<NT, CH>(A, r, sp, blockIdx.y, out + 2 * p * (long long)(sp ? A.n_dn : A.n_up));
}

}  // namespace ds
