// ds_ecp.h -- the semi-local pseudopotential (ECP) energy of a batch of walkers: the local part summed directly, the non-local part
// from ratios psi(R') / psi(R) at quadrature points on a sphere around every ion an electron is close to.
//
// The reference has no pseudopotentials: the conventions are this project's own (include/deepsolid_hip.h).
//   v(r) = sum_k c_k r^(n_k - 2) exp(-zeta_k r^2), n_k in 0..4; a species has v_loc (without the -Z_eff / r tail, which Ewald carries)
//   and n_l channels v_l; inside its cutoff a function is used as it is, outside it is exactly 0.
//   E_loc(w) = sum_i sum_I [r_iI < r_cut_loc,I] v_loc,I(r_iI)
//   E_nl(w)  = sum_{(i,I): r_iI < r_cut_nl,I} sum_{q < N_q} (1 / N_q) W_iIq psi(R'_iIq) / psi(R),
//   W_iIq = sum_l (2l + 1) v_I,l(r_iI) P_l(U_q . dhat_iI),   R'_iIq = R with r_i replaced by r_i - d_iI + r_iI U_q (not wrapped),
//   U_q = Rot_w u_q: the octahedron (N_q = 6) or the icosahedron (N_q = 12) under one rotation per walker and call.
//
// Minimum image.  f = (r_i - R_I) . inv(a);  f <- f - floor(f + 1/2);  d = f . a;  r = |d|;  dhat = d / r (z if r = 0).
// Why this is the only image that can lie inside a cutoff: component c of f is the scalar product of d with column c of inv(a), so
// |f_c| <= r ||column c|| = r / height_c, that is r >= |f_c| height_c for every c.  Every cutoff is at most half the smallest
// height (ds_ecp_create refuses a larger one), so an image with r below a cutoff has every |f_c| < 1/2.  Two images differ by an
// integer in at least one component, and of all the numbers f_c + n only one lies in [-1/2, 1/2): the wrapped one.  Any other
// image has some |f_c| >= 1/2 and with it r >= height_c / 2 >= the cutoff: it is outside.
//
//   k_ecp_scan     one thread per walker: the walker's rotation (Philox stream 4, or the caller's), then every (i, I) in order:
//                  minimum image, E_loc added in (i, I) order, the pairs inside r_cut_nl counted; a walker with a non-finite
//                  coordinate is flagged and counts no pair
//   k_ecp_offsets  one workgroup: exclusive scan of the counts over the walkers, the total behind the last offset
//   k_ecp_fill     one thread per walker: the pair records (w, i, I, r, dhat, v_l(r)) at the walker's offset, in (i, I) order
//   (the host reads the total back: 8 bytes and ONE stream synchronisation, the only one of the call)
//   k_ecp_propose  one thread per (configuration, electron) of a chunk: the row of the walker, or the quadrature point
//   (value chain on the chunk: log|psi(R')|, phase(R'))
//   k_ecp_term     one thread per configuration: q = exp(log|psi(R')| - log|psi(R)|) phase(R') conj(phase(R)) and the term
//                  (W / N_q) q in float64 into the call's term buffer (and q, on request, into out_ratio)
//   k_ecp_walker   after the last chunk, one wave per walker: lane l adds the walker's terms l, l + 64, ... in order, lane 0 adds
//                  the 64 lane results in lane order -> out_energy[w] = (E_loc, Re E_nl, Im E_nl)
//
// Pairs are ordered by (w, i, I), configurations by (pair, q): configuration c = pair * N_q + q.  The order of every addition is a
// function of the walkers alone, and the chunks only decide which launch computes a term: the results are bit-identical for any
// workspace size and from run to run.  No floating-point atomics.  Distances, radial functions, Legendre polynomials and weights
// are float64 for either element type; the products and sums of the minimum image and of the radial functions are rounded one by
// one (no contraction into fused multiply-adds), so a host replay of them is bit-exact up to exp.
#pragma once
#include "ds_mcmc.h"

namespace ds {

constexpr int ECP_MAX_TERMS = 16;      // terms of one radial function
constexpr int ECP_SLOTS = 5;           // radial functions per species in the tables: v_loc, then v_l for l = 0..3
constexpr int ECP_MAX_L = 3;           // channels that run: l = 0..2 (l = 3 needs a rule of degree >= 6)

struct EcpDev {
    double a[9], ainv[9];              // simulation cell (rows = lattice vectors) and its inverse
    double quad[36];                   // the unrotated points u_q
    int n_atoms, n_species, n_quad;
    const double* atoms;               // (n_atoms, 3)
    const int* atom_species;           // (n_atoms,)
    const int* n_l;                    // (n_species,)
    const double *rc_loc, *rc_nl;      // (n_species,)
    const int* term_off;               // (n_species * ECP_SLOTS + 1,): the terms of slot j are term_off[j] .. term_off[j + 1] - 1
    const int* term_n;
    const double *term_z, *term_c;
};

// minimum image of p - R_I (see the head of the file) -> r, dh = dhat
__device__ __forceinline__ double ecp_min_image(const EcpDev& E, const double p[3], int I, double dh[3]) {
    const double* R = E.atoms + 3 * I;
    double d[3], r;
    {
#pragma clang fp contract(off)
        const double x0 = p[0] - R[0], x1 = p[1] - R[1], x2 = p[2] - R[2];
        double f[3];
        for (int c = 0; c < 3; ++c) f[c] = (x0 * E.ainv[c] + x1 * E.ainv[3 + c]) + x2 * E.ainv[6 + c];
        for (int c = 0; c < 3; ++c) f[c] = f[c] - floor(f[c] + 0.5);
        for (int c = 0; c < 3; ++c) d[c] = (f[0] * E.a[c] + f[1] * E.a[3 + c]) + f[2] * E.a[6 + c];
        r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }
    if (r > 0.0) { dh[0] = d[0] / r; dh[1] = d[1] / r; dh[2] = d[2] / r; }
    else { dh[0] = 0.0; dh[1] = 0.0; dh[2] = 1.0; }
    return r;
}

// radial function of table slot `slot` at r: the terms added in table order
__device__ __forceinline__ double ecp_radial(const EcpDev& E, int slot, double r) {
    double v = 0.0;
    {
#pragma clang fp contract(off)
        const double r2 = r * r;
        for (int k = E.term_off[slot]; k < E.term_off[slot + 1]; ++k) {
            const int n = E.term_n[k];
            const double pw = n == 0 ? 1.0 / r2 : n == 1 ? 1.0 / r : n == 2 ? 1.0 : n == 3 ? r : r2;
            v = v + (E.term_c[k] * pw) * exp(-(E.term_z[k] * r2));
        }
    }
    return v;
}

// whether the pair of an electron at distance r from an atom of species sp takes quadrature points
__device__ __forceinline__ bool ecp_nonlocal(const EcpDev& E, int sp, double r) { return E.n_l[sp] > 0 && r < E.rc_nl[sp]; }

// rotation of walker w: Philox stream 4, block A at index 2w, block B at index 2w + 1, counter `offset`, step 0; Shoemake's
// uniform unit quaternion and the standard matrix of a unit quaternion (row-major)
__device__ __forceinline__ void ecp_rotation(const PhiloxKey key, unsigned long long w, double R[9]) {
    const unsigned k0 = (unsigned)key.seed, k1 = (unsigned)(key.seed >> 32);
    const unsigned c2 = (unsigned)key.offset, c3 = (unsigned)(key.offset >> 32) & 0x3fffffffu;
    const unsigned long long ia = 2ull * w, ib = ia + 1;
    // stream 4 = stream 0 of a second bank: streams 0..3 fill the two top bits of c3, so stream 4 sets bit 29 of c3 beside
    // stream number 0 (an offset below 2^61 never reaches that bit)
    const unsigned c3s = c3 | 0x20000000u;
    const Philox4 pa = philox4x32_10((unsigned)ia, (unsigned)(ia >> 32), c2, c3s, k0, k1);
    const Philox4 pb = philox4x32_10((unsigned)ib, (unsigned)(ib >> 32), c2, c3s, k0, k1);
    const double u1 = u53_co(pa.v[0], pa.v[1]), u2 = u53_co(pa.v[2], pa.v[3]), u3 = u53_co(pb.v[0], pb.v[1]);
    double s2, c2a, s3, c3a;
    sincos(2.0 * DS_PI * u2, &s2, &c2a);
    sincos(2.0 * DS_PI * u3, &s3, &c3a);
    const double ra = sqrt(1.0 - u1), rb = sqrt(u1);
    const double x = ra * s2, y = ra * c2a, z = rb * s3, q = rb * c3a;
    {
#pragma clang fp contract(off)
        // (the factor 2 of the standard matrix as 2 / |quaternion|^2: the rounding of the norm then does not enter the orthogonality)
        const double s = 2.0 / ((x * x + y * y) + (z * z + q * q));
        R[0] = 1.0 - s * (y * y + z * z); R[1] = s * (x * y - z * q); R[2] = s * (x * z + y * q);
        R[3] = s * (x * y + z * q); R[4] = 1.0 - s * (x * x + z * z); R[5] = s * (y * z - x * q);
        R[6] = s * (x * z - y * q); R[7] = s * (y * z + x * q); R[8] = 1.0 - s * (x * x + y * y);
    }
}

// U_q = Rot u_q
__device__ __forceinline__ void ecp_point(const EcpDev& E, const double* __restrict__ rot, int q, double U[3]) {
    const double* u = E.quad + 3 * q;
    for (int c = 0; c < 3; ++c) U[c] = (rot[3 * c] * u[0] + rot[3 * c + 1] * u[1]) + rot[3 * c + 2] * u[2];
}

// per walker: rot (B, 9), eloc (B,), cnt (B,) pairs inside r_cut_nl, bad (B,) 1 for a walker with a non-finite coordinate
template <typename T>
__global__ void __launch_bounds__(64) k_ecp_scan(EcpDev E, const T* __restrict__ x, long long B, int N, PhiloxKey key,
                                                 const double* __restrict__ rotations, double* __restrict__ rot,
                                                 double* __restrict__ eloc, long long* __restrict__ cnt, int* __restrict__ bad,
                                                 double* __restrict__ out_rotation) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B) return;
    double R[9];
    if (rotations)
        for (int c = 0; c < 9; ++c) R[c] = rotations[9 * w + c];
    else
        ecp_rotation(key, (unsigned long long)w, R);
    for (int c = 0; c < 9; ++c) rot[9 * w + c] = R[c];
    if (out_rotation)
        for (int c = 0; c < 9; ++c) out_rotation[9 * w + c] = R[c];
    const T* xw = x + w * 3 * N;
    int nonfinite = 0;
    for (int c = 0; c < 3 * N; ++c) nonfinite |= !isfinite((double)xw[c]);
    if (nonfinite) {
        bad[w] = 1; cnt[w] = 0; eloc[w] = __builtin_nan("");
        return;
    }
    double e = 0.0;
    long long n = 0;
    for (int i = 0; i < N; ++i) {
        const double p[3] = {(double)xw[3 * i], (double)xw[3 * i + 1], (double)xw[3 * i + 2]};
        for (int I = 0; I < E.n_atoms; ++I) {
            double dh[3];
            const double r = ecp_min_image(E, p, I, dh);
            const int sp = E.atom_species[I];
            if (r < E.rc_loc[sp]) e += ecp_radial(E, sp * ECP_SLOTS, r);
            n += ecp_nonlocal(E, sp, r) ? 1 : 0;
        }
    }
    bad[w] = 0; cnt[w] = n; eloc[w] = e;
}

// off (B + 1,): off[w] = pairs of the walkers before w, off[B] = all pairs.  One workgroup: thread t takes a contiguous run of
// walkers (integer sums: the order is immaterial)
__global__ void __launch_bounds__(1024) k_ecp_offsets(const long long* __restrict__ cnt, long long B, long long* __restrict__ off,
                                                      long long* __restrict__ out_pairs) {
    __shared__ long long s_s[1024];
    const int t = threadIdx.x;
    const long long per = (B + 1023) / 1024;
    const long long lo = min((long long)t * per, B), hi = min(lo + per, B);
    long long s = 0;
    for (long long w = lo; w < hi; ++w) s += cnt[w];
    s_s[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = t >= d ? s_s[t - d] : 0;
        __syncthreads();
        s_s[t] += v;
        __syncthreads();
    }
    long long base = t > 0 ? s_s[t - 1] : 0;
    for (long long w = lo; w < hi; ++w) {
        off[w] = base;
        base += cnt[w];
        if (out_pairs) out_pairs[w] = cnt[w];
    }
    if (t == 1023) off[B] = s_s[1023];
}

// the records of walker w's pairs at off[w].., in (i, I) order: pw = w, pi = (i, I), pr = (r, dhat), pv = (v_0, v_1, v_2)(r) with
// 0 for the channels the species does not have.  A record beyond `capacity` is not written (the call then fails on the total)
template <typename T>
__global__ void __launch_bounds__(64) k_ecp_fill(EcpDev E, const T* __restrict__ x, long long B, int N, const int* __restrict__ bad,
                                                 const long long* __restrict__ off, long long capacity, long long* __restrict__ pw,
                                                 int* __restrict__ pi, double* __restrict__ pr, double* __restrict__ pv) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B || bad[w]) return;
    const T* xw = x + w * 3 * N;
    long long p = off[w];
    for (int i = 0; i < N; ++i) {
        const double pos[3] = {(double)xw[3 * i], (double)xw[3 * i + 1], (double)xw[3 * i + 2]};
        for (int I = 0; I < E.n_atoms; ++I) {
            double dh[3];
            const double r = ecp_min_image(E, pos, I, dh);
            const int sp = E.atom_species[I];
            if (!ecp_nonlocal(E, sp, r)) continue;
            if (p < capacity) {
                pw[p] = w; pi[2 * p] = i; pi[2 * p + 1] = I;
                pr[4 * p] = r; pr[4 * p + 1] = dh[0]; pr[4 * p + 2] = dh[1]; pr[4 * p + 3] = dh[2];
                for (int l = 0; l < ECP_MAX_L; ++l) pv[3 * p + l] = l < E.n_l[sp] ? ecp_radial(E, sp * ECP_SLOTS + 1 + l, r) : 0.0;
            }
            ++p;
        }
    }
}

struct EcpChunk {
    long long c0, n;                   // first configuration of the chunk, configurations in the chunk
    int N, n_quad;
};

// xd (n, 3N): row j is the walker of configuration c0 + j with electron i of its pair at r_i - d + r U_q
template <typename T>
__global__ void __launch_bounds__(256) k_ecp_propose(EcpDev E, EcpChunk A, const T* __restrict__ x, const double* __restrict__ rot,
                                                     const long long* __restrict__ pw, const int* __restrict__ pi,
                                                     const double* __restrict__ pr, T* __restrict__ xd) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n * A.N) return;
    const long long j = t / A.N, c = A.c0 + j, p = c / A.n_quad;
    const int el = (int)(t % A.N), q = (int)(c % A.n_quad);
    const long long w = pw[p];
    const T* in = x + (w * A.N + el) * 3;
    T* o = xd + t * 3;
    if (el != pi[2 * p]) {
        for (int k = 0; k < 3; ++k) o[k] = in[k];
        return;
    }
    double U[3];
    ecp_point(E, rot + 9 * w, q, U);
    const double r = pr[4 * p];
    for (int k = 0; k < 3; ++k) o[k] = (T)(((double)in[k] - r * pr[4 * p + 1 + k]) + r * U[k]);
}

// term (total, 2): (W / N_q) q of configuration c0 + j; out_ratio (total, 2) = q in the system's element type
template <typename T>
__global__ void __launch_bounds__(256) k_ecp_term(EcpDev E, EcpChunk A, const double* __restrict__ rot, const long long* __restrict__ pw,
                                                  const double* __restrict__ pr, const double* __restrict__ pv,
                                                  const T* __restrict__ la0, const T* __restrict__ ph0, const T* __restrict__ la,
                                                  const T* __restrict__ ph, double* __restrict__ term, T* __restrict__ out_ratio) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.n) return;
    const long long c = A.c0 + j, p = c / A.n_quad, w = pw[p];
    double U[3];
    ecp_point(E, rot + 9 * w, (int)(c % A.n_quad), U);
    const double t = (U[0] * pr[4 * p + 1] + U[1] * pr[4 * p + 2]) + U[2] * pr[4 * p + 3];
    const double W = (pv[3 * p] + 3.0 * pv[3 * p + 1] * t + 5.0 * pv[3 * p + 2] * (0.5 * (3.0 * t * t - 1.0))) / (double)A.n_quad;
    const double mag = exp((double)la[j] - (double)la0[w]);
    const double pr_ = (double)ph[2 * j], pi_ = (double)ph[2 * j + 1], rr = (double)ph0[2 * w], ri = (double)ph0[2 * w + 1];
    const double qr = mag * (pr_ * rr + pi_ * ri), qi = mag * (pi_ * rr - pr_ * ri);       // phase(R') conj(phase(R))
    term[2 * c] = W * qr; term[2 * c + 1] = W * qi;
    if (out_ratio) { out_ratio[2 * c] = (T)qr; out_ratio[2 * c + 1] = (T)qi; }
}

// out_energy (B, 3) = (E_loc, Re E_nl, Im E_nl); NaN in all three for a flagged walker.  The walker's terms are those of the
// configurations off[w] N_q .. off[w + 1] N_q - 1
constexpr int ECP_WAVES = 4;           // walkers per workgroup of k_ecp_walker
__global__ void __launch_bounds__(64 * ECP_WAVES) k_ecp_walker(const double* __restrict__ term, const long long* __restrict__ off,
                                                               const double* __restrict__ eloc, const int* __restrict__ bad,
                                                               long long B, int n_quad, double* __restrict__ out_energy) {
    __shared__ double l_s[ECP_WAVES][64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * ECP_WAVES + wave;
    double ar = 0.0, ai = 0.0;
    if (w < B && !bad[w]) {
        const long long c0 = off[w] * n_quad, c1 = off[w + 1] * n_quad;
        for (long long c = c0 + lane; c < c1; c += 64) { ar += term[2 * c]; ai += term[2 * c + 1]; }
    }
    l_s[wave][lane][0] = ar; l_s[wave][lane][1] = ai;
    __syncthreads();
    if (lane == 0 && w < B) {
        double tr = l_s[wave][0][0], ti = l_s[wave][0][1], e = eloc[w];
        for (int l = 1; l < 64; ++l) { tr += l_s[wave][l][0]; ti += l_s[wave][l][1]; }
        if (bad[w]) e = tr = ti = __builtin_nan("");
        out_energy[3 * w] = e; out_energy[3 * w + 1] = tr; out_energy[3 * w + 2] = ti;
    }
}

// The heat-bath T-move of ds_dmc_step_tmove (Casula 2006; include/deepsolid_hip.h has the normative text), on what an evaluation of
// the walkers at x left in its workspace.  One thread per walker walks the walker's terms twice, in configuration order:
//   t_c = -tau min(Re term_c, 0);  r_{-1} = 1, r_c = r_{c-1} + t_c (one rounded float64 addition each);  Z = r_last;
//   theta = u Z;  theta < 1 (or no t_c > 0): no move;  else c = #{c: r_c <= theta}, clamped to the last c with t_c > 0.
// Only a walker of positive weight and finite energy with at least one pair moves.  The electron of the chosen pair goes to the
// quadrature point by the arithmetic of k_ecp_propose and is wrapped as k_dmc_propose wraps; nothing else of the row changes.
// choice[w] (and out_choice[w]) = the walker-local configuration pair_local * N_q + q, or -1.  A few hundred terms per walker: the
// sequential walk is the normative order and costs nothing beside the evaluation.
template <typename T>
__global__ void __launch_bounds__(64) k_ecp_tmove(EcpDev E, const T* __restrict__ a, const T* __restrict__ ainv, T* __restrict__ x, long long B,
                                                  int N, double tau, const double* __restrict__ rot, const long long* __restrict__ off,
                                                  const int* __restrict__ pi, const double* __restrict__ pr,
                                                  const double* __restrict__ term, const double* __restrict__ weight,
                                                  const double* __restrict__ energy, const double* __restrict__ uniform, PhiloxKey key,
                                                  unsigned long long step, int* __restrict__ choice, int* __restrict__ out_choice) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= B) return;
    const long long p0 = off[w], n = (off[w + 1] - p0) * E.n_quad;
    long long ch = -1;
    if (weight[w] > 0.0 && isfinite(energy[w]) && n > 0) {
        const double* t = term + 2 * p0 * E.n_quad;
        double r = 1.0, theta;
        long long last = -1;
        {
#pragma clang fp contract(off)
            for (long long c = 0; c < n; ++c) {
                const double re = t[2 * c], tc = -tau * (re < 0.0 ? re : 0.0);
                r = r + tc;
                if (tc > 0.0) last = c;
            }
            const double u = uniform ? uniform[w] : philox_uniform(key, step, (unsigned long long)(B + 1 + w));
            theta = u * r;
        }
        if (!(theta < 1.0) && last >= 0) {
#pragma clang fp contract(off)
            long long c = 0;
            r = 1.0;
            for (; c < n; ++c) {                       // (the r_c do not decrease: the count is the first c with r_c > theta)
                const double re = t[2 * c];
                r = r + -tau * (re < 0.0 ? re : 0.0);
                if (!(r <= theta)) break;
            }
            ch = c < last ? c : last;
        }
    }
    choice[w] = (int)ch;
    if (out_choice) out_choice[w] = (int)ch;
    if (ch < 0) return;
    const long long p = p0 + ch / E.n_quad;
    T* xe = x + (w * N + pi[2 * p]) * 3;
    double U[3];
    ecp_point(E, rot + 9 * w, (int)(ch % E.n_quad), U);
    const double rr = pr[4 * p];
    T pos[3], o[3], wr[3];
    for (int k = 0; k < 3; ++k) pos[k] = (T)(((double)xe[k] - rr * pr[4 * p + 1 + k]) + rr * U[k]);
    wrap_point(pos, a, ainv, o, wr);
    for (int k = 0; k < 3; ++k) xe[k] = o[k];
}

}  // namespace ds
