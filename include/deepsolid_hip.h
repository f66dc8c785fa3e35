/*
 * deepsolid_hip.h -- C ABI of libdeepsolid_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the VMC inner loop of bytedance/DeepSolid.  The reference
 * has no FFI layer: the boundary is three Python factories whose closures are
 * consumed by process.py / train.py.  Each entry point below names the reference
 * function(s) whose arithmetic it replaces; the Python side
 * (deepsolid_amd/{network,hamiltonian,qmc,ewaldsum,distance}.py) keeps the
 * reference signatures and calls these through ctypes with raw device pointers.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; ds_last_error()
 *     returns a thread-local message for the last failure;
 *   - all `const void*` / `void*` data arguments are DEVICE pointers owned by the
 *     caller (torch tensors), element type given by ds_system_desc.dtype
 *     (0 = float64, 1 = float32); walkers are (B, 3*N) row-major, B = batch;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); nothing is
 *     allocated or synchronised after ds_system_create.  A handle carries device
 *     scratch of its own (the int8 digit planes of the hidden-layer weights, refilled
 *     by the first launch of every call that takes `params`): calls on ONE handle
 *     must be issued from one host thread and complete in issue order (one stream, or
 *     streams ordered by events); for concurrent streams create one handle per stream;
 *   - no torch types appear anywhere in this interface.
 */
#ifndef DEEPSOLID_HIP_H
#define DEEPSOLID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_MAX_LAYERS 8
#define DS_MAX_SYM 6 /* rows of AV/BV: 3 ('minimal'), 4 (fcc/hexagonal), 6 (bcc) -- supercell.py:98-140 */

typedef struct ds_system ds_system; /* opaque handle, one per device */

/* Host-side description of one simulation cell + network architecture.  All
 * pointers are HOST pointers to float64 / int data and are copied by
 * ds_system_create.  Field provenance (reference file:line):
 *   n_up,n_dn            simulation_cell.nelec                      network.py:644
 *   prim_* / sim_*       simulation_cell.original_cell.a/.AV/.BV,
 *                        simulation_cell.a/.AV/.BV                  network.py:281-296
 *   prim_atoms           original_cell.atom_coords()                network.py:643
 *   klist_up/dn          hf.SCF.klist                               hf.py:84-104
 *   hidden_single/double, n_det, ...  cfg.network.detnet            base_config.py:129-139
 *   ewald_*              EwaldSum.__init__ products                 ewaldsum.py:34-136
 *   dist_mode            MinimalImageDistance dispatch              distance.py:43-61
 */
typedef struct ds_system_desc {
    int32_t dtype;               /* 0 = f64, 1 = f32 */
    int32_t n_up, n_dn;
    int32_t n_atoms_prim;
    const double* prim_atoms;    /* (n_atoms_prim, 3) */
    double prim_a[9];
    double sim_a[9];
    int32_t n_sym;               /* rows of AV/BV */
    double prim_AV[DS_MAX_SYM * 3], prim_BV[DS_MAX_SYM * 3];
    double sim_AV[DS_MAX_SYM * 3], sim_BV[DS_MAX_SYM * 3];
    /* network */
    int32_t n_layers;            /* len(hidden_dims) */
    int32_t hidden_single[DS_MAX_LAYERS];   /* the REFERENCE's hidden_dims[l][0] verbatim (network.py:111-132): 1..1024 */
    int32_t hidden_double[DS_MAX_LAYERS];   /* ... hidden_dims[l][1]: 1..32.  The library pads both internally (ds_device_widths) */
    int32_t n_det;               /* determinants */
    int32_t distance_type;       /* 0 = 'nu' (network.py:207), 1 = 'tri' (network.py:227; isotropic envelope only) */
    int32_t envelope_type;       /* 0 = 'isotropic' (network.py:335), 1 = 'diagonal' (:340), 2 = 'full' (:358) */
    int32_t full_det;            /* 0 block-diagonal determinants per spin (base_config default), 1 dense N x N (network.py:558) */
    int32_t use_last_layer;      /* 1: the orbital head takes the symmetric features of the last layer (network.py:535) */
    int32_t bias_orbitals;       /* 1: orbital[s]['b'] is added to the orbital head (network.py:181-184) */
    const double* klist_up;      /* (n_up, 3) */
    const double* klist_dn;      /* (n_dn, 3) */
    /* Ewald tables */
    int32_t n_atoms_sim;
    const double* sim_atoms;     /* (n_atoms_sim, 3) */
    const double* sim_charges;   /* (n_atoms_sim,) */
    int32_t dist_mode;           /* 0 diagonal, 1 orthogonal, 2 general */
    int32_t n_g;
    const double* gpoints;       /* (n_g, 3) */
    const double* gweight;       /* (n_g,) */
    const double* ion_exp_re;    /* (n_g,)  Re sum_a Z_a exp(i G.R_a) */
    const double* ion_exp_im;    /* (n_g,) */
    double ewald_alpha;
    double ee_const;             /* EwaldSum.ee_const(N)   ewaldsum.py:109 */
    double ei_const;             /* EwaldSum.ei_const(N)   ewaldsum.py:112 */
    double ii_total;             /* ion_ion + ii_const     ewaldsum.py:190 */
} ds_system_desc;

/* Parameter buffer: one flat device array of `dtype` elements.  ds_param_layout
 * reports, for the handle's architecture, the element offset and the logical
 * (rows, cols) of every block in this order:
 *   for l in layers:  W_loc_l  [(h1_in + nch*h2_in), h1_out]   rows: h_i | mean_j h2_ij (up) | (dn)
 *                     W_sh_l   [(nch*h1_in), h1_out]           rows: mean_up h | mean_dn h
 *                     b_l      [1, h1_out]
 *   for l in double layers: W2_l [h2_in, h2_out], b2_l [1, h2_out]        (n_layers-1 of them, n_layers with use_last_layer)
 *   for s in active spins:  W_orb_s [h1_last (+ nch*h2_last with use_last_layer), cols]  cols = 2*norb*n_det rounded up to 64,
 *                             norb = n_s (N with full_det); Re/Im columns interleaved per 16-column tile, see
 *                             deepsolid_amd/params.py::orbital_column_map and csrc/ds_gemm.h::orb_col
 *                           [W_sh_orb_s [nch*h1_last, cols]   only with use_last_layer]
 *                           [b_orb_s [1, 2*norb*n_det]        only with bias_orbitals]
 *                           pi_s [A, norb*n_det], sigma_s [A | 3A | 9A, norb*n_det] (isotropic | diagonal | full)
 * Layer-0 rows are padded with zero rows to multiples of 4 (only 'tri', 7 features, needs it).
 * i.e. the rows of the reference's `single[l]['w']` (network.py:126-158) split
 * into the per-electron and the shared (spin-mean) part. */
typedef struct ds_param_block {
    int64_t offset;
    int32_t rows, cols;
} ds_param_block;

/* The widths the kernels run for the reference's hidden_dims, and where a residual is added (host code, needs no GPU).
 * One-electron widths are zero-padded to multiples of 64, pair widths to 16 or 32 -- exact: a padded feature is tanh(0) = 0 in
 * every layer and meets zero rows in the next.  res_single[l] / res_double[l] = 1 where the reference adds a residual
 * (network.py:525-528: input width == output width of the REFERENCE's widths), independent of the padded widths.
 * n_in_single / n_in_double: widths of the input features (nf * atoms, nf; nf = 4 for 'nu', 7 for 'tri'); n_double: pair layers
 * that run (n_layers - 1, or n_layers with use_last_layer).  ds_system_create applies exactly this to its descriptor;
 * ds_param_layout reports the PADDED block shapes: a caller copies each reference block into the top-left corner of its
 * padded segments ([h | pair-up | pair-dn] rows of W_loc, [mean-up | mean-dn] rows of W_sh, ...) and leaves the rest zero. */
int ds_device_widths(const int32_t* hidden_single, const int32_t* hidden_double, int32_t n_layers, int32_t n_in_single,
                     int32_t n_in_double, int32_t n_double, int32_t* dev_single, int32_t* dev_double, int32_t* res_single,
                     int32_t* res_double);

int ds_system_create(const ds_system_desc* desc, ds_system** out);
void ds_system_destroy(ds_system* sys);
const char* ds_last_error(void);

/* Number of dense hidden one-electron layers per local-energy evaluation whose per-electron contraction runs as a 47-bit
 * truncating fixed-point split on the int8 matrix pipe (csrc/ds_i8.h: float64 in, float64 out; 5-slot-tile float64 cells with 256
 * features).  Opt-in since round 6 (environment DS_I8=1 at ds_system_create): 0 otherwise, or when the architecture has no instance. */
int ds_int8_layers(const ds_system* sys);

/* Number of pair-stream layers per local-energy evaluation (dump != 0: per stage dump) that run the pair layer in front of them in
 * registers instead of reading its output (float64 cells whose pair layers write the pair-mean rows themselves; 0 with
 * DS_NO_PAIR_RECOMPUTE=1 at ds_system_create, for float32 handles and in a stage dump). */
int ds_pair_recompute_layers(const ds_system* sys, int dump);

int64_t ds_param_count(const ds_system* sys);
/* fills up to `max_blocks` entries, returns the number of blocks */
int ds_param_layout(const ds_system* sys, ds_param_block* blocks, int max_blocks);

/* bytes of scratch the calls below need for a batch of B walkers */
int64_t ds_workspace_bytes(const ds_system* sys, int64_t B);

/* network.eval_func (network.py:563-606), methods eval_phase_and_slogdet /
 * eval_slogdet / eval_logdet, batched as process.py:116-118 vmaps it.
 * out_logabs (B,), out_phase (B,2) = (Re, Im) of the unit phase; either may be NULL. */
int ds_logpsi(ds_system* sys, const void* params, const void* x, int64_t B,
              void* out_logabs, void* out_phase, void* ws, int64_t ws_bytes, void* stream);

/* value and gradient of log psi w.r.t. the walker coordinates: what qmc.make_mcmc_step builds with
 * jax.vmap(jax.value_and_grad(importance_sampling, argnums=1)) (qmc.py:324) for importance_update
 * (qmc.py:83-150).  out_grad (B, 3N, 2): Re = grad log|psi|, Im = grad arg psi.  Uses the
 * forward-Laplacian chain (the gradient is its trace stage); out_logabs / out_phase optional. */
int ds_logpsi_grad(ds_system* sys, const void* params, const void* x, int64_t B,
                   void* out_logabs, void* out_phase, void* out_grad, void* ws, int64_t ws_bytes, void* stream);

/* Parameter gradient of  L = sum_b [ cot[b][0] * log|psi_b| + cot[b][1] * arg psi_b ]  (reverse sweep over
 * the value chain).  This is the vector-Jacobian product the reference obtains from jax.jvp / jax.grad of
 * batch_network inside the custom JVP of total_energy (train.py:91-142): with cot = clip_diff / B (Re, Im)
 * the result is  tangents_dot = mean(Re(clip_diff * conj(d log psi)))  for every parameter direction, i.e.
 * the energy gradient jax.value_and_grad(total_energy) returns (train.py:147-176, process.py:226-228).
 * cot (B, 2); grad (ds_param_count(),) in the packed layout of ds_param_layout, overwritten (padding entries
 * are zero); out_logabs / out_phase optional.  Every network option of ds_system_desc is supported.
 * Weight gradients are reduced over
 * walkers in a fixed order (no atomics): the result is bit-reproducible run to run. */
int64_t ds_vjp_workspace_bytes(const ds_system* sys, int64_t B);
int ds_logpsi_vjp(ds_system* sys, const void* params, const void* x, int64_t B, const void* cot, void* grad,
                  void* out_logabs, void* out_phase, void* ws, int64_t ws_bytes, void* stream);

/* Orbital-matching pretraining (pretrain.py:70-94, make_pretrain_step's loss_fn and its jax.value_and_grad):
 *   loss = mean over the spin channels with electrons of  mean_{b,k,i,m} |target_s[b,i,m] - M_s[b,k,i,m]|^2,
 * M = the orbital matrices of ds_orbitals.  target_up (B, n_up, n_up, 2), target_dn (B, n_dn, n_dn, 2) in the layout of
 * hf.SCF.eval_orb_mat, [walker, electron, orbital] complex as (Re, Im) pairs; target_dn is NULL when n_dn = 0.  With full_det
 * the single dense target is blockdiag(target_up, target_dn) (pretrain.py:79-86); the zero blocks are implied, never passed.
 * The means run over the B walkers of THIS call (per-device jnp.mean; the caller averages loss and gradient over ranks).
 * out_loss (1,) float64 on the device for both dtypes (a float32 system sums |r|^2 per workgroup in float32; the per-workgroup
 * partials are added in float64); grad (ds_param_count(),) packed like ds_logpsi_vjp's, overwritten,
 * padding entries zero.  The batch is processed in chunks that fit ws; loss and gradient are summed in a fixed order (no
 * atomics): two calls give the same bits.  The forward stops behind the orbital head: no determinant work is launched.
 * Nothing is allocated or synchronised.  B = 0: zero loss, zero gradient.  Every network option of ds_system_desc is supported. */
int64_t ds_pretrain_workspace_bytes(const ds_system* sys, int64_t B);
int ds_pretrain_loss_vjp(ds_system* sys, const void* params, const void* x, int64_t B, const void* target_up,
                         const void* target_dn, void* out_loss, void* grad, void* ws, int64_t ws_bytes, void* stream);

/* KFAC factor pass: the curvature statistics of the reference's default optimizer (process.py:209-228,
 * kfac_ferminet_alpha.Optimizer with estimation_mode = 'fisher_exact' on the normal predictive distribution train.py:133 registers).
 * Every linear layer is a `repeated_dense` block (network.py:430-446; curvature_blocks.py:158-281).  With x the layer's input
 * rows -- one per walker and repeat --, x~ = [x | 1] when the layer has a bias, and dy = sqrt2 * d log|psi_b| / d (layer output)
 * (the one extra reverse sweep of 'fisher_exact': seed 1 / sqrt(variance 0.5) on every walker, independent of E_L),
 *   A = x~^T x~ / (B R)  (d_in x d_in),   G = dy^T dy / (B R)  (d_out x d_out).
 * ds_kfac_layout describes the blocks, in the order single[0..], double[0..], orbital[0..]:
 *   kind / index      0 one-electron layer l (R = N), 1 pair layer l (R = N^2), 2 orbital head of spin channel s (R = n_s)
 *   param_blocks      the n_param_blocks entries of ds_param_layout the block covers: W_loc [, W_sh] [, b]
 *   d_in, d_out       the REFERENCE's unpadded sizes, d_in including the bias row when has_bias; rows of A in the reference's
 *                     order [h | mean_up h | mean_dn h | pair-mean_up | pair-mean_dn | 1] (empty spin channels dropped,
 *                     network.py:327-328), columns of G in the order of the reference's weight columns (orbital head: Re | Im)
 *   a_offset, g_offset  element offsets of A and G in `factors` (row-major); the last block's g_offset + d_out^2 is its length
 * ds_kfac_factors runs the value chain and ONE reverse sweep with cotangent (sqrt2, 0) on every walker (the buffers and kernels
 * of ds_logpsi_vjp) and overwrites `factors` with every block's A and G, already divided by B R, exactly symmetric.  The
 * contractions over (repeat, walker) run as symmetric rank-k updates on the MFMA pipe (csrc/ds_kfac.h), upper triangle only;
 * padded rows and walkers beyond the batch never reach the output.  grad_seed (ds_param_count(),), may be NULL: the packed
 * gradient of the same seed, sum_b sqrt2 log|psi_b| (the untagged envelope parameters take their diagonal curvature from it,
 * curvature_blocks.py:111-154).  The batch is processed in the chunks that fit ws; all sums run in a fixed order without atomics:
 * two calls give the same bits.  Nothing is allocated or synchronised.  B = 0: zeros.  envelope_type 'full' is not supported
 * (its sigma is a tagged block of its own, `qmc1`, network.py:358-362): the call returns an error. */
typedef struct ds_kfac_block {
    int32_t kind, index;
    int32_t n_param_blocks;
    int32_t param_blocks[3];
    int32_t has_bias, d_in, d_out, repeats;
    int64_t a_offset, g_offset;
} ds_kfac_block;
int ds_kfac_block_count(const ds_system* sys);
int ds_kfac_layout(const ds_system* sys, ds_kfac_block* blocks, int max_blocks);
int64_t ds_kfac_workspace_bytes(const ds_system* sys, int64_t B);
int ds_kfac_factors(ds_system* sys, const void* params, const void* x, int64_t B, void* factors, void* grad_seed, void* ws,
                    int64_t ws_bytes, void* stream);

/* KFAC step, device part (csrc/ds_kfac.h; reference utils.py:130-218, curvature_blocks.py:233-281).  Both calls work on the
 * blocks of ds_kfac_layout, enqueue on `stream`, allocate nothing, read nothing back and use no atomics: two calls give the
 * same bits.  ws: ds_kfac_step_workspace_bytes() bytes, shared by the two calls.
 * ds_kfac_inverses: `factors` holds the raw moving-average arrays in the flat layout of ds_kfac_factors; their value is
 *   array / ema_weight.  With lambda = damping / R (damping = l2_reg + damping of the optimizer), n0 = tr A, n1 = tr G, s = n0 n1,
 *     s > 0:  A^- = (A / n0 + sqrt(lambda d_out / (s d_in)) I)^-1 / sqrt(s),  G^- = (G / n1 + sqrt(lambda d_in / (s d_out)) I)^-1 / sqrt(s)
 *     else:   both I / sqrt(lambda)
 *   is written to `inverses` in the same layout, exactly symmetric.  Traces, the branch and the damping terms are computed on
 *   the device.  The elimination (blocked Gauss-Jordan without pivoting, block 32, trailing update on the f64 MFMA, then one
 *   Newton step X (2 I - M X)) runs in float64 for both dtypes.  A block with d_in == 1 or d_out == 1 is refused (the reference treats it specially).
 * ds_kfac_precondition: v and out hold one dense row-major d_in x d_out matrix per block in layout order (block b starts at
 *   element sum_{j<b} d_in_j d_out_j); out_b = A^-_b v_b G^-_b / R_b and sq_norm[b] = sum(out_b o v_b), accumulated in float64
 *   in a fixed order (sq_norm: n_blocks float64 values on the device).
 * ds_kfac_inverses_sized: the same inverse kernels on blocks of explicit sizes, without a system handle (n_blocks <= 18;
 *   dtype 0 float64, 1 float32; flat layout A_0, G_0, A_1, ...): the general formula above for ANY size, 1 included.  For tests
 *   of the block arithmetic at sizes the network layouts do not reach. */
int64_t ds_kfac_step_workspace_bytes(const ds_system* sys);
int ds_kfac_inverses(ds_system* sys, const void* factors, double ema_weight, double damping, void* inverses, void* ws,
                     int64_t ws_bytes, void* stream);
int ds_kfac_precondition(ds_system* sys, const void* inverses, const void* v, void* out, double* sq_norm, void* ws,
                         int64_t ws_bytes, void* stream);
int64_t ds_kfac_inverses_sized_workspace_bytes(int n_blocks, const int32_t* d_in, const int32_t* d_out);
int ds_kfac_inverses_sized(int dtype, int n_blocks, const int32_t* d_in, const int32_t* d_out, const int32_t* repeats,
                           const void* factors, double ema_weight, double damping, void* inverses, void* ws, int64_t ws_bytes,
                           void* stream);

/* Per-walker Jacobian of log psi_b = u_b + i phi_b (u = log|psi|, phi = arg psi) with respect to the packed parameters: the
 * primitive of the sample-space optimizers (MinSR, SPRING; deepsolid_amd/spring.py).  jac is (2B, ld) row-major in the system's
 * dtype, ld >= ds_param_count(): row b = d u_b / d theta, row B + b = d phi_b / d theta, in the packed layout of
 * ds_param_layout -- the gradient ds_logpsi_vjp returns for a cotangent that is (1, 0), resp. (0, 1), on walker b and zero
 * elsewhere.  Every column in [0, ds_param_count()) of every row is written, padding columns with exact zeros; columns beyond
 * are not touched.  out_logabs / out_phase optional, as in ds_logpsi_vjp.  Per chunk of the batch that fits ws the value chain
 * runs once and the reverse sweep twice (seed (1, 0), then (0, 1), on every walker; the sweep leaves the chain's buffers
 * intact), with the per-walker kernels of csrc/ds_jac.h in place of the batch-summed contractions.  Nothing is allocated or
 * synchronised.  All sums run in a fixed order without atomics: two calls give the same bits, a capped workspace gives the
 * same bits as an uncapped one.  B = 0 succeeds and writes nothing.  Every network option of ds_system_desc is supported. */
int64_t ds_jacobian_workspace_bytes(const ds_system* sys, int64_t B);
int ds_logpsi_jacobian(ds_system* sys, const void* params, const void* x, int64_t B, void* jac, int64_t ld, void* out_logabs,
                       void* out_phase, void* ws, int64_t ws_bytes, void* stream);

/* Linear algebra on such a Jacobian (csrc/ds_minsr.h), without a system handle: jac is (R, ld) row-major, P <= ld columns count.
 * dtype 0: float64 operands, 1: float32 (converted on load).  All accumulation is float64; no atomics: two calls give the same
 * bits.  Each call enqueues on `stream`, allocates nothing and reads nothing back; ws: what its *_workspace_bytes reports.
 * ds_minsr_gram:   G = J J^T (R x R float64).  Only the 128 x 128 tiles on and above the diagonal are computed, on
 *   v_mfma_f64_16x16x4_f64 from LDS-staged row panels; both triangles are written from them: symmetric to the bit.  For small R
 *   the P axis is split over workgroups and the partials are added in index order (the split depends on the shape alone).
 * ds_minsr_matvec: mode 0: out = J v (R,), mode 1: out = J^T v (P,); v and out float64.  One pass over J, fixed-order sums.
 * ds_minsr_solve:  (scale H G H + lambda I) zeta = rhs in float64.  H centres each consecutive `block` rows and columns
 *   (block = 0: no centring); R % block == 0 and lambda > 0 are checked before any launch.  The matrix is formed exactly
 *   symmetric from the upper triangle of G, inverted by the blocked Gauss-Jordan elimination and Newton step of the KFAC
 *   inverses (csrc/ds_kfac.h), and zeta = X rhs takes one step of iterative refinement against the matrix itself. */
int64_t ds_minsr_gram_workspace_bytes(int64_t R, int64_t P);
int ds_minsr_gram(int dtype, const void* jac, int64_t R, int64_t P, int64_t ld, double* G, void* ws, int64_t ws_bytes, void* stream);
int64_t ds_minsr_matvec_workspace_bytes(int mode, int64_t R, int64_t P);
int ds_minsr_matvec(int dtype, int mode, const void* jac, int64_t R, int64_t P, int64_t ld, const double* v, double* out, void* ws,
                    int64_t ws_bytes, void* stream);
int64_t ds_minsr_solve_workspace_bytes(int64_t R, int64_t block);
int ds_minsr_solve(int64_t R, int64_t block, double scale, double lambda, const double* G, const double* rhs, double* zeta, void* ws,
                   int64_t ws_bytes, void* stream);

/* network.eval_func method 'eval_mats' (network.py:601): out_up (B, n_det, n_up, n_up, 2),
 * out_dn (B, n_det, n_dn, n_dn, 2), complex as (Re, Im) pairs. */
int ds_orbitals(ds_system* sys, const void* params, const void* x, int64_t B,
                void* out_up, void* out_dn, void* ws, int64_t ws_bytes, void* stream);

/* ewaldsum.EwaldSum.energy (ewaldsum.py:185-191): out (B,3) = (ee, ei, ii). */
int ds_ewald(ds_system* sys, const void* x, int64_t B, void* out, void* stream);

/* hamiltonian.local_energy_seperate (hamiltonian.py:194-228), all Laplacian modes
 * (for / dim_batch / hessian / partition return the same numbers and map to one
 * forward-Laplacian kernel chain).  out_ke (B,2) = complex kinetic energy,
 * out_ewald (B,) = ee+ei+ii; out_logabs (B,) / out_phase (B,2) optional (NULL). */
int ds_local_energy(ds_system* sys, const void* params, const void* x, int64_t B,
                    void* out_ke, void* out_ewald, void* out_logabs, void* out_phase,
                    void* ws, int64_t ws_bytes, void* stream);

/* distance.enforce_pbc (distance.py:144-163), batched over B*N electrons; needs no handle.
 * latvec: HOST pointer to the 3x3 lattice (rows = lattice vectors); dtype 0 = f64, 1 = f32;
 * x, out_x: (n_elec, 3) device arrays; out_wrap (n_elec, 3) device array or NULL. */
int ds_enforce_pbc(const double* latvec, int dtype, const void* x, int64_t n_elec, void* out_x,
                   void* out_wrap, void* stream);

/* Walker observables of estimator.py (complex polarization :15-42, structure factor :44-84) as float64 sums over the batch;
 * needs no handle.  recvec: HOST pointer to the simulation cell's reciprocal vectors (3x3, row j = g_j = 2 pi inv(a)^T row j);
 * dtype 0 = f64, 1 = f32; x: (B, 3 n_elec) device array, 1 <= n_elec <= 128, B >= 1;
 * q_int: HOST pointer to n_q (0..512) integer points (n1, n2, n3), 0 <= n_j <= 7, q = n1 g_1 + n2 g_2 + n3 g_3;
 * pol_direction: 0..2, or -1 for no polarization.  out_sums: device array of 2 + 3 n_q doubles,
 *   [sum_b Re P_b, sum_b Im P_b, sum_b Re rho_b(q_k) (k < n_q), sum_b Im rho_b(q_k) (k < n_q), sum_b |rho_b(q_k)|^2 (k < n_q)]
 * with P_b = exp(i sum_e g_dir . r_be), rho_b(q) = sum_e exp(i q . r_be); the polarization pair is 0 when pol_direction = -1.
 * ws: device workspace of at least ds_observables_workspace_bytes(B, n_q) bytes.  Fixed reduction order, no atomics:
 * the same input gives bit-identical sums. */
int64_t ds_observables_workspace_bytes(int64_t B, int n_q);
int ds_observables(const double* recvec, int dtype, const void* x, int64_t B, int64_t n_elec, const int32_t* q_int, int n_q,
                   int pol_direction, double* out_sums, void* ws, int64_t ws_bytes, void* stream);

/* Real-space walker observables as integer counts (csrc/ds_realspace.h): the spin-resolved electron density on a grid of a
 * folding lattice, and the spin-resolved radial pair histogram behind g(r).  Needs no handle and no workspace.  The reference has
 * no such estimator: the conventions are this library's own.  One call takes the walkers x (B, 3 n_elec) (device array; dtype
 * 0 = f64, 1 = f32 widened to f64 on load; all arithmetic is float64) and ADDS to two caller-owned int64 device buffers; it never
 * zeroes them.  Either buffer may be NULL: that part is skipped and its arguments are not read; both NULL is an error.
 *
 * Density counts dens[2][g0*g1*g2]:
 *   - Spin of electron e is 0 if e < n_up, else 1.
 *   - The electron is folded into a folding lattice A_f (3x3, rows = lattice vectors; normally the primitive cell, or any lattice
 *     whose translations are symmetries, for example the simulation cell itself).
 *   - Folding rule: f = r . inv(A_f), f -= floor(f), i_j = min(int(f_j * g_j), g_j - 1).
 *   - Flat bin index: (i0*g1 + i1)*g2 + i2.
 *   fold_inv: HOST pointer to inv(A_f), row-major; grid: HOST pointer to (g0, g1, g2).
 *
 * Pair counts pair[3][n_r]:
 *   - Channels are up-up, up-down, down-down.
 *   - For each pair i < j, take the minimum-image distance in the simulation cell A.
 *   - Rule: f = (r_i - r_j) . inv(A), f -= floor(f + 1/2).  Then take the shortest of |(f + s) . A| over s in {-1,0,1}^3.
 *   - Bin index: k = int(r * n_r / r_max).  Count the pair only if r < r_max.
 *   latvec / latvec_inv: HOST pointers to A (rows = lattice vectors) and inv(A).  The caller guarantees two conditions:
 *   r_max <= r_ws, half the shortest non-zero lattice vector (at most one image can then lie inside r_max), and
 *   r_max < 1.5 * the smallest plane spacing of A (the 27 shifts are then enough).
 *
 * Limits, refused with a ds_last_error message before any launch: 1 <= n_elec <= 128, 0 <= n_up <= n_elec, 1 <= g_j <= 256,
 * g0*g1*g2 <= 2^22, 1 <= n_r <= 1024, r_max > 0, B >= 1.  Counts are added with integer atomics, so the buffers do not depend on
 * the order of the additions: the same input gives bit-identical counts. */
int ds_realspace_counts(const double* fold_inv, const int32_t* grid, const double* latvec, const double* latvec_inv, double r_max,
                        int n_r, int dtype, const void* x, int64_t B, int64_t n_elec, int64_t n_up, int64_t* dens, int64_t* pair,
                        void* stream);

/* qmc.mh_update symmetric branch (qmc.py:190-196, 217-222) split around the network call:
 *   propose: x2 = wrap(x1 + width * normal)
 *   accept : cond = (lp2 - lp1) > log(uniform); x1,lp1 <- select; n_accept[0] += sum(cond)
 * `normal` (B,3N) and `uniform` (B,) are caller-supplied noise (torch Philox on device). */
int ds_mh_propose(ds_system* sys, const void* x1, const void* normal, double width, int64_t B,
                  void* x2, void* stream);
int ds_mh_accept(ds_system* sys, void* x1, void* lp1, const void* x2, const void* lp2,
                 const void* uniform, int64_t B, void* n_accept, void* stream);

/* The reference's other proposals around the network call, per move, with caller-supplied noise (both are flagged "untested" in
 * base_config.py:122-126):
 *   mode 1: asymmetric all-electron move of qmc.mh_update with `atoms` (qmc.py:197-215): x2 = wrap(x1 + width * hmean(x1) * normal),
 *           hmean = harmonic mean of an electron's non-periodic distances to the nuclei aux (n_aux, 3) (qmc.py:44-60); the test adds
 *           the reverse / forward proposal densities (_log_prob_gaussian, qmc.py:26-42);
 *   mode 2: drift-biased move of qmc.importance_update (qmc.py:83-124): x2 = wrap(x1 + width * normal + width^2 * limdrift(grad)),
 *           aux / aux1 = grad log|psi| at x1 (B,3N), aux2 = the same at x2 (both from ds_logpsi_grad); lp <- 2 log|psi(x2)| +
 *           (|gauss|^2 - |gauss + width^2 (limdrift g1 + limdrift g2)|^2) / (2 width^2).
 *           `scratch`: 2 device elements shared by the two calls of one move -- the batch maxima of |grad| that limdrift's clip
 *           uses as its upper bound (qmc.py:78; it binds only when every drift of the batch is below the cutoff).
 * ds_mh_accept_ex takes log|psi(x2)| (B,), selects x1 / lp1 in place and increments n_accept. */
int ds_mh_propose_ex(ds_system* sys, int mode, const void* x1, const void* normal, double width, const void* aux, int n_aux,
                     int64_t B, void* x2, void* scratch, void* stream);
int ds_mh_accept_ex(ds_system* sys, int mode, void* x1, void* lp1, const void* x2, const void* logabs2, const void* uniform,
                    const void* normal, double width, const void* aux1, const void* aux2, int n_aux, int64_t B,
                    void* n_accept, void* scratch, void* stream);

/* qmc.make_mcmc_step's jitted loop (qmc.py:335-362) for the default sampler (all-electron symmetric mh_update,
 * qmc.py:153-196,217-222): `steps` moves enqueued back to back on `stream`, no host synchronisation:
 *     [lp = 2 log|psi(x)|  if !lp_valid (:357)]
 *     repeat steps times:  x2 = wrap(x + width * N(0,1));  lp2 = 2 log|psi(x2)|;
 *                          accept iff lp2 - lp > log u;  x, lp <- select;  n_accept[0] += #accepted
 * Noise: a counter-based Philox4x32-10 generator evaluated inside the kernels replaces jax.random.split / normal /
 * uniform (:190-192, :217-218): the draw for (move i, electron e | walker w) is a pure function of
 * (philox_seed, philox_offset + i, index), so runs are reproducible and ranks decorrelate by seed.  A caller
 * advances philox_offset by `steps` between calls.  Test mode: `normals` (steps, B, 3N) and `uniforms` (steps, B)
 * device arrays replay caller-supplied noise instead (both or neither).
 * x (B,3N) and lp (B,) are updated in place; n_accept (1,) of dtype is incremented (pmove = n_accept / (steps * B),
 * qmc.py:360).  Workspace: ds_mcmc_workspace_bytes(sys, B). */
int64_t ds_mcmc_workspace_bytes(const ds_system* sys, int64_t B);
int ds_mcmc_step(ds_system* sys, const void* params, void* x, void* lp, int64_t B, int steps, double width,
                 uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms,
                 int lp_valid, void* n_accept, void* ws, int64_t ws_bytes, void* stream);
/* The same loop with ONE-ELECTRON moves -- qmc.mh_one_electron_update (qmc.py:227-287) as make_mcmc_step drives it
 * (qmc.py:355-358: nsteps = N * steps, move i displaces electron i % N): move i of this call displaces electron
 * (first_electron + i) % N of every walker, wraps the whole configuration, evaluates log|psi| and selects.
 * Philox index of the displaced electron's normals = w * N + electron (the all-electron stream's index of that
 * electron); test mode: `normals` (moves, B, 3), `uniforms` (moves, B).  pmove = n_accept / (moves * B). */
int ds_mcmc_step_one_electron(ds_system* sys, const void* params, void* x, void* lp, int64_t B, int moves, int first_electron,
                              double width, uint64_t philox_seed, uint64_t philox_offset, const void* normals,
                              const void* uniforms, int lp_valid, void* n_accept, void* ws, int64_t ws_bytes, void* stream);
/* The same loop with the drift-biased importance-sampled move -- qmc.importance_update (qmc.py:83-150, symmetric branch) as
 * make_mcmc_step(importance_sampling=...) drives it: per move  g1 = grad log|psi|(x);  x2 = wrap(x + width * N + width^2 *
 * limdrift(g1));  (log|psi|, g2) at x2;  accept with the forward / reverse proposal densities (qmc.py:119-137).
 * Noise as in ds_mcmc_step: Philox (normals of electron e: index w * N + e, uniform of walker w), or explicit
 * `normals` (steps, B, 3N) / `uniforms` (steps, B).  Workspace: ds_mcmc_workspace_bytes(sys, B). */
int ds_mcmc_step_importance(ds_system* sys, const void* params, void* x, void* lp, int64_t B, int steps, double width,
                            uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms,
                            int lp_valid, void* n_accept, void* ws, int64_t ws_bytes, void* stream);
/* The same loop with the asymmetric proposal of mh_update(atoms=...) (qmc.py:197-215): the step width of an electron is
 * width x the harmonic mean of its (non-periodic) distances to `atoms` (n_atoms, 3) [device, dtype]; the forward / reverse
 * proposal densities enter the acceptance.  Noise as in ds_mcmc_step.  Workspace: ds_mcmc_workspace_bytes(sys, B). */
int ds_mcmc_step_asymmetric(ds_system* sys, const void* params, void* x, void* lp, int64_t B, int steps, double width,
                            const void* atoms, int n_atoms, uint64_t philox_seed, uint64_t philox_offset, const void* normals,
                            const void* uniforms, int lp_valid, void* n_accept, void* ws, int64_t ws_bytes, void* stream);
/* the raw Philox block ds_mcmc_step uses for (seed, offset + step, index, stream_id): host evaluation for tests
 * (stream_id 0 / 1: normal deviates of electron `index`, 2: the uniform deviate of walker `index`, 3: the shifts of
 * ds_one_body_ratios; the rotations of ds_ecp_energy, its stream 4, are stream_id 0 at offset + 2^61). */
void ds_philox_host(uint64_t seed, uint64_t offset, uint64_t step, uint64_t index, int stream_id, uint32_t out[4]);

/* One-body ratios q = psi(R') / psi(R), with R' = R except for ONE displaced electron, and the momentum distribution n(k) folded
 * from them (csrc/ds_onebody.h).  The reference has no such estimator: the conventions are this library's own.
 *   n_s(k) = < sum_{i in spin s} (1 / V) int_V ds  psi(.., r_i + s, ..) / psi(R)  exp(-i k.s) >_{|psi|^2},  V = the simulation cell,
 * for the Bloch-allowed k = k_t + n . G_S (k_t any entry of the network's klist, G_S the rows of 2 pi inv(a)^T); sum_k n_s(k) = N_s.
 *
 * One call draws M = n_samples shifts per walker:
 *   - Sample (w, m) moves electron e = (first_electron + m) % N of walker w by s; every other coordinate is copied.  R' is NOT
 *     wrapped: the Bloch phase of the network reads the unwrapped coordinates.
 *   - Philox mode (shifts == NULL): stream 3 of the generator of ds_mcmc_step.  Block A = (philox_seed, philox_offset, step 0,
 *     index 2 (w M + m)), block B = the same at index 2 (w M + m) + 1 (both are ds_philox_host(.., stream_id 3));
 *     f = (u53_co(A0, A1), u53_co(A2, A3), u53_co(B0, B1)) in [0, 1)^3 and s = f . a (rows of a = lattice vectors) in float64,
 *     products and sums rounded one by one.  A caller advances philox_offset by 1 per call.
 *   - Test mode: shifts (B, M, 3), a device array of the system's dtype, replaces the draw.
 *   - q = exp(log|psi(R')| - log|psi(R)|) phase(R') conj(phase(R)), formed in float64 from the outputs of the value chain
 *     (that of ds_logpsi: batches large enough for the int8 value layers use them here too).
 *   - nk_sums[s(e)][k] += q exp(-i k.s), s(e) = 0 if e < n_up else 1.  kvec: DEVICE array (n_k, 3) float64, Cartesian, n_k in
 *     0..512.  nk_sums: device (2, n_k, 2) float64 for either dtype, ADDED to and never zeroed; NULL iff n_k == 0.
 *   - A sample whose q is not finite (this covers a walker whose own log psi is not finite) is left out of the sums and counted
 *     per spin in n_bad (device (2,) int64, ADDED to; optional).
 *   - Normalisation is the caller's: n_s(k) = N_s sums_s(k) / (samples taken on spin s - n_bad_s).
 *   - out_ratio (B, M, 2) = (Re q, Im q) and out_shift (B, M, 3) = s: device arrays of the system's dtype, optional.
 * The call runs one forward of the B walkers, then per chunk of displaced rows: propose, value chain, accumulate, and a second
 * stage that adds the per-workgroup partials in a fixed order.  No floating-point atomics, no host synchronisation, no
 * allocation: the same input gives bit-identical sums, for ANY workspace size -- the chunk length follows from ws_bytes (at most
 * 65535 configurations; a smaller workspace means more chunks; below one group of 80 configurations it is an error), and the
 * partials are formed over fixed groups of 80 consecutive samples whatever the chunks are.
 * Refused with a ds_last_error message before any launch: B < 1, n_samples < 1, first_electron outside 0..N-1, n_k outside
 * 0..512, n_k > 0 with a NULL kvec or nk_sums, and nothing to write at all (n_k == 0 and out_ratio == NULL).
 * A cell with spin-down electrons only runs as its mirror image: its electrons count as spin 0. */
int64_t ds_one_body_workspace_bytes(const ds_system* sys, int64_t B, int n_samples);
int ds_one_body_ratios(ds_system* sys, const void* params, const void* x, int64_t B, int n_samples, int first_electron,
                       uint64_t philox_seed, uint64_t philox_offset, const void* shifts, const double* kvec, int n_k,
                       double* nk_sums, void* out_ratio, void* out_shift, int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream);

/* Spin-exchange ratios and the per-walker sums of the total-spin estimator <S^2> (csrc/ds_spin.h).  The
 * reference has no such estimator: the conventions are this library's own.
 *   Electrons 0 .. n_up-1 are spin up, the rest spin down.  P = n_up n_dn pairs.  Pair p = i n_dn + (j - n_up), with i < n_up <= j.
 *   P_p R is R with the positions of electrons i and j exchanged.  Nothing is wrapped or shifted: both positions already belong to R.
 *       q_p(R) = psi(P_p R) / psi(R)
 *       <S^2>  = S_z (S_z + 1) + n_dn - < sum_p q_p(R) >_{|psi|^2},   S_z = (n_up - n_dn) / 2
 *   The real part is the estimate.  The imaginary part vanishes in expectation.
 *   Two checks of the sign and the n_dn term: one up and one down electron in the same orbital give 0; in orthogonal orbitals
 *   they give 1.
 *   psi is antisymmetric within each spin channel, so every pair has the same expectation.  Any subset of M pairs scaled by P / M
 *   is therefore unbiased.
 *
 * One call takes M = n_pairs pairs per walker:
 *   - Sample (w, m), m < M, takes pair (first_pair + m) % P of walker w.  M may exceed P: the index wraps, as first_electron does in
 *     ds_one_body_ratios.  There is no random number in this call.
 *   - q = exp(log|psi(P R)| - log|psi(R)|) phase(P R) conj(phase(R)), formed in float64 from the outputs of the value chain (that of
 *     ds_logpsi: batches large enough for the int8 value layers use them here too).
 *   - t_w = sum_m q_{w,m}, added in an order that is a function of M alone: lane l of one wave adds m = l, l + 64, ... in order, then
 *     the 64 lane results are added in lane order.
 *   - A walker with any non-finite q among its M samples is bad: it is left out of the sums, its out_walker entry is NaN, and it is
 *     counted in n_bad (device (1,) int64, ADDED to; optional).
 *   - sums: device (4,) float64 for either dtype, ADDED to and never zeroed, optional:
 *       [ sum_w Re t_w, sum_w Im t_w, sum_w (Re t_w)^2, number of good walkers ]   over the good walkers of the call.
 *     Normalisation is the caller's: <S^2> = S_z (S_z + 1) + n_dn - (P / M) sums[0] / sums[3].
 *   - out_ratio (B, M, 2) = (Re q, Im q): device array of the system's dtype, optional.  out_walker (B, 2) = t_w: device float64,
 *     optional.
 * The call runs one forward of the B walkers, then per chunk of exchanged rows: propose, value chain, ratio; after the last chunk
 * one kernel forms the walker sums and one reduces them over the walkers in a fixed order, making ONE addition per call and entry
 * to sums.  No floating-point atomics, no host synchronisation, no allocation: the same input gives bit-identical results, a
 * second call doubles sums exactly, and ANY workspace size gives the same bits under the condition of ds_one_body_ratios (the
 * chunk length follows from ws_bytes, at most 65535 configurations; below one group of 80 configurations it is an error; the
 * value chain must pick the same kernels for the chunk lengths involved, which holds whenever no int8 value layer is in play).
 * Refused with a ds_last_error message before any launch: B < 1, n_pairs < 1, P == 0 (a fully polarised cell, the mirrored
 * (0, n) cell among them: there S^2 = S_z (S_z + 1) exactly), first_pair outside 0..P-1, and nothing to write at all (sums, out_ratio
 * and out_walker all NULL). */
int64_t ds_spin_exchange_workspace_bytes(const ds_system* sys, int64_t B, int n_pairs);
int ds_spin_exchange_ratios(ds_system* sys, const void* params, const void* x, int64_t B, int n_pairs, int first_pair,
                            double* sums, void* out_ratio, double* out_walker, int64_t* n_bad, void* ws, int64_t ws_bytes,
                            void* stream);

/* Ionic forces of a batch of walkers (csrc/ds_force.h): the Hellmann-Feynman (HF) force of the Ewald energy
 * and the Assaraf-Caffarel zero-variance (ZV) force.  The reference has no force estimator: the conventions are this library's own.
 *   Per walker and ion a of the simulation cell (A = n_atoms_sim ions, charges sim_charges):
 *       F^hf_a = -d(E_ei + E_ii)/dR_a of exactly the Ewald expressions of ds_ewald, the minimal-image choice held fixed
 *       F^zv_a = F^hf_a + dF_a,   dF_a = -1/2 lap Q_a - grad Q_a . Re grad log psi,
 *       Q_a(R) = -Z_a sum_i c(r_ia) v_ia / r_ia,   c(r) = (1 - r^2/r_c^2)^3 for r < r_c, 0 beyond,
 *       v_ia = the NEAREST image of r_i - R_a: not the minimal image of ds_ewald, which on the bcc cells (fractional wrap of a
 *       non-orthogonal lattice) and for walkers outside the cell is a longer one; the call finds it itself (csrc/ds_force.h)
 *   dF has zero expectation over |psi|^2 and removes the 1/r^2 singularity (the infinite variance) of F^hf at an all-electron
 *   nucleus.  NOT included: the Pulay term 2 <(E_L - E) d log psi / dR_a>.  HF + ZV is the force only for an exact psi; its bias is
 *   first order in the error of the wave function.  All-electron ions only: no pseudopotential term.
 *   (ds_logpsi_ion_vjp below gives d log psi / dR_a for the atoms of the primitive cell; estimator.PrimitiveForces adds the Pulay term.)
 *   - x (B, 3N) and drift (B, 3N) = Re grad log psi (the real parts of ds_logpsi_grad's out_grad): device arrays of the system's
 *     dtype.  drift is needed for out_zv and for sums, and may be NULL otherwise.  All arithmetic is float64 for either dtype.
 *   - r_c: 0 < r_c <= the Wigner-Seitz radius of the simulation cell (half its shortest lattice vector); with out_zv or sums also
 *     below the smallest plane spacing of the cell (the nearest-image search looks one cell around the wrapped difference; every
 *     reduced cell meets this with room).
 *   - ion_ion (A, 3) float64 device array, optional: the ion-ion force, a constant of the geometry, added to both outputs.
 *   - out_hf, out_zv (B, A, 3) float64, each optional.
 *   - sums: device float64 [12 A + 1], ADDED to and never zeroed, optional: per (a, c), at 4 (3 a + c),
 *       [ sum F^hf, sum (F^hf)^2, sum F^zv, sum (F^zv)^2 ]  over the good walkers of the call, then their number.
 *   - A walker with a non-finite coordinate, drift or result is bad: NaN in all its outputs, left out of sums, counted in n_bad
 *     (device (1,) int64, ADDED to; optional).
 *   - ws: needed for sums only: at least one group of 256 walkers (256 x 6 A + 12 A + 1 doubles).
 * Every addition is made in a fixed order (ds_force.h): the LDS tree over the 256 threads of a walker's workgroup, the same tree over
 * the 256 walkers of a group, the groups in order onto sums.  Groups are cut at multiples of 256 walkers of the batch whatever the
 * workspace, so the results are bit-identical from run to run and for ANY workspace size.  No floating-point atomics, no host
 * synchronisation, no allocation.
 * Refused with a ds_last_error message before any launch: a null handle or x, B < 1, nothing to write, a null drift with out_zv or
 * sums, r_c <= 0, not finite, above the Wigner-Seitz radius or (with out_zv or sums) not below the smallest plane spacing, a cell
 * with so many ions (about a thousand) that the kernel's LDS layout exceeds 64 KB, and with sums a workspace below one group. */
int64_t ds_ion_forces_workspace_bytes(const ds_system* sys, int64_t B);
int ds_ion_forces(ds_system* sys, const void* x, const void* drift, int64_t B, double r_c, const double* ion_ion, double* out_hf,
                  double* out_zv, double* sums, int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream);

/* Strain derivative of the energy of a batch of walkers (csrc/ds_stress.h): what the stress tensor and the
 * pressure are made of.  The reference has no stress estimator: the conventions are this library's own.
 *   Homogeneous strain eps (symmetric 3 x 3): every electron and ion position and every lattice vector v -> v (1 + eps), reciprocal
 *   vectors G -> G (1 + eps)^-1, V -> V (1 + tr eps).  Held fixed: alpha, the integer list of G points above the weight cut-off, and
 *   the minimal-image choice of every pair -- exactly what ds_ewald sums.  Per walker, as symmetric tensors in the component order
 *   xx, yy, zz, yz, xz, xy, in Hartree (dE / d eps; the stress is the total over the cell volume, the pressure -tr / 3 of that):
 *       kin_ab = -sum_i (Re d_ia Re d_ib + Im d_ia Im d_ib),  d = grad log psi: the integrated-by-parts kinetic tensor, -2 K_ab with
 *                <tr K> = <T>; valid under periodic and twisted boundary conditions; its variance is NOT the zero variance of E_L
 *       ee, ei = d E_ee / d eps_ab, d E_ei / d eps_ab of the Ewald expressions of ds_ewald: the real-space sums over the same pairs
 *                and 27 images with q f'(r) v_a v_b / r, f'(r) = -[erfc(alpha r) / r^2 + (2 alpha / sqrt pi) exp(-alpha^2 r^2) / r]; the
 *                reciprocal sums with dw_G = w_G [-delta_ab + 2 G_a G_b (1 / G^2 + 1 / (4 alpha^2))] at unchanged phases; and the
 *                constants, d ijconst = -ijconst delta_ab.  They go as 1 / r at a nucleus, like the potential energy: finite variance
 *       total  = kin + ee + ei + ion_ion
 *   kin + Ewald is the strain derivative of the energy only for an exact psi: for a variational psi the energy also changes because
 *   psi at fixed parameters changes with the cell; that term is not evaluated.  All-electron ions only: no pseudopotential term.
 *   - x (B, 3N): device array of the system's dtype.  grad (B, 3N, 2) = (Re, Im) of grad log psi as ds_logpsi_grad writes out_grad,
 *     the system's dtype; NULL leaves the kinetic row zero (total is then the Ewald part alone) and is refused with sums.  All
 *     arithmetic is float64 for either dtype.
 *   - ion_ion: 6 float64 on the device, optional: d E_ii / d eps, a constant of the geometry, added to the total row.
 *   - out (B, 4, 6) float64, optional: the rows kin, ee, ei, total.
 *   - sums: device float64 [2 x 4 x 6 + 1], ADDED to and never zeroed, optional: per row and component, at 2 (6 row + component),
 *       [ sum, sum of squares ]  over the good walkers of the call, then their number.
 *   - A walker with a non-finite coordinate, gradient or result is bad: NaN in all its outputs, left out of sums, counted in n_bad
 *     (device (1,) int64, ADDED to; optional).
 *   - ws: needed for sums only: at least one group of 256 walkers (256 x 24 + 49 doubles).
 * Every addition is made in a fixed order (ds_stress.h): per thread its G points, pairs and electrons in order, the LDS tree over the
 * 256 threads of a walker's workgroup, the same tree over the 256 walkers of a group, the groups in order onto sums.  Groups are cut
 * at multiples of 256 walkers of the batch whatever the workspace, so the results are bit-identical from run to run and for ANY
 * workspace size.  No floating-point atomics, no host synchronisation, no allocation.
 * Refused with a ds_last_error message before any launch: a null handle or x, B < 1, nothing to write (out and sums both NULL), sums
 * without grad, with sums a workspace below one group, and a kernel LDS layout above 64 KB (no handle the library creates reaches
 * it: the layout without phase tables is 49.6 KB at the largest N = 128). */
int64_t ds_stress_workspace_bytes(const ds_system* sys, int64_t B);
int ds_stress(ds_system* sys, const void* x, const void* grad, int64_t B, const double* ion_ion, double* out, double* sums,
              int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream);

/* Gradient of log psi in the ion positions, per walker (csrc/ds_iongrad.h): the primitive of the Pulay force
 *   F_a = sum_{s image of a} F^zv_s - 2 Re < conj(E_L - E) (O_a - <O_a>) >,   O_a = d log psi / d R_a = d log|psi| + i d arg psi,
 * which completes ds_ion_forces (estimator.PrimitiveForces).  E_L = ke + ewald is complex as ds_local_energy returns it: for a complex
 * psi the term 2 <Im E_L d arg psi> belongs to the force.
 *   out[b][a][c] = d/dR_{a,c} [ cot[b][0] log|psi_b| + cot[b][1] arg psi_b ]     PER WALKER (not summed over the batch)
 * a runs over the A = n_atoms_prim atoms of the PRIMITIVE cell (`atoms`), the only ions psi sees: its features are
 * f(wrap(r_i) - R_a), periodic in the primitive lattice, so moving atom a moves all its images in the simulation cell together.
 * The derivative in a single ion of a supercell does not exist in this ansatz; what the call gives is the force on each primitive
 * atom per simulation cell (q = 0).  The ions of the simulation cell are ordered atom-major (image s belongs to atom s / scale).
 *   - cot (B, 2) of the system's dtype, the convention of ds_logpsi_vjp; out (B, A, 3) FLOAT64 for either dtype, overwritten;
 *     out_logabs (B,) / out_phase (B, 2) optional, as in ds_logpsi_vjp.
 *   - The forward and the seed are ds_logpsi_vjp's, and so is the one-electron cotangent chain down to layer 0; nothing that only
 *     forms a parameter sum is launched and the pair-stream backward is left out (the pair stream does not depend on R).
 *     k_ion_grad then contracts the cotangent of the input features and of the envelope with d f / d o in float64.
 *   - Every network option of ds_system_desc runs.  All-electron ions only.  Large batches inherit the value chain's int8 split of
 *     the residual hidden layers exactly as ds_logpsi_vjp does (float64 handles, DS_NO_I8_VAL unset).
 *   - Every addition is made in a fixed order and chunks are cut at groups of 80 walkers: bit-identical from run to run and for any
 *     workspace size.  No floating-point atomics.
 * Refused with a ds_last_error message before any launch: a null handle, params, x, cot, out or ws, B < 1, a workspace below one
 * group of 80 walkers (ds_ion_vjp_workspace_bytes(sys, 1)). */
int64_t ds_ion_vjp_workspace_bytes(const ds_system* sys, int64_t B);
int ds_logpsi_ion_vjp(ds_system* sys, const void* params, const void* x, int64_t B, const void* cot, double* out, void* out_logabs,
                      void* out_phase, void* ws, int64_t ws_bytes, void* stream);

/* Semi-local pseudopotential (ECP) energy of a batch of walkers (csrc/ds_ecp.h).  The reference has no
 * pseudopotentials: the conventions are this library's own.
 *
 * Potential.  Each atom I of the simulation cell has a species.  A species has a local radial function v_loc and n_l in 0..4
 * non-local channels v_l, l = 0 .. n_l-1.  Every radial function has the form
 *       v(r) = sum_k c_k r^(n_k - 2) exp(-zeta_k r^2),   n_k in {0, 1, 2, 3, 4},   at most 16 terms
 *   - This is the Gaussian expansion in which ccECP, BFD and Stuttgart potentials are published.
 *   - v_loc is the local part WITHOUT the -Z_eff / r tail.  Ewald carries that tail.
 *   - The caller's cell already has the valence electron count in nelec and Z_eff in atom_charges().
 *
 * Cutoffs.  Each species has two cutoffs: r_cut_loc and r_cut_nl, the latter one value for all of its channels.
 *   - Inside the cutoff the function is used as it is.  Outside it is exactly 0.  Nothing is smoothed.
 *   - Every cutoff must be <= half the smallest height of the simulation cell, where height c = 1 / ||column c of inv(a)||.
 *     Creation refuses a larger cutoff with a message that names the atom, the cutoff and the limit.
 *   Under the height condition exactly one periodic image of an ion can lie inside the cutoff.  It is the one with all fractional
 *   components in [-1/2, 1/2):
 *       f = (r_i - R_I) . inv(a);   f <- f - floor(f + 1/2);   d = f . a;   r = |d|;   dhat = d / r   (dhat = z if r = 0)
 *   (r >= |f_c| height_c for each c, so r below half the smallest height forces every |f_c| < 1/2: csrc/ds_ecp.h has the proof.)
 *
 * Energy of walker w.
 *       E_loc(w) = sum_i sum_I [r_iI < r_cut_loc,I] v_loc,I(r_iI)
 *       E_nl(w)  = sum_{(i,I): r_iI < r_cut_nl,I}  sum_{q < N_q} (1 / N_q) W_iIq psi(R'_iIq) / psi(R)
 *       W_iIq    = sum_l (2l + 1) v_I,l(r_iI) P_l(U_q . dhat_iI)
 *       R'_iIq   = R with r_i replaced by r_i - d_iI + r_iI U_q
 *   - R' is not wrapped, as in ds_one_body_ratios.
 *   - E_loc is real and E_nl is complex.
 *   - The total to add to E_L is E_loc + E_nl.
 *
 * Quadrature.  N_q in {6, 12}, with equal weights.  U_q = Rot_w u_q.
 *   - Octahedron, exact to degree 3: +x, -x, +y, -y, +z, -z.
 *   - Icosahedron, exact to degree 5.  Let phi = (1 + sqrt 5) / 2 and n = sqrt(1 + phi^2).  For (s1, s2) in the order
 *     (+,+), (+,-), (-,+), (-,-), take all four of (0, s1, s2 phi) / n, then all four of (s1, s2 phi, 0) / n, then all four of
 *     (s2 phi, 0, s1) / n.
 *   - Creation refuses n_l such that 2 (n_l - 1) exceeds the degree of the rule.  That is l <= 1 with 6 points and l <= 2 with 12.
 *     It refuses l = 3 altogether with these two rules.  n_l up to 3 is therefore what runs, and the n_l <= 4 of the table format
 *     is reserved.
 *
 * Rotation.  There is one rotation per walker and call.  It is a pure function of (seed, offset, w).
 *   - It uses Philox stream 4.  Streams 0-3 are taken.  The stream number of ds_philox_host fills the two top bits of the fourth
 *     counter word, which hold 0..3; stream 4 is stream number 0 with bit 29 of that word set, i.e. the block
 *     ds_philox_host(seed, offset + 2^61, step, index, 0).  philox_offset must stay below 2^61.
 *   - Block A is at index 2w and block B at index 2w + 1, with counter philox_offset and step 0.
 *   - u1 = u53_co(A0, A1), u2 = u53_co(A2, A3), u3 = u53_co(B0, B1).
 *   - The quaternion follows Shoemake: (x, y, z, w) = (sqrt(1 - u1) sin 2 pi u2, sqrt(1 - u1) cos 2 pi u2, sqrt(u1) sin 2 pi u3,
 *     sqrt(u1) cos 2 pi u3).  The matrix is the standard one of a unit quaternion, in float64 (its factor 2 is taken as
 *     2 / |quaternion|^2, so that the rounding of the norm does not enter the orthogonality).
 *   - Test mode takes caller-supplied rotations (B, 3, 3) in float64 [device, row-major].
 *   - The caller advances the offset by 1 per call.
 *
 * Arithmetic.
 *   - Distances, radial functions, Legendre polynomials and weights are float64 for either dtype, computed from the walker
 *     coordinates as stored.  A float32 system reads float32 positions and widens them.
 *   - q = exp(log|psi(R')| - log|psi(R)|) phase(R') conj(phase(R)) in float64 from the value chain's outputs, as in
 *     ds_one_body_ratios.
 *
 * Pair order.  Pairs are ordered by (w, i, I) and configurations by (pair, q).  That order fixes every sum.
 *
 * Non-finite input.
 *   - A walker with a non-finite coordinate gets NaN in all three of its outputs and contributes no pair.
 *   - A non-finite ratio makes that walker's E_nl non-finite and nothing else.  It shows up in n_nonfinite of ds_energy_stats as
 *     any non-finite E_L does.
 *   - There is no n_bad.
 *
 * The descriptor holds HOST arrays that ds_ecp_create copies: the cell a (rows = lattice vectors, Bohr); atoms (n_atoms, 3) of the
 * SIMULATION cell and atom_species (n_atoms,); per species n_l, r_cut_loc, r_cut_nl (n_species,); the term tables term_n / term_zeta
 * / term_c of all radial functions back to back, with term_offset (5 n_species + 1,): slot 5 s is v_loc of species s, slot 5 s + 1
 * + l its v_l, and the terms of slot j are term_offset[j] .. term_offset[j + 1] - 1; n_quad.
 * ds_ecp_create refuses, before it touches the device: n_quad other than 6 or 12, n_l outside 0..4 or beyond the rule (above), more
 * than 16 terms in a function, n_k outside 0..4, non-finite entries, an atom_species outside the species, and a cutoff beyond half
 * the smallest height.
 *
 * ds_ecp_energy, one call:
 *   1. per walker: the rotation, the minimum image of every (i, I), E_loc added in (i, I) order, the pairs inside r_cut_nl counted;
 *   2. an exclusive scan of the counts over the walkers, and the pair records (w, i, I, r, dhat, v_l(r)) at their offsets;
 *   3. the pair total is read back: ONE 8-byte copy and ONE stream synchronisation, the only synchronisation of the call.  The
 *      call therefore CANNOT be captured into a graph.  A total above pair_capacity fails the call before any forward; the message
 *      carries the number needed ("... the walkers have <n> pairs ...");
 *   4. one forward of the B walkers (none when there is no pair), then per chunk of a whole number of 80-configuration groups --
 *      the chunk length follows from ws_bytes as in ds_one_body_ratios, at most 65535 configurations -- propose, value chain (that
 *      of ds_logpsi), and the term (W / N_q) q of every configuration in float64 into the workspace (q into out_ratio on request);
 *   5. per walker, one wave: lane l adds the walker's terms l, l + 64, ... in order, then lane 0 adds the 64 results in lane order.
 * out_energy (B, 3) float64 = (E_loc, Re E_nl, Im E_nl), written by step 5 only; out_pairs (B,) int64: pairs per walker;
 * out_ratio (pair_capacity N_q, 2) of the system's dtype: q of configuration pair * N_q + q; out_rotation (B, 3, 3) float64: all
 * device arrays, the last three optional.  No floating-point atomics, no allocation, 64-bit indices; results are bit-identical
 * from run to run and for ANY workspace size under the condition of ds_spin_exchange_ratios (the value chain must pick the same
 * kernels for the chunk lengths involved).
 * Refused with a ds_last_error message before any launch: B < 1, out_energy NULL, pair_capacity < 1, a workspace below one group
 * ("workspace too small"), and a descriptor whose cell or atom count differs from the system's. */
typedef struct ds_ecp ds_ecp;
typedef struct ds_ecp_desc {
    double a[9];
    int32_t n_atoms;
    const double* atoms;
    const int32_t* atom_species;
    int32_t n_species;
    const int32_t* n_l;
    const double* r_cut_loc;
    const double* r_cut_nl;
    const int32_t* term_offset;
    const int32_t* term_n;
    const double* term_zeta;
    const double* term_c;
    int32_t n_quad;
} ds_ecp_desc;
int ds_ecp_create(const ds_ecp_desc* desc, ds_ecp** out);
void ds_ecp_destroy(ds_ecp* ecp);
int64_t ds_ecp_workspace_bytes(const ds_system* sys, const ds_ecp* ecp, int64_t B, int64_t pair_capacity);
int ds_ecp_energy(ds_system* sys, const ds_ecp* ecp, const void* params, const void* x, int64_t B, uint64_t philox_seed,
                  uint64_t philox_offset, const double* rotations, int64_t pair_capacity, double* out_energy, int64_t* out_pairs,
                  void* out_ratio, double* out_rotation, void* ws, int64_t ws_bytes, void* stream);

/* Ionic forces of the semi-local pseudopotential (csrc/ds_ecp_force.h): minus the derivative of the
 * E_loc + E_nl of ds_ecp_energy in the position of every ion of the simulation cell, per walker.  Every convention of ds_ecp_energy
 * holds: the potential, the cutoffs, the minimum image, the two rules, the pair order.
 *
 * Estimator.  Per pair p = (w, i, I) inside r_cut_nl:
 *       d = the minimum image of r_i - R_I,  r = |d|,  dhat = d / r;   U_q = Rot_w u_q;   c_q = U_q . dhat;
 *       W_q = sum_l (2l + 1) v_l(r) P_l(c_q);   R'_q = R with r_i replaced by r_i - d + r U_q;   rho_q = psi(R'_q) / psi(R);
 *       g_q = the three complex components of electron i of grad log psi at R'_q (Re = grad log|psi|, Im = grad arg psi, as
 *             ds_logpsi_grad writes them).
 *   The derivative is taken with psi held fixed as a function of the electron coordinates; the rotation of the call, the electron
 *   positions and the image choice are held fixed too.  With d d / d R_I = -1 and d r'_a / d R_b = delta_ab - U_qa dhat_b:
 *       F^loc_I(w) = sum_i [r_iI < r_cut_loc,I]  v'_loc,I(r) dhat
 *       F^nl_I(w)  = sum_{i: r_iI < r_cut_nl,I} sum_q (1 / N_q) rho_q { sum_l (2l + 1) [ v'_l(r) P_l(c_q) dhat
 *                                                                                       + v_l(r) P'_l(c_q) (U_q - c_q dhat) / r ]
 *                                                                     - W_q ( g_q - (g_q . U_q) dhat ) }
 *       v'(r) = sum_k c_k [ (n_k - 2) r^(n_k - 3) - 2 zeta_k r^(n_k - 1) ] exp(-zeta_k r^2)
 *   - F^loc is real, F^nl complex.  An estimator uses F^pp = F^loc + Re F^nl; Im F^nl vanishes in expectation for a psi of fixed
 *     phase.
 *   - The radial functions are exactly 0 outside their cutoffs.  The jump at a cutoff is a delta term of the exact derivative and is
 *     LEFT OUT; its size is that of the function at its cutoff.
 *   - This is the Hellmann-Feynman part only: no Pulay term (E_pp is not part of the E_L of ds_logpsi_ion_vjp's estimator), no
 *     zero-variance term.  Its bias is first order in the error of psi.  The Ewald force of the Z_eff ions is ds_ion_forces' out_hf.
 *
 * Rotation.  Philox stream 4 with the offset rule of ds_ecp_energy, or caller-supplied rotations: a force call and an energy call
 * with the same (philox_seed, philox_offset) use the same points.
 *
 * ds_ecp_forces, one call:
 *   1. steps 1-3 of ds_ecp_energy with its kernels: rotation, counts, offsets, pair records, and the pair total read back: ONE 8-byte
 *      copy and ONE stream synchronisation, the only one of the call.  The call therefore CANNOT be captured into a graph.  A total
 *      above pair_capacity fails the call before any chain pass, with ds_ecp_energy's message ("... the walkers have <n> pairs ...");
 *   2. per walker F^loc: for every ion the electrons added in order i = 0 .. N-1; per pair the second record v'_l(r);
 *   3. log psi(R): ONE pass of the forward-Laplacian chain with the gradient output (that of ds_logpsi_grad) over the B walkers (none
 *      when there is no pair).  The ratios take this log|psi(R)| and phase(R), not the value chain's, so that numerator and
 *      denominator come from the same arithmetic;
 *   4. per chunk of a whole number of 80-configuration groups -- the chunk length follows from ws_bytes with the chain's per-walker
 *      layout, at most 65535 configurations -- propose (ds_ecp_energy's rows), the same chain, and per configuration the complex
 *      3-vector (rho_q / N_q) { ... } in float64 into the workspace.  A walker without a pair costs no chain work beyond step 3;
 *   5. per walker one workgroup: for every ion, lane l of a wave adds the terms of the walker's configurations l, l + 64, ... in
 *      order whose pair belongs to the ion, then the 64 lane results through the fixed tree (l += l + s, s = 32 .. 1);
 *   6. with sums: k_force_part / k_force_final of ds_ion_forces on the rows (F^pp, F^tot): the tree over the 256 walkers of a group,
 *      the groups in order onto sums.  Groups are cut at multiples of 256 walkers of the batch whatever the workspace.
 *   - base (B, A, 3) float64, optional: added per walker, F^tot = F^pp + base; without it F^tot = F^pp.  It is meant for out_hf of
 *     ds_ion_forces (the Ewald force with Z_eff, ion-ion force included); a base of another meaning cannot be detected and is the
 *     caller's responsibility.
 *   - out_force (B, A, 3, 3) float64, optional: last index = (F^loc, Re F^nl, Im F^nl).
 *   - sums: device float64 [12 A + 1], ADDED to and never zeroed, optional: the layout of ds_ion_forces: per (a, c), at 4 (3 a + c),
 *       [ sum F^pp, sum (F^pp)^2, sum F^tot, sum (F^tot)^2 ]  over the good walkers of the call, then their number.
 *   - A walker with a non-finite coordinate, with a pair at r = 0 inside a cutoff (it has no dhat), or with a non-finite result
 *     (base included) is bad: NaN in all its outputs, left out of sums, counted in n_bad (device (1,) int64, ADDED to; optional).
 *   - out_pairs (B,) int64 and out_rotation (B, 3, 3) float64 as in ds_ecp_energy, optional.
 * The chain is per-walker bit-independent of the batch it runs in and the order of every addition is a function of the walker's pair
 * list (and, for sums, of B) alone: results are bit-identical from run to run and for ANY workspace size.  No floating-point
 * atomics, no allocation, 64-bit indices.  Geometry, radial functions and Legendre polynomials are float64 for either dtype; products
 * and sums are rounded one by one.
 * Cost: one forward-Laplacian chain evaluation per quadrature configuration (EXPERIMENTS.md has the measured ratio to ds_ecp_energy).
 * Refused with a ds_last_error message before any launch: a null handle, descriptor, params, x or ws; out_force and sums both NULL
 * (nothing to write); everything ds_ecp_energy refuses of (B, pair_capacity, descriptor); a workspace below one group ("workspace too
 * small"), with or without sums. */
int64_t ds_ecp_forces_workspace_bytes(const ds_system* sys, const ds_ecp* ecp, int64_t B, int64_t pair_capacity);
int ds_ecp_forces(ds_system* sys, const ds_ecp* ecp, const void* params, const void* x, int64_t B, uint64_t philox_seed,
                  uint64_t philox_offset, const double* rotations, int64_t pair_capacity, const double* base, double* out_force,
                  double* sums, int64_t* n_bad, int64_t* out_pairs, double* out_rotation, void* ws, int64_t ws_bytes, void* stream);

/* Fixed-phase diffusion Monte Carlo (csrc/ds_dmc.h): all-electron drift-diffusion move, Metropolis
 * acceptance, symmetric branching weights, energy cut-off, fixed-population comb.  The reference has no DMC: the conventions are
 * this library's own.  One call runs a block of `steps` steps with no host synchronisation and no allocation.
 *
 * Walker state.  Caller-owned device buffers, T = the system's dtype:
 *       x (B, 3N) T        walker coordinates
 *       logabs (B,) T      log|psi|
 *       phase (B, 2) T     (Re, Im) of the unit phase
 *       drift (B, 3N) T    Re grad log psi
 *       eloc (B,) float64  Re E_kin + E_ewald
 *       weight (B,) float64  branching weight, >= 0
 *   With state_valid = 0 the call first fills logabs, phase, drift and eloc from x by one chain pass plus Ewald.  Weights are not
 *   touched, except that a walker whose log|psi| or E_L is not finite gets weight 0.
 *
 * Step i of a call, with tau, tau_eff, e_trial, e_ref, e_cut, node_mode:
 *   1. Limited drift per electron: vbar_e = v_e * 2 / (1 + sqrt(1 + 2 |v_e|^2 tau)).  This is the Umrigar-Nightingale-Runge limiter
 *      with a = 1, written in the form that has no cancellation.  It is NOT qmc.limdrift (the clip by the batch maximum that
 *      ds_mcmc_step_importance uses): it needs nothing from the other walkers.
 *   2. Proposal: x' = wrap(x + tau vbar + sqrt(tau) chi).  chi is the samplers' normals: streams 0 and 1, index w N + e, counter
 *      philox_offset + i, rounded to T.  Wrap as ds_mh_propose_ex does.
 *   3. One chain pass at x' with both outputs (kinetic energy and walker gradient), plus the Ewald kernel: log|psi'|, phase',
 *      grad', ke'.  E' = Re ke' + ewald' in float64 (the Ewald triple summed in T as ds_local_energy sums it).
 *   4. Log ratio: A = 2 (log|psi'| - log|psi|) + 1/2 (|chi|^2 - |chi + sqrt(tau) (vbar + vbar')|^2), float64.  It is built from chi
 *      and the drifts, never from wrapped position differences, as mode 2 of ds_mh_accept_ex does.  Accept iff all of: A and E'
 *      are finite; A > log u, u = stream 2 at index w; node_mode == 0 or Re(phase' conj(phase)) > 0.  node_mode = 1 is fixed-node
 *      for real wavefunctions: a sign change is a node crossing.  p = min(1, e^A), and p = 0 for a move refused as non-finite or
 *      node-crossing.
 *   5. Weight update, all float64: E_new = E' if accepted else E;
 *        weight <- weight * exp(-tau_eff (1/2 (clip(E_new) + clip(E)) - e_trial)),  clip(e) = e_ref + clamp(e - e_ref, +-e_cut);
 *      e_cut <= 0 switches the clip off.  A weight that comes out not finite (the walker's energy is not finite) becomes 0.
 *   6. x, logabs, phase, drift and eloc are selected in place.
 *   7. One row of out_stats (steps, 9) float64, taken after the weight update and before branching:
 *        [0] sum w   [1] sum w E (unclipped)   [2] sum w E^2   [3] number accepted   [4] sum p   [5] number of walkers whose E_new
 *        was clipped   [6] number of non-finite proposals   [7] sum w^2   [8] distinct parents of this step's comb (B if the step
 *        has none, 0 if its comb was skipped).
 *      A walker of weight 0 adds nothing to [1] and [2] (its energy may be NaN).  Fixed order, no floating-point atomics: one row of
 *      partials per 256 consecutive walkers (thread t holds walker t; a tree adds t and t + s for s = 128, 64, .., 1), then the
 *      rows are added in order.
 *   8. If branch_every > 0 and (i + 1) % branch_every == 0, the comb:
 *        xi = the stream-2 uniform at index B (one past the walkers), counter philox_offset + i.
 *        C = inclusive prefix sums of the weights in this order: chunk c holds walkers 256 c .. 256 c + 255; inside a chunk
 *          r_0 = w_first, r_i = r_{i-1} + w_i; chunk offsets O_0 = 0, O_c = O_{c-1} + r_last(c-1); C_j = O_c + r_i.  Every sum is
 *          one rounded float64 addition.  W = C_{B-1}.
 *        Tooth k = (k + xi) (W/B), taken as its two products k (W/B) and xi (W/B), each rounded on its own:
 *          parent of k = number of j with (C_j - k (W/B)) <= xi (W/B), the difference rounded too, clamped to the last walker of
 *          positive weight (= the number of j with C_j < W; B - 1 unless the batch ends in dead walkers, which a tooth that
 *          rounding puts on the last edge must not revive).
 *          (A single rounded (k + xi) (W/B) would round xi = 1 - 2^-53 up to the next edge; in this form equal weights give the
 *          identity for every xi in [0, 1).)
 *        All state arrays are gathered from the parents and every weight becomes W/B.  A total W that is not finite or not
 *        positive skips the comb: the state stays, the parents are the identity and entry [8] of the row is 0.
 *      The comb keeps sum w, so the library has no trial-energy feedback of its own: e_trial only keeps W in range and the host
 *      moves it between calls.  Ranks comb their own populations.
 * Noise.  Philox as above, or explicit: normals (steps, B, 3N) and uniforms (steps, B) of dtype T and comb_uniforms (steps,)
 * float64, all three or none.  A caller advances philox_offset by `steps` between calls; `steps` steps in one call and `steps`
 * calls of one step with the offset advanced and state_valid = 1 give the same bits when branch_every is 0 or 1.
 * out_parents (steps, B) int32, optional: the parents of every step (the identity for a step without a comb).
 * The chain is chunked by ws_bytes as ds_logpsi_grad chunks it; results are bit-identical from run to run and for any workspace
 * size under the condition of ds_spin_exchange_ratios (the chain picks the same kernels for the chunk lengths involved).
 * Refused with a ds_last_error message before any launch: null state pointers or out_stats; B < 1 or B > 2^20 (the chunk offsets
 * of the scan are kept in one workgroup's LDS); steps < 1; tau <= 0, tau_eff < 0 or a non-finite scalar; node_mode outside
 * {0, 1}; branch_every < 0; noise arrays given in part; a workspace below one chain chunk ("workspace too small").
 * Out of scope: a pseudopotential in ds_dmc_step itself (it takes no ds_ecp and adds no ECP term: ds_dmc_step_ecp below is the
 * locality approximation, ds_dmc_step_tmove below it adds T-moves), electron-by-electron moves, cross-rank walker exchange
 * (ranks keep fixed populations with their own total weights, which is unbiased).  Forward walking and the weighted estimators
 * built on out_parents: ds_dmc_ancestry, ds_realspace_counts_w and ds_dmc_fw_sums below.
 *
 * ds_dmc_branch is the comb of step 8 alone with a given xi in [0, 1); it needs no handle (dtype: 0 float64, else float32) and is
 * the code ds_dmc_step runs.  Workspace: ds_dmc_branch_workspace_bytes.  The caller's buffers may alias nothing else. */
int64_t ds_dmc_workspace_bytes(const ds_system* sys, int64_t B);
int ds_dmc_step(ds_system* sys, const void* params, void* x, void* logabs, void* phase, void* drift, double* eloc, double* weight,
                int64_t B, int steps, double tau, double tau_eff, double e_trial, double e_ref, double e_cut, int node_mode,
                int branch_every, uint64_t philox_seed, uint64_t philox_offset, const void* normals, const void* uniforms,
                const double* comb_uniforms, int state_valid, double* out_stats, int32_t* out_parents, void* ws, int64_t ws_bytes,
                void* stream);
/* DMC with a semi-local pseudopotential in the LOCALITY APPROXIMATION: the branching energy is
 *   E = ((Re E_kin + E_ewald) + E_loc) + Re E_nl,
 * with E_loc and E_nl projected on the trial function exactly as ds_ecp_energy defines them.  T-moves: ds_dmc_step_tmove below
 * (DESIGN.md section 19.2).
 * ds_dmc_step_ecp takes every argument of ds_dmc_step, plus:
 *   ecp             the descriptor's handle (ds_ecp_create)
 *   pair_capacity   as in ds_ecp_energy, for ONE evaluation (all B walkers at one position each)
 *   rotations       NULL, or (steps + 1, B, 3, 3) float64 [device]: slot 0 is for the initialisation (ignored when state_valid = 1),
 *                   slot i + 1 for step i
 *   epp             caller-owned state, (B, 3) float64 = (E_loc, Re E_nl, Im E_nl) at the walker's current position: the SEVENTH
 *                   state array
 *   out_ecp_stats   NULL, or (steps, 3) float64 [device]: per step sum w E_loc, sum w Re E_nl, sum w Im E_nl over the walkers of
 *                   non-zero weight, taken at the same point as the out_stats row (after the weight update, before the comb) and in
 *                   the same fixed order: partials per 256 consecutive walkers, then one pass in row order.  No floating-point atomics
 *   out_pairs       NULL, or (steps + 1,) int64 [device]: the pair total of the initialisation (entry 0, untouched when
 *                   state_valid = 1) and of every step's evaluation (entry i + 1)
 *   steps_done      host pointer, may be NULL: receives the number of completed steps
 * The algorithm is that of ds_dmc_step word for word, with three changes.
 *   Initialisation (state_valid = 0).  The pseudopotential is evaluated at x exactly as ds_ecp_energy(x, philox_seed,
 *     philox_offset) evaluates it.  eloc = ((what ds_dmc_step's initialisation computes) + E_loc) + Re E_nl, each addition rounded
 *     in float64, in that order; epp is the triple.  A walker whose total is not finite gets weight 0.
 *   Step i.  After the chain pass at x' the pseudopotential is evaluated at x' exactly as ds_ecp_energy(x', philox_seed,
 *     philox_offset + 1 + i) evaluates it, and E' = ((Re ke' + ewald') + E_loc') + Re E_nl' in float64.  Everything downstream
 *     (the finiteness test of step 4, the clip, the symmetric weight, the stats row, the comb) sees only E' and eloc.  A
 *     non-finite ratio makes E' non-finite: the move is refused as non-finite and counted in column [6].  epp is selected with
 *     the other rows on acceptance.
 *   Comb.  epp is gathered from the same parents by one small kernel after the comb's own; a skipped comb leaves it untouched.
 * The pseudopotential term never passes through the system's element type: the float64 triple goes to the acceptance kernel as it is.
 * Rotations: Philox stream 4 of ds_ecp_energy with the counter philox_offset for the initialisation and philox_offset + 1 + i for
 * step i (the move's noise is on streams 0-2).  With these counters `steps` steps in one call equal `steps` calls of one step
 * with the offset advanced.  The explicit inputs (normals, uniforms, comb_uniforms, rotations) come all together or not at all.
 * SYNCHRONISATION.  Every pseudopotential evaluation keeps ds_ecp_energy's one 8-byte read-back of the pair total: a call
 * synchronises the stream `steps` times, plus once for an initialisation, and CANNOT be captured into a graph.
 * Capacity.  The pair total of step i is checked before that step's acceptance kernel.  A total above pair_capacity fails the call
 * with ds_ecp_energy's message, which carries the number needed; *steps_done is then the number of completed steps, the state
 * is exactly that after those steps, and the out_stats rows of the completed steps are valid.  An overflow at the initialisation
 * leaves all seven arrays untouched.
 * Workspace: ds_dmc_ecp_workspace_bytes = the layout of ds_dmc_step followed by that of ds_ecp_energy for (B, pair_capacity).  A
 * smaller one is split so: beside ONE chain walker the pseudopotential keeps room for up to 64 groups of 80 configurations (what
 * ds_ecp_workspace_bytes provides at most); the chain's chunk then takes what fits; the groups follow from what is left, as
 * ds_ecp_energy derives them.  Results are bit-identical for any split under the condition of ds_dmc_step and
 * ds_ecp_energy.  The in-step evaluation is bit-identical to a ds_ecp_energy call on the same array with the same counter.
 * Refused with a ds_last_error message before any launch: everything ds_dmc_step refuses; everything ds_ecp_energy refuses of a
 * descriptor (NULL, atom count or cell differing from the system's) and pair_capacity < 1; epp NULL; philox_offset + steps >= 2^61;
 * explicit inputs given in part; a workspace below one chain walker plus one 80-configuration group ("workspace too small").
 * ds_dmc_step, ds_dmc_branch, ds_dmc_noise and ds_ecp_energy are unchanged.  ds_dmc_branch knows no epp: a caller gathers it from
 * the parents that call returns. */
int64_t ds_dmc_ecp_workspace_bytes(const ds_system* sys, const ds_ecp* ecp, int64_t B, int64_t pair_capacity);
int ds_dmc_step_ecp(ds_system* sys, const ds_ecp* ecp, const void* params, void* x, void* logabs, void* phase, void* drift,
                    double* eloc, double* weight, double* epp, int64_t B, int steps, double tau, double tau_eff, double e_trial,
                    double e_ref, double e_cut, int node_mode, int branch_every, uint64_t philox_seed, uint64_t philox_offset,
                    const void* normals, const void* uniforms, const double* comb_uniforms, const double* rotations,
                    int64_t pair_capacity, int state_valid, double* out_stats, double* out_ecp_stats, int32_t* out_parents,
                    int64_t* out_pairs, int* steps_done, void* ws, int64_t ws_bytes, void* stream);
/* DMC with a semi-local pseudopotential and T-MOVES (Casula, Phys. Rev. B 74, 161102 (2006)): the terms of
 * E_nl with a negative real part become heat-bath moves of one electron to a quadrature point, so that the mixed energy is an upper
 * bound.  The pseudopotential is evaluated AFTER the accept/reject decision, at the position the walker then has: a rejected
 * walker is evaluated where it stands, the term list is used within the step and discarded, and a step costs one pseudopotential
 * evaluation, as in ds_dmc_step_ecp, plus one more chain pass.  The price is Casula's one-point branching weight.
 * ds_dmc_step_tmove takes every argument of ds_dmc_step_ecp, with these differences:
 *   tmove_uniforms  NULL, or (steps, B) float64 [device]: joins the explicit inputs (normals, uniforms, comb_uniforms, rotations,
 *                   tmove_uniforms), which come all together or not at all
 *   rotations       NULL, or (steps, B, 3, 3) float64 [device]: slot i for step i (the initialisation evaluates no pseudopotential)
 *   out_ecp_stats   NULL, or (steps, 4) float64 [device]: the three columns of ds_dmc_step_ecp and the number of walkers that made
 *                   a T-move in the step (an exact count)
 *   out_pairs       NULL, or (steps,) int64 [device]: the pair total of every step's evaluation
 *   out_tmove       NULL, or (steps, B) int32 [device]: the walker-local configuration pair_local * N_q + q of the move taken (pairs
 *                   of the walker in (i, I) order, as ds_ecp_energy orders them), or -1 for none
 *   out_energy      NULL, or (steps, B) float64 [device]: E of step 5 below for every walker
 * State: the seven arrays of ds_dmc_step_ecp with these meanings:
 *   eloc = Re E_kin + E_ewald at the walker's CURRENT position (the meaning it has in ds_dmc_step: without the pseudopotential);
 *   epp  = (E_loc, Re E_nl, Im E_nl) of the walker's LAST EVALUATION, that is at its position before its T-move.  It is reported
 *          only and never an input.
 * With state_valid = 0 the call does exactly what ds_dmc_step's initialisation does, and sets epp to 0.
 * Step i of a call:
 *   1. Limited drift and proposal: steps 1 and 2 of ds_dmc_step, with the same kernels.
 *   2. One chain pass at x' with both outputs, plus Ewald.  E_c' = Re ke' + ewald' in float64, as ds_dmc_step forms E'.
 *   3. Decision: step 4 of ds_dmc_step with "E' finite" read as "E_c' finite".  Nothing is committed yet: the decision, p and the
 *      flags go to the workspace, and the selected position x_cur (x' if accepted, else x) is gathered into a workspace buffer.
 *   4. The pseudopotential at x_cur, exactly as ds_ecp_energy(x_cur, philox_seed, philox_offset + 1 + i) evaluates it: the triple
 *      (E_loc, Re E_nl, Im E_nl), and in the workspace the pair offsets, the pair records and the terms (W / N_q) q of every
 *      configuration.  A pair total above pair_capacity fails the call here, with ds_ecp_energy's message: the state is exactly
 *      that after i steps and *steps_done = i.
 *   5. Commit.  x, logabs, phase, drift and eloc (= E_c' or the old eloc) are selected.  E = ((E_c + E_loc) + Re E_nl), each
 *      addition rounded in float64, in that order.  weight <- weight * exp(-tau_eff (clip(E) - e_trial)) with the clip of
 *      ds_dmc_step: the ONE-POINT weight; a result that is not finite becomes 0.  epp <- the triple.  Flag "clipped" from clip(E).
 *   6. T-move, only for a walker of positive weight and finite E that has at least one pair.  Its configurations are
 *      c = 0 .. n_w N_q - 1 in (pair, q) order, term_c the complex (W / N_q) q of step 4.
 *        t_c = -tau min(Re term_c, 0)          (tau, not tau_eff; for a complex wavefunction the real part decides)
 *        r_{-1} = 1,  r_c = r_{c-1} + t_c      (one rounded float64 addition each, in this order);  Z = r_last
 *        u = the stream-2 uniform at index B + 1 + w, counter philox_offset + i, as a 53-bit uniform in [0, 1) (index w is the
 *            acceptance uniform, index B the comb's), or tmove_uniforms[i, w]
 *        theta = u Z                            (one rounded product)
 *        theta < 1: no move.  Otherwise the chosen c = the number of c with r_c <= theta, clamped to the last c with t_c > 0
 *        (no t_c > 0: no move).  This sequential order is normative.
 *      The electron of the chosen pair moves to the quadrature point by the arithmetic of ds_ecp_energy's displaced rows,
 *      (r_i - r dhat) + r U_q from the same pair record and rotation, rounded to T, and is wrapped as step 2 wraps.  Nothing else
 *      in the row changes.  There is no node test on a T-move (node_mode governs the diffusion move only): the terms with
 *      Re term < 0 are exactly those the effective Hamiltonian keeps, whatever the sign of the ratio.
 *   7. One chain pass at x (all B walkers), plus Ewald.  For the walkers that made a T-move only, logabs, phase, drift and eloc are
 *      replaced by its outputs; a logabs or eloc that is not finite there sets the weight to 0.  The others keep their rows.
 *   8. The out_stats row: the nine columns of ds_dmc_step in its fixed order, from the weights after step 5 and E of step 5
 *      (column [6] counts the non-finite proposals as before).  out_ecp_stats is taken at the same point with the same tree.
 *   9. The comb, as in ds_dmc_step_ecp, epp gathered from the same parents.
 * Rotations: stream 4 with the counter philox_offset + 1 + i, the counter step i of ds_dmc_step_ecp uses.  `steps` steps in one call
 * equal `steps` calls of one step with the offset advanced and state_valid = 1 (branch_every 0 or 1).
 * Synchronisation, capacity, the split of a smaller workspace and bit-identity for any split are those of ds_dmc_step_ecp, with one
 * synchronisation per step and none for the initialisation.  Workspace: ds_dmc_tmove_workspace_bytes = the layout of
 * ds_dmc_step_ecp followed by x_cur, E, the partials of out_ecp_stats and the choice.
 * Refused with a ds_last_error message before any launch: everything ds_dmc_step_ecp refuses, with the five explicit inputs given in
 * part in place of its four.  Every other entry point is unchanged.
 * Out of scope: the size-consistent per-electron T-moves of Casula, Moroni, Sorella and Filippi (2010), a symmetric weight with
 * T-moves, T-moves in ds_dmc_branch, a synchronisation-free evaluation. */
int64_t ds_dmc_tmove_workspace_bytes(const ds_system* sys, const ds_ecp* ecp, int64_t B, int64_t pair_capacity);
int ds_dmc_step_tmove(ds_system* sys, const ds_ecp* ecp, const void* params, void* x, void* logabs, void* phase, void* drift,
                      double* eloc, double* weight, double* epp, int64_t B, int steps, double tau, double tau_eff, double e_trial,
                      double e_ref, double e_cut, int node_mode, int branch_every, uint64_t philox_seed, uint64_t philox_offset,
                      const void* normals, const void* uniforms, const double* comb_uniforms, const double* rotations,
                      const double* tmove_uniforms, int64_t pair_capacity, int state_valid, double* out_stats,
                      double* out_ecp_stats, int32_t* out_parents, int64_t* out_pairs, int32_t* out_tmove, double* out_energy,
                      int* steps_done, void* ws, int64_t ws_bytes, void* stream);
/* What a Philox-mode ds_dmc_step call of `steps` steps draws, written out in the layout of its explicit mode: normals
 * (steps, B, 3N) and uniforms (steps, B) of dtype T, comb_uniforms (steps,) float64 [device].  The normals are the device's own
 * Box-Muller values (a host model agrees with them to a few ulp, not to the bit), so a float64 call that replays these arrays
 * gives the bits of the Philox-mode call.  (In float32 the explicit uniforms are rounded to T; the Philox mode compares in float64.) */
int ds_dmc_noise(int dtype, int n_elec, int64_t B, int steps, uint64_t philox_seed, uint64_t philox_offset, void* normals,
                 void* uniforms, double* comb_uniforms, void* stream);
int64_t ds_dmc_branch_workspace_bytes(int dtype, int n_elec, int64_t B);
int ds_dmc_branch(int dtype, int n_elec, int64_t B, double xi, void* x, void* logabs, void* phase, void* drift, double* eloc,
                  double* weight, int32_t* out_parents, void* ws, int64_t ws_bytes, void* stream);

/* Forward walking for the DMC above (csrc/ds_fw.h): pure estimators from the parents that every DMC entry
 * can write.  The pure estimate of an observable O at a lag of L blocks is
 *   sum_w w_w(t + L) O(x_anc(w)(t)) / sum_w w_w(t + L),
 * the snapshot taken L blocks ago weighted with what its descendants weigh now; anc(w) is the walker of the snapshot from which
 * walker w descends.  The three entries need no ds_system, use no floating-point atomics and are bit-identical from run to run.
 * An index read from a caller's array is range-checked in the kernel before it is used as an address: garbage in `parents` or
 * `index` gives counted skips, never a fault.  All pointers are device arrays unless marked HOST.
 *
 * ds_dmc_ancestry carries ancestor tables through one block of `steps` steps.
 *   parents (steps, B) int32: parents[k][w] is the walker before step k from which walker w after step k descends.  This is
 *     exactly what the step entries write to out_parents: the identity for a step without a comb.  NULL with steps = 0.
 *   Block map: P[w] = parents[0][parents[1][... parents[steps-1][w]]].  An entry outside [0, B) anywhere in the chain gives
 *     P[w] = -1.  steps = 0 gives the identity.
 *   anc (n_slots, B) int32, updated in place: for every slot s, anc_s[w] <- anc_s_old[P[w]], and -1 where P[w] = -1.  The old
 *     table is read out of place (a copy in the workspace).  A value of the old table is copied as it is, never used as an address:
 *     anc_old = -1 stays -1, "-1 means the lineage is lost" propagates.  NULL with n_slots = 0.
 *   out_block (B,) int32, or NULL: receives P.
 *   steps = 0 or n_slots = 0 is valid.  Workspace: ds_dmc_ancestry_workspace_bytes(B, n_slots) = 4 B (1 + n_slots) bytes; a
 *   smaller ws_bytes is refused ("workspace too small").  Refused too: B < 1 or B > 2^31 - 1, negative steps or n_slots, a null
 *   array that the call would read or write.
 *
 * ds_realspace_counts_w is ds_realspace_counts with a source row and an integer weight per walker.  It takes the arguments of
 * ds_realspace_counts, with the same meaning, limits and binning rules (the two kernels share the binning code), and then:
 *   B_src: x has shape (B_src, 3 n_elec); B is the number of walkers, the length of index and weight.
 *   index (B,) int32, or NULL: walker w contributes the positions of source row src = index ? index[w] : w of x.
 *   weight (B,) float64, or NULL, and weight_scale: the walker contributes with the integer weight
 *     q = weight ? llrint(weight[w] * weight_scale) : 1   (round to nearest, ties to even).
 *   Skipped and counted in n_bad[0]: src outside [0, B_src).  Skipped and counted in n_bad[1]: a weight that is not finite, a
 *     negative weight, or q > 2^24.  A walker with both counts under n_bad[0] alone.  q = 0 contributes nothing and is not bad.
 *   Every density bin and pair bin that ds_realspace_counts would increment by 1 for that row is incremented by q.
 *   q_sum int64[1]: q_sum += the sum of q over the contributing walkers.  n_bad int64[2]: added to, as above.  Neither is zeroed.
 *   All additions are integer atomics, so the buffers do not depend on the order of the additions.  The pair bins in LDS are
 *   64-bit: one workgroup adds at most 2^18 walkers x 8128 pairs x 2^24 < 2^55 to a bin.  Overflow of the global int64 buffers is the
 *   caller's: a call adds at most B n_elec 2^24 to a density bin and B n_elec (n_elec - 1) / 2 x 2^24 to a pair bin.
 *   Refused too: null q_sum or n_bad, B_src < 1, B > B_src without an index, a weight_scale that is not positive and finite (with
 *   a weight).
 *
 * ds_dmc_fw_sums forms weighted sums of per-walker values.
 *   values (B_src, K) float64, 1 <= K <= 64; index, weight as above (weight = NULL means 1; there is no scale: the weight enters
 *   as the float64 it is).
 *   out (K, 2) float64, overwritten: out[k] = (sum_w w_w v[src_w, k], sum_w w_w).  The sum runs over the walkers with a valid src, a
 *     finite weight > 0 and a finite v[src, k].
 *   n_bad int64[2], added to: [0] walkers whose src is outside [0, B_src); [1] walkers whose weight is not finite or negative,
 *     plus every (walker, column) whose value is not finite.  A weight of 0 is skipped and not bad.
 *   Summation order: that of out_stats in ds_dmc_step.  One row of partials per 256 consecutive walkers (thread t holds walker t, a
 *     skipped one holds 0; a tree adds t and t + s for s = 128, 64, .., 1), then the rows are added in order onto 0.  Each product
 *     w v is rounded once before it is added.
 *   Workspace: ds_dmc_fw_sums_workspace_bytes(B, K) = 16 K ceil(B / 256) bytes. */
int64_t ds_dmc_ancestry_workspace_bytes(int64_t B, int n_slots);
int ds_dmc_ancestry(int64_t B, int steps, const int32_t* parents, int n_slots, int32_t* anc, int32_t* out_block, void* ws,
                    int64_t ws_bytes, void* stream);
int ds_realspace_counts_w(const double* fold_inv, const int32_t* grid, const double* latvec, const double* latvec_inv, double r_max,
                          int n_r, int dtype, const void* x, int64_t B, int64_t n_elec, int64_t n_up, int64_t* dens, int64_t* pair,
                          int64_t B_src, const int32_t* index, const double* weight, double weight_scale, int64_t* q_sum,
                          int64_t* n_bad, void* stream);
int64_t ds_dmc_fw_sums_workspace_bytes(int64_t B, int K);
int ds_dmc_fw_sums(int64_t B, int K, const double* values, int64_t B_src, const int32_t* index, const double* weight, double* out,
                   int64_t* n_bad, void* ws, int64_t ws_bytes, void* stream);

/* Packed batch statistics of train.make_loss.total_energy (train.py:74-82) in one deterministic reduction:
 * out_stats (8,) float64 on the device =
 *   [ sum Re E_L, sum Im E_L, sum |E_L|^2, n, n_nonfinite, sum Re E_kin, sum Im E_kin, sum E_ewald ],  E_L = ke + ewald.
 * The vector is what crosses GPUs in ONE all-reduce (replacing the pmeans of train.py:78-80); n_nonfinite is the
 * count behind the reference's optional check_nan step rejection (process.py:303-318). */
int ds_energy_stats(ds_system* sys, const void* ke, const void* ewald, int64_t B, double* out_stats, void* stream);

/* Stage dumps for parity tests (tests only; sizes documented in DESIGN.md).
 * Runs the forward-Laplacian chain for the first walkers of the batch and copies
 * the named intermediate into `out` (device, dtype elements).  Returns elements written. */
int64_t ds_debug_stage(ds_system* sys, const void* params, const void* x, int64_t B,
                       const char* stage, void* out, int64_t out_elems,
                       void* ws, int64_t ws_bytes, void* stream);

/* Per-kernel timing with HIP events recorded on the caller's stream around every launch of the
 * local-energy chain (bench.py's roofline numbers).  ds_profile_enable(sys, 1) resets and starts for every
 * kernel, ds_profile_enable(sys, 2 + kind) for one kernel kind only (no events around the others), 0 stops;
 * ds_profile_read synchronises the recorded events and returns, per kernel kind, the summed
 * duration in ms and the number of launches (arrays of DS_PROF_KINDS entries). */
#define DS_PROF_FEATURES 0
#define DS_PROF_M2_EXPAND 1
#define DS_PROF_TWO_LAYER 2
#define DS_PROF_SINGLE_FIRST 3   /* one-electron layer 0 (K = 4A + 8): k_layer0_stats / k_jet_gemm<.,9> + k_layer0_means in front of the low-rank layer 1, else k_jet_gemm<.,1> */
#define DS_PROF_SINGLE_HIDDEN 4  /* k_jet_gemm<.,2> of the dense hidden one-electron layers (K = 256 + 64): the dominant kernel */
#define DS_PROF_ORBITAL 5        /* k_jet_gemm<.,5> of the orbital head (fused envelope x phase epilogue) */
#define DS_PROF_DET_INVERSE 6
#define DS_PROF_DET_TRACE 7
#define DS_PROF_COMBINE 8
#define DS_PROF_EWALD 9
#define DS_PROF_SHARED_TERM 10    /* per-walker spin-mean term S = W_sh^T mean_i h_i (k_shared_term; layer 0: k_jet_gemm<.,0>) */
#define DS_PROF_SINGLE_LR 11     /* k_layer1_lr: the first hidden layer on the low-rank form of the layer-0 output */
#define DS_PROF_ION_VJP 12      /* one chunk of ds_logpsi_ion_vjp: value chain, seed, one-electron sweep, k_ion_grad */
#define DS_PROF_KINDS 13
int ds_profile_enable(ds_system* sys, int on);
int ds_profile_read(ds_system* sys, double* ms_total, int64_t* launches);
/* In-kernel clock probe of the dominant kernel (hidden one-electron layers), active while profiling is enabled for it: one
 * wave per workgroup reads the shader-clock counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) at entry
 * and exit; the sums over all workgroups since ds_profile_enable are returned.  shader_cycles / ref_ticks x 100 MHz is the
 * clock the kernel actually ran at in that region (the MFMA peak scales with it). */
int ds_profile_read_clock(ds_system* sys, double* shader_cycles, double* ref_ticks);
/* Kernel-development aid: shader-clock stamps written by one wave of the hidden-layer kernel at its phase boundaries when the
 * library runs with DS_DBG=32 and profiling is enabled (tools/gemm_timeline.py); n <= 1022 stamps. */
int ds_debug_timeline(ds_system* sys, uint64_t* out, int n);

/* Calibration kernel for the rocprofv3 FETCH_SIZE / WRITE_SIZE counters: copies n_elems float64
 * with the 8-byte-per-lane access pattern of the jet tensors (known traffic = 8 n read + 8 n written). */
int ds_calib_copy(const void* src, void* dst, int64_t n_elems, void* stream);

/* fp64 MFMA issue-rate micro-benchmark used to confirm the roofline peak: every wave issues
 * `iters` x `n_acc` independent v_mfma_f64_16x16x4_f64 (n_acc = 1,2,4,8,16 accumulators), with
 * `blocks_per_cu` waves resident per SIMD; returns the FLOPs executed (caller times with HIP events). */
int64_t ds_mfma_f64_peak(int64_t iters, int blocks_per_cu, int n_acc, void* scratch, void* stream);

/* Hartree-Fock crystalline orbitals of a Gaussian basis (hf.py:84-153 without PySCF; csrc/ds_hf.h); needs no
 * ds_system.  Every pointer of the descriptor is a HOST array that ds_hf_create copies; conventions of PySCF's PBCGTOval_sph:
 *   ao_k,mu(r) = sum_L exp(i k.L) R_mu(|d|) S_lm(d),  d = r - R_atom(mu) - L,  R = sum_p coefs_p exp(-exps_p |d|^2),
 *   S_lm orthonormal real solid harmonics, l = 1: x, y, z; l = 2: xy, yz, z^2, xz, x^2-y^2; AO index: shells in order, m inside.
 * a: primitive cell (rows = lattice vectors, Bohr); atoms (n_atoms, 3); shell_atom / shell_l (0..2) / shell_nprim (n_shells),
 * exps / coefs: the primitives of all shells back to back, coefficients as applied (normalised); sum (2l+1) <= 128 AOs;
 * kpts (n_k <= 64, 3); images (n_images, 3): the lattice translations L to sum over, in summation order;
 * n_up, n_dn <= 64 electrons per spin; nocc_up / nocc_dn (n_k): occupied bands per k point, summing to n_up / n_dn;
 * mo_up / mo_dn: (nao, n_s) complex128 as (re, im) pairs, row-major, columns ordered by k point and then band. */
typedef struct ds_hf ds_hf;
typedef struct ds_hf_desc {
    double a[9];
    int32_t n_atoms;
    const double* atoms;
    int32_t n_shells;
    const int32_t* shell_atom;
    const int32_t* shell_l;
    const int32_t* shell_nprim;
    const double* exps;
    const double* coefs;
    int32_t n_k;
    const double* kpts;
    int32_t n_images;
    const double* images;
    int32_t n_up, n_dn;
    const int32_t* nocc_up;
    const int32_t* nocc_dn;
    const double* mo_up;
    const double* mo_dn;
} ds_hf_desc;
/* Copies the tables to the device once and precomputes the (n_k, n_images) table of exp(i k.L); no allocation afterwards. */
int ds_hf_create(const ds_hf_desc* desc, ds_hf** out);
void ds_hf_destroy(ds_hf* hf);
/* Orbital matrices at B walkers: x (B, 3N) device array, dtype 0 = f64, 1 = f32 (widened on load; all arithmetic is float64);
 * out_up (B, n_up, n_up), out_dn (B, n_dn, n_dn) complex128 device arrays [walker, electron, orbital] (NULL for a spin without
 * electrons).  The walker is wrapped into the primitive cell and the wrap phase exp(i k.(wrap a)) applied (hf.py:113-120).
 * Needs no workspace; no atomics and a fixed summation order: a walker's rows have the same bits wherever it sits in the batch.
 * A chunk of 64 images (32 beyond 64 AOs) is skipped when alpha_min |d|^2 > 90 for each of its images and every atom. */
int ds_hf_orbitals(ds_hf* hf, int dtype, const void* x, int64_t B, void* out_up, void* out_dn, void* stream);
/* The orbitals of ONE spin at arbitrary points: points (P, 3) device array of `dtype`, out (P, M_spin) complex128 [point, orbital].
 * The same computation as ds_hf_orbitals, by the same device function (wrap into the primitive cell, wrap phase, image sum on
 * v_mfma_f64_16x16x4_f64, contraction with the MO columns in index order); only the spin is the argument's instead of derived from
 * an electron index: for an electron's position the bits are those ds_hf_orbitals returns for it.  M_spin == 0 or P == 0 returns 0
 * and launches nothing.  At most 2^31 - 1 points per call. */
int ds_hf_orbitals_at(ds_hf* hf, int spin, int dtype, const void* points, int64_t P, void* out, void* stream);

/* One-body reduced density matrix (1-RDM) in a basis of crystalline orbitals, folded from the ratios and shifts that
 * ds_one_body_ratios exports (csrc/ds_obdm.h); needs no ds_system.  The reference has no such estimator: the
 * conventions are this library's own.
 *
 * A basis is a ds_hf (a `hf.GaussianOrbitals` object).
 *   - Its columns per spin are the basis functions phi^s_i, i < M_s <= 64.
 *   - They need not be occupied or orthonormal.  Its `nelec` is simply (M_up, M_dn).
 *   - It is independent of the electron numbers of the network.
 *   - PySCF normalises an orbital to 1 over the basis's primitive cell, volume Omega_p = |det a|.
 *
 * For spin s:
 *     n^s_ij = < sum_{e in s} int_{Omega_S} dr' chi_i*(r') chi_j(r_e) psi(..., r_e -> r', ...)/psi(R) >_{|psi|^2},
 *                                                                                       chi = phi / sqrt(Omega_S/Omega_p)
 *     S^s_ij = int_{Omega_S} dr' chi_i*(r') chi_j(r')
 * Here r' = r_e + s, and s is uniform in the simulation cell Omega_S, as drawn by ds_one_body_ratios.
 *
 * One sample (w, m) moves electron e = (first_electron + m) % N of walker w.  Its spin is s(e) = 0 if e < n_up, else 1.  With an
 * optional weight w_s (default 1) it adds:
 *     dm_sums[s][i][j] += w_s q conj(phi^s_i(r')) phi^s_j(r_e)
 *     ov_sums[s][i][j] += w_s   conj(phi^s_i(r')) phi^s_j(r')
 * The weight is 1/(Omega_S p(s)) for a caller who supplies shifts from another proposal density p.
 *
 * Host normalisation, with the same sample counting as the momentum distribution:
 *   - n^s = N_s Omega_p dm_sums[s] / good_s
 *   - S^s = Omega_p ov_sums[s] / good_s
 *   - good_s = samples on s - bad_s
 * With phi_k = e^{ik.r}/sqrt(Omega_p) this reduces to n_s(k) of section 16.
 *
 * A sample whose q or weight is not finite is left out of both sums and counted per spin.
 *
 * The integrand is periodic over Omega_S only under two conditions (checked by `estimator.OneBodyDensityMatrix`, not here):
 *   - the simulation cell is a superlattice of the basis's cell, so sim.a @ inv(basis.a) is an integer matrix;
 *   - every basis k point is Bloch-allowed, so (k - k_t).a_S/2pi is an integer vector for the network's k_t.
 *
 * Arguments: x (B, 3N); ratio (B, M, 2) and shift (B, M, 3) exactly as ds_one_body_ratios writes them; x, ratio and shift of `dtype`
 * (0 = f64, 1 = f32); weight (B, M) float64 or NULL; dm_sums and ov_sums (2, Mb, Mb, 2) float64 with Mb = max(M_up, M_dn), ADDED to
 * and never zeroed, either one may be NULL, not both; rows and columns >= M_s are not touched; n_bad (2,) int64, added to, optional.
 * r_e is the walker's coordinate widened to float64; r' is formed as (T)((double)r_e + (double)shift) in the type T of `dtype` --
 * the expression and type in which ds_one_body_ratios forms the displaced coordinate -- and then widened: the basis is evaluated
 * where the network was.  (In float32 the exported shift is the drawn float64 shift rounded once, so r' can differ from the
 * network's by one float32 rounding; a float32 caller who needs the identical point replays the exported shifts in both calls.)
 *
 * Per chunk of samples: (1) the basis of spin s(e) at r_e and at r' into the workspace, through the device function of
 * ds_hf_orbitals_at; (2) k_obdm_accumulate: one workgroup per fixed group of 128 consecutive global sample indices contracts, on
 * the f64 MFMA and per spin, the rows [Re; Im] of conj phi(r') against the columns of w_s q phi(r_e) (and of w_s phi(r')) staged
 * through LDS -- a sample of the other spin or a bad one is an exact zero -- and writes one partial row; (3) a second kernel adds the
 * rows in row order to a running sum and after the last chunk adds that to the caller's buffers.  No floating-point atomics, no
 * host synchronisation, no allocation.  The sums are bit-identical from run to run and for ANY ws_bytes: chunks are whole groups,
 * a smaller workspace means more chunks; below one group the call is an error.  A second call on the same buffers doubles them
 * exactly.  ds_obdm_workspace_bytes: room for every group of the call, at most 256 MiB (one group at least); -1 for a null basis,
 * B < 1 or n_samples < 1.
 *
 * Refused before any launch: a null basis, x, ratio or shift; both sums NULL; B < 1; n_samples < 1; n_elec < 1; n_up outside
 * 0..n_elec; first_electron outside 0..n_elec-1; dtype not 0 or 1; more than 2^31 - 1 samples.  A spin that has electrons but no
 * basis functions contributes nothing and is not counted as bad.
 *
 * Limits: uniform r' has a large variance for core orbitals of all-electron ions (of order Omega_S over the orbital's volume);
 * valence bands and pseudopotential cells are the use case.  No error bars.  <= 64 basis functions per spin, <= 128 AOs, l <= 2. */
int64_t ds_obdm_workspace_bytes(const ds_hf* basis, int64_t B, int n_samples);
int ds_obdm_accumulate(ds_hf* basis, int dtype, const void* x, int64_t B, int n_elec, int n_up, int n_samples, int first_electron,
                       const void* ratio, const void* shift, const double* weight, double* dm_sums, double* ov_sums, int64_t* n_bad,
                       void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPSOLID_HIP_H */
