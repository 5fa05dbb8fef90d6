/* mtip_hip.h -- C ABI of libmtip_hip.so, the MI355X (gfx950) MTIP phasing engine.
 *
 * This is the drop-in boundary for the hot path of European-XFEL/xFrame's
 * `xframe/projects/fxs/reconstruct.py` (reference file:line cited per entry point; paths are
 * relative to the reference checkout).  The reference binds its GPU code through PyOpenCL
 * (`xframe/externalLibraries/openCL_plugin.py:154-226`) behind
 * `Multiprocessing.comm_module.add_gpu_process` (`xframe/control/communicators.py:79-82`);
 * a maintainer replaces that with a ctypes binding of the functions below.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MTIP_E* code; nothing throws across the ABI;
 *     `mtip_last_error(ctx)` returns a human readable message (ctx may be NULL for create errors: the message of the
 *     last failed mtip_create on the calling thread);
 *   - host buffers are caller-owned, C-contiguous; complex128 = interleaved (re,im) doubles
 *     (numpy complex128); masks are uint8 (numpy bool); device memory is library-owned;
 *   - a ctx is bound to one device and one hipStream_t; it is not thread-safe; several ctxs may
 *     be used concurrently (one per GPU / per process, or several per GPU from different host threads);
 *     the stream is created hipStreamNonBlocking: it does NOT synchronise with the null stream, so a caller's own
 *     null-stream work is not ordered against a ctx's kernels (call mtip_synchronize); every entry point that moves
 *     data to or from the host waits for the ctx's own stream itself and returns with the copy complete;
 *   - array shapes: grid  (n_batch, Nq, n_theta, n_phi);  coeff 'direct' (n_batch, Nq, (L+1)^2)
 *     with index l(l+1)+m  (`xframe/externalLibraries/shtns_plugin.py:24,105-114,250-261`).
 */
#ifndef MTIP_HIP_H
#define MTIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mtip_ctx mtip_ctx;
typedef struct { double re, im; } mtip_cdouble;

enum {
    MTIP_OK = 0,
    MTIP_EINVAL = -1,      /* bad argument / shape                        */
    MTIP_ENODEV = -2,      /* no usable HIP device                        */
    MTIP_EHIP = -3,        /* a HIP runtime call or kernel launch failed  */
    MTIP_ENOMEM = -4,
    MTIP_ESTATE = -5       /* call order violated (e.g. run before setup) */
};

/* phasing methods: the sketches of reconstruct.py:565-596 */
enum { MTIP_HIO = 0, MTIP_ER = 1, MTIP_HIO_NON_FXS = 2, MTIP_ER_NON_FXS = 3 };

/* SHT load-side prologues (fused elementwise stages) */
enum { MTIP_PRE_NONE = 0, MTIP_PRE_SQUARE = 1 /* |x|^2, misk.py:159-168 */, MTIP_PRE_ABS = 2 /* |x|, misk.py:221-225 */ };

typedef struct {
    int32_t n_radial;      /* Nq: grid.n_radial_points                                   */
    int32_t l_max;         /* L : grid.max_order, 0 <= L <= 128.  L <= 63: everything; 64 <= L <= 128: the transforms
                              (mtip_op_sht_*, mtip_op_hankel, mtip_op_fourier_transform), mtip_op_deg2_invariants and the
                              context-independent operators -- the phasing loop (mtip_run*, mtip_shrinkwrap, ..),
                              mtip_set_projection_matrix, mtip_op_project_* and mtip_op_apply_unknowns return MTIP_ESTATE
                              unless `reserved` has MTIP_CFG_LOOP_BIG_L.  With it they run up to L = 128; still refused
                              (MTIP_ESTATE, before any launch): an active order with min(2l+1, Nq) > 128 columns, a
                              per-restart ft_stab mask (mtip_set_ft_stab_mask with both values) */
    int32_t n_theta;       /* Gauss-Legendre nodes (shtns_plugin.py:94-101 for defaults) */
    int32_t n_phi;         /* power of two, > 2L                                         */
    int32_t n_batch;       /* restarts resident in this ctx (>=1)                        */
    int32_t hankel_trapz;  /* 0: midpoint/gauss rule (hankel_transforms.py:702-731);
                              1: trapz/Zernike (671-700: weights have Nq-1 rows, reads f[p+1]) */
    int32_t fused;         /* 1: algebraically fused step, 0: reference operator order */
    int32_t reserved;      /* flag word: MTIP_CFG_* below; any other bit makes mtip_create fail (invalid cfg) */
} mtip_cfg;

/* mtip_cfg.reserved bit 0: the phasing loop and the projection beyond L = 63 (opt-in; no effect for L <= 63) */
#define MTIP_CFG_LOOP_BIG_L 1

/* ---- life cycle ------------------------------------------------------------------------------
 * replaces Multiprocessing.get_number_of_gpus (xframe/Multiprocessing.py:892-898) and the
 * OpenCL context/buffer creation of openCL_plugin.py:28-61,118-152 */
int mtip_device_count(void);
mtip_ctx* mtip_create(const mtip_cfg* cfg, int device);
void mtip_destroy(mtip_ctx* ctx);
const char* mtip_last_error(const mtip_ctx* ctx);
int mtip_get_cfg(const mtip_ctx* ctx, mtip_cfg* out);
int mtip_synchronize(mtip_ctx* ctx);

/* ---- one-off setup (host side of rows a1, a2, a4, a7 of SURVEY section 8) -------------------- */
/* cos(theta) north->south and Gauss weights, n_theta each (shtns_plugin.py:130-133). The library
 * builds the orthonormal Condon-Shortley Legendre tables itself. */
int mtip_set_angular_grid(mtip_ctx* ctx, const double* cos_theta, const double* gauss_weights);
/* radial points r_p, q_k (ft_grid_pairs.py:282-291), Nq each */
int mtip_set_radial_grid(mtip_ctx* ctx, const double* r, const double* q);
/* raw real Hankel weights w[l][p][k] exactly as calc_spherical_mid_weights / _trapz_weights return
 * them (hankel_transforms.py:399-410 / 322-333), shape (L+1, Np, Nq) with Np = Nq (midpoint) or Nq-1
 * (trapz); fwd_scale=(r_max/N)^3 sqrt(2/pi), inv_scale=(q_max/N)^3 sqrt(2/pi) (assemble_weights_mid,
 * 426-452); the (-i)^l / (+i)^l phases are applied in the kernel epilogue. */
int mtip_set_hankel_weights(mtip_ctx* ctx, const double* w_raw, double fwd_scale, double inv_scale);
/* modified projection matrix V_l (fxs_Projections.py:679-714), shape (Nq, k_l) row-major, its radial
 * mask row (578-629, Nq bytes) and whether order l takes part in the projection (used_orders, 492). */
int mtip_set_projection_matrix(mtip_ctx* ctx, int l, const mtip_cdouble* V, int k_l,
                               const uint8_t* radial_mask, int used);
int mtip_set_number_of_particles(mtip_ctx* ctx, double n_particles);   /* fxs_Projections.py:497,870 */
/* projections.reciprocal.SO_freedom (fxs_Projections.py:493, 768-780): after every approximate_unknowns the element [4][2] of the
 * unknowns of `order` loses its imaginary part before the unknowns are applied (the host ranks the orders,
 * fxs_invariant_tools.py:1467-1486); order = -1 switches it off (default) */
int mtip_set_so_freedom(mtip_ctx* ctx, int order);
/* reference B_l = V_l V_l^+ masks for the deg2_invariant_l2_diff metric are derived internally
 * (fxs_IO_methods.py:408-447); enable = 1 evaluates it every step. */
int mtip_set_deg2_metric(mtip_ctx* ctx, int enable);
/* generate_main_error_routine (fxs_IO_methods.py:746-765): the main error of a step is `type` (0 mean, 1 min, 2 max,
 * 3 prod) over the last values of the chosen metrics.  use_reciprocal_deg2 = 0: the real l2_projection_diff metric (a
 * scalar: every type returns it); 1: the per-order values of deg2_invariant_l2_diff (one entry per used order, -1 where
 * the reference invariant vanishes).  Mixing both makes the reference itself raise (np.array of a scalar and a vector). */
int mtip_set_main_error(mtip_ctx* ctx, int use_reciprocal_deg2, int type);
/* the same routine over any of the metrics the loop records (fxs_IO_methods.py:753-760: the last values of main.metrics.real, then
 * of main.metrics.reciprocal, each in the order the settings list them): items[n_items <= 8] = 0 real l2_projection_diff,
 * 1 deg2_invariant_l2_diff (the per-order vector: the only item then, as the reference raises on a mix), 2 reciprocal
 * l2_projection_diff, 3 II_error, 4 ccd_diff, 5 deg2_ranked_invariant_l2_diff = the entry of order deg2_ranked_column (0 .. L) of
 * the deg2 metric (fxs_IO_methods.py:330-366).  Reduced as numpy does: mean = the sum in list order / n, and a NaN item makes every
 * type NaN, which never becomes the best error (reconstruct.py:934).  A *_non_FXS step records no reciprocal value and reads
 * the last FXS step's; while there is none -- none since mtip_init_state, or since one of the metrics was switched on -- the main
 * error is -1 (762-764).  An item whose metric is off fails the run with MTIP_ESTATE before anything is launched.
 * mtip_set_main_error(ctx, u, type) is items = {u ? 1 : 0}. */
int mtip_set_main_error_ex(mtip_ctx* ctx, int type, int n_items, const int* items, int deg2_ranked_column);
/* the non-default reciprocal metrics II_error / ccd_diff / fqc_error (fxs_IO_methods.py:587-627, 651-683, 507-550), evaluated in
 * every FXS step from B_l of the current intensity coefficients.  which: 1 | 2 | 4 (0 switches them off); zero_mask (L+1, Nq, Nq):
 * 1 = entry of B_l outside the invariant mask (zeroed); II: masked reference sum_{l>=1} B_l^ref (Nq, Nq), qq = (q q')^2;
 * ccd: P^C_l(q) P^C_l(q') / (2l+1) per order with the rows of order 0 and of orders < C_order zero (L+1, Nq, Nq), reference C (Nq, Nq),
 * its squared norm; fqc: P (L+1, Nq, Nq, L+1) = P^m_l(q) P^m_l(q') / (2l+1) indexed [l][q][q'][m], reference average (Nq, Nq),
 * reference weights (L+1, Nq, Nq).  The host prepares the tables (xframe_amd/fxs/hostsetup.py). */
int mtip_set_invariant_metrics(mtip_ctx* ctx, uint32_t which, const uint8_t* zero_mask, const mtip_cdouble* II_reference, const double* qq,
                               const double* ccd_weights, const mtip_cdouble* ccd_reference, double ccd_norm, const double* fqc_P,
                               const double* fqc_reference_average, const double* fqc_reference_weights);
/* their values for the steps [first, first + n_steps): II (n, n_batch), ccd (n, n_batch), fqc (n, n_batch, Nq); NULL skips one */
int mtip_fetch_invariant_metrics(mtip_ctx* ctx, int64_t first_step, int64_t n_steps, double* II, double* ccd, double* fqc);
/* the same metrics of given intensity coefficients (n_batch, Nq, (L+1)^2): II (n_batch), ccd (n_batch), fqc (n_batch, Nq) */
int mtip_op_invariant_metrics(mtip_ctx* ctx, const mtip_cdouble* Ilm, double* II, double* ccd, double* fqc);
/* the reciprocal metric l2_projection_diff (fxs_IO_methods.py:301-310, 96-127, 131-205): per FXS step int |F - F'|^2 / int |F|^2 with the
 * integrator weights radial_w (Nq), theta_w (n_theta) -- shell Nq - 2 zeroed by the caller, the reference's `square[~True] = 0`; NULL
 * weights switch the metric off.  fetch: the steps [first, first + n_steps) as (n, n_batch). */
int mtip_set_reciprocal_l2_metric(mtip_ctx* ctx, const double* radial_w, const double* theta_w);
int mtip_fetch_reciprocal_l2_metric(mtip_ctx* ctx, int64_t first_step, int64_t n_steps, double* out);
/* real-space constraints (fxs_Projections.py:72-130, pythonLibrary.py:1289-1320):
 * flags bit0 support, bit1 value lower bound, bit2 value upper bound, bit3 limit_imag;
 * hio_mask_flags: which of those feed the HIO mask gamma ('considered_projections',
 * fxs_IO_methods.py:40-64; ['all'] = same as flags). */
int mtip_set_real_constraints(mtip_ctx* ctx, uint32_t flags, double value_lo, double value_hi,
                              double imag_threshold, uint32_t hio_mask_flags);
/* initial support S0 (fxs_Projections.py:133-155), (Nq, n_theta, n_phi) bytes, shared by the batch;
 * resets every restart's support to S0 and enforce_initial_support to 1 (fxs_Projections.py:34). */
int mtip_set_initial_support(mtip_ctx* ctx, const uint8_t* support);
/* error metric weights (fxs_IO_methods.py:97-128 with mathLibrary.py:1223-1235):
 * E = sum m(x) wr[q] wt[theta] |w-P|^2 / sum m(x) wr[q] wt[theta] |w|^2 ;
 * use_initial_support_mask: m = S0, else m = 1. */
int mtip_set_error_weights(mtip_ctx* ctx, const double* radial_w, const double* theta_w,
                           int use_initial_support_mask);

/* ---- state ------------------------------------------------------------------------------------ */
/* inject a starting density for restart `batch` (reconstruct.py:957-966: rho0 -> F0=FT(rho0),
 * rho0'=IFT(F0) is done by mtip_init_state) */
/* The guesses are staged in device scratch that every mtip_op_* call may overwrite: set all restarts, then call
 * mtip_init_state, with no mtip_op_* call in between. */
int mtip_set_density(mtip_ctx* ctx, int batch, const mtip_cdouble* rho);
int mtip_init_state(mtip_ctx* ctx);
/* which = 0 latest pair, 1 best pair (reconstruct.py:934-938) */
int mtip_get_density(mtip_ctx* ctx, int batch, int which, mtip_cdouble* rho);
int mtip_get_reciprocal_density(mtip_ctx* ctx, int batch, int which, mtip_cdouble* F);
int mtip_get_support(mtip_ctx* ctx, int batch, int which, uint8_t* support);
int mtip_set_support(mtip_ctx* ctx, int batch, const uint8_t* support, int enforce_initial_support);
/* fxs_unknowns U_l of the last step (k_l x (2l+1), row-major), fxs_Projections.py:752-767 */
int mtip_get_unknowns(mtip_ctx* ctx, int batch, int l, mtip_cdouble* U);
/* best_error per restart (n_batch doubles) and the number of steps done */
int mtip_get_best_error(mtip_ctx* ctx, double* best_error, int64_t* n_steps_done);
/* take the best pair as the latest one (reconstruct.py:945-949) */
int mtip_select_best(mtip_ctx* ctx);
/* the same for the restarts with select[b] != 0 only (the reference decides per reconstruction process); NULL = all */
int mtip_select_best_where(mtip_ctx* ctx, const uint8_t* select);

/* ---- the loop (reconstruct.py:854-951) ------------------------------------------------------------
 * runs n_steps steps of `method` for every restart without host synchronisation; betas[n_steps] is the
 * HIO beta per step (ExponentialRamp, reconstruct.py:911).  real_err (n_steps x n_batch, may be NULL)
 * receives the l2_projection_diff error per step; deg2_err (n_steps x n_batch x (L+1), may be NULL)
 * the deg2_invariant_l2_diff metric when enabled. The call returns after the results are on the host. */
int mtip_run(mtip_ctx* ctx, int method, int ft_stab, int n_steps, const double* betas,
             double* real_err, double* deg2_err);
/* same, but only enqueues (no download, no sync): errors stay on the device until mtip_fetch_errors */
int mtip_run_async(mtip_ctx* ctx, int method, int ft_stab, int n_steps, const double* betas);
/* mtip_run_async for the n_ctx contexts of ONE device that a worker runs side by side (the restart groups of
 * reconstruct.py:104 `n_gpu_workers`, one stream each): the same steps, every context's results bit-identical to its own
 * mtip_run_async, enqueued so that the contexts take turns at the transforms of a step (which fill the chip) while the
 * projections of the others (a long chain on a few CUs) run beside them -- see mtip_api.hip.  All contexts must be in the
 * same loop state a mtip_run_async call would need; n_ctx = 1 is mtip_run_async.  On an error return the failing context holds
 * the message (mtip_last_error) and the contexts may have advanced by different numbers of steps (mtip_get_best_error reports each). */
int mtip_run_group_async(mtip_ctx* const* ctxs, int n_ctx, int method, int ft_stab, int n_steps, const double* betas);
/* ft_stab per restart for the runs that follow (ft_stab = 1 in mtip_run*): mask[n_batch] != 0 = this restart takes the
 * add-back.  The reference decides `ft_stab: link_to_enforce_initial_support` per reconstruction process
 * (reconstruct.py:836-850), so restarts of one batch can disagree.  NULL (default) or all set = every restart; needs the
 * fused step (cfg.fused = 1) when the values differ. */
int mtip_set_ft_stab_mask(mtip_ctx* ctx, const uint8_t* mask);
int mtip_fetch_errors(mtip_ctx* ctx, int64_t first_step, int64_t n_steps, double* real_err, double* deg2_err);
/* the main error per step (n_steps x n_batch): what best-pair tracking and the enforce_initial_support decision use */
int mtip_fetch_main_errors(mtip_ctx* ctx, int64_t first_step, int64_t n_steps, double* main_err);
/* one shrink-wrap update (reconstruct.py:598-605, 877-885; fxs_Projections.py:245-258):
 * enforce_initial_support_b = (last main error_b > error_limit); enforced[n_batch] (may be NULL)
 * returns the decision per restart.  The fixed amplitudes of the *_non_FXS variants survive this call and
 * mtip_refresh_reciprocal_density (reconstruct.py:898-904: only an FXS method or a new sub-loop resets them); they are
 * |F'| of the pair the reference's stale `hist` ends with (901): the input pair of the most recent step. */
int mtip_shrinkwrap(mtip_ctx* ctx, double sigma, double threshold, double error_limit, uint8_t* enforced);
/* Top of a sub-loop call (reconstruct.py:852-866): the reference re-reads its local `hist` from the state and forgets
 * the fixed amplitudes of the *_non_FXS variants.  Call it before the first method of every sub-loop. */
int mtip_begin_sub_loop(mtip_ctx* ctx);
/* 'SW_center' (reconstruct.py:606-613, 886-897), after mtip_shrinkwrap.  Reproduces the reference literally: its process
 * returns (support, copy(rho), FT(rho)), which the loop unpacks as (support, ft_density, density), so the latest pair
 * becomes (reciprocal, real) = (rho, FT(rho)); the history is rebuilt from the stale `hist` (893), i.e. the pair of the
 * most recent step is dropped.  The best pair is left untouched. */
int mtip_refresh_reciprocal_density(mtip_ctx* ctx);
/* B_l = I_l I_l^+ of FT(latest rho) (reconstruct.py:757-765, 992-993), (L+1, Nq, Nq) complex */
int mtip_last_deg2_invariant(mtip_ctx* ctx, int batch, mtip_cdouble* Bl);

/* ---- single operators (parity tests; the operator registry of reconstruct.py:370,391,445,485; the
 *      averaging of f-1).  All arrays carry the leading n_batch dimension.  The caller's buffers may be
 *      host memory or memory of the context's device (unified addressing decides the copy): the
 *      averaging keeps its batch in HBM between these calls. ---------------------------------------- */
int mtip_op_sht_forward(mtip_ctx* ctx, const mtip_cdouble* grid, mtip_cdouble* coeff, int prologue);
int mtip_op_sht_inverse(mtip_ctx* ctx, const mtip_cdouble* coeff, mtip_cdouble* grid);
/* inverse transform and, on the grid it produced, the forward transform of prologue(grid) -- inverse_harmonic_transform then
 * [square_grid, misk.py:159-168, then] harmonic_transform, the way three links of a phasing step chain them
 * (reconstruct.py:518-528, 576-593): grid = iSHT(coeff), coeff_out = SHT(grid) (prologue 0) or SHT(|grid|^2) (prologue 1).
 * One kernel per shell where the angular grid allows it (csrc/k_sht_chain.hip; profile family "sht_chain"), else the two
 * transforms one after the other. */
int mtip_op_sht_inverse_forward(mtip_ctx* ctx, const mtip_cdouble* coeff, mtip_cdouble* grid, mtip_cdouble* coeff_out, int prologue);
int mtip_op_hankel(mtip_ctx* ctx, const mtip_cdouble* coeff_in, mtip_cdouble* coeff_out, int inverse);
/* the difference variant of the Hankel step, through the launcher the one-pass ft_stab step uses (csrc/k_hankel.hip, SUB):
 * coeff_out = H(coeff_in - coeff_sub) above output shell 0 and H(coeff_in) on shell 0, for the restarts whose byte of sub_mask
 * (n_batch bytes) is non-zero; the others get H(coeff_in).  sub_mask NULL: every restart subtracts.  MTIP_ESTATE when the
 * Hankel kernel in use has no difference variant. */
int mtip_op_hankel_difference(mtip_ctx* ctx, const mtip_cdouble* coeff_in, const mtip_cdouble* coeff_sub, mtip_cdouble* coeff_out,
                              int inverse, const uint8_t* sub_mask);
int mtip_op_fourier_transform(mtip_ctx* ctx, const mtip_cdouble* grid_in, mtip_cdouble* grid_out, int inverse);
/* approximate_unknowns + mtip_projection (fxs_Projections.py:752-767, 832-872) on 'direct' coefficients */
int mtip_op_project_coefficients(mtip_ctx* ctx, const mtip_cdouble* Ilm, mtip_cdouble* Ilm_projected);
/* the same for coefficients of a REAL intensity, I_{l,-m} = (-1)^m conj(I_{l,m}) -- what the phasing loop always passes
 * (reconstruct.py:866-870: SHT of |F|^2).  Only the m >= 0 half is read.  With projection matrices whose imaginary part
 * is exactly zero (eigenvectors of a real B_l, fxs_invariant_tools.py:1114-1141, 1207: what the reference's cross-correlation
 * route gives; env MTIP_PROJ_REAL_TOL=t additionally drops imaginary parts below t max|V_l|, the rounding residue of its
 * `density` route) the polar factors are computed in real arithmetic; any other case takes the general path of
 * mtip_op_project_coefficients.  Same result as that function to rounding. */
int mtip_op_project_real_intensity(mtip_ctx* ctx, const mtip_cdouble* Ilm, mtip_cdouble* Ilm_projected);
/* mtip_projection with caller-supplied unknowns (fxs_Projections.py:832-849, 866-871; registry operator
 * 'mtip_projection(Ilm, unknowns)', reconstruct.py:391): U = per restart the concatenation over l = 0..L of the
 * row-major (min(2l+1, Nq), 2l+1) blocks, i.e. the layout mtip_get_unknowns reads order by order */
int mtip_op_apply_unknowns(mtip_ctx* ctx, const mtip_cdouble* Ilm, const mtip_cdouble* U, mtip_cdouble* Ilm_projected);
/* project_to_modified_intensity (fxs_Projections.py:899-909): F' = F sqrt(Re I'/|F|^2) */
int mtip_op_modulus_replacement(mtip_ctx* ctx, const mtip_cdouble* F, const mtip_cdouble* I_new, mtip_cdouble* F_new);
/* real_projection + hybrid_input_output / error_reduction + l2 error (fxs_Projections.py:110-130,
 * fxs_IO_methods.py:40-68, 97-128) using the ctx's current support of each restart */
int mtip_op_real_space_update(mtip_ctx* ctx, const mtip_cdouble* w, const mtip_cdouble* rho_prev, int method,
                              double beta, mtip_cdouble* rho_new, double* error);
int mtip_op_deg2_invariants(mtip_ctx* ctx, const mtip_cdouble* Ilm, mtip_cdouble* Bl);
/* generic y = M x used by the GPU-process boundary test (tests/test_framework_integration.py:230-400
 * of the reference: gpu_func(vects) == matrix @ vects), float64 row-major */
int mtip_op_apply_matrix(mtip_ctx* ctx, const double* matrix, const double* vects, double* out,
                         int n_rows, int n_cols, int n_vec);

/* ---- rotational alignment of reconstructions (xframe/projects/fxs/average.py:920-960 -> pysofft through
 *      externalLibraries/soft_plugin.py:64-99; conventions: oracle/alignment.py, pysofft itself is not available) ---------
 * d_table: d^l_mn(beta_b), beta_b = pi (2b+1) / 4bw, b < 2bw, bw = L + 1: (2bw, sum_l (2l+1)^2) doubles, order l at offset
 * l(4l^2-1)/3, row m = -l..l, column n = -l..l */
int mtip_set_so3_tables(mtip_ctx* ctx, int bw, const double* d_table);
/* C(alpha_j, beta_b, gamma_k) = mean over the shells r_lo <= r < r_hi of Re <ref_r, R(alpha, beta, gamma) sig_r> for every
 * restart of the batch: ref (Nq, nlm), sig (n_batch, Nq, nlm) 'direct' coefficients, C (n_batch, 2bw, 2bw, 2bw) doubles
 * indexed [alpha][beta][gamma] (soft.calc_mean_C, soft_plugin.py:82-99) */
int mtip_op_so3_correlation(mtip_ctx* ctx, const mtip_cdouble* ref, const mtip_cdouble* sig, int r_lo, int r_hi, double* C);
/* f_lm -> sum_n D^l_mn f_ln on every shell (soft.rotate_coeff, soft_plugin.py:64-79): D (n_batch, sum_l (2l+1)^2) Wigner
 * matrices in the table layout above (one rotation per restart) */
int mtip_op_rotate_coefficients(mtip_ctx* ctx, const mtip_cdouble* coeff, const mtip_cdouble* D, mtip_cdouble* out);
/* find_rotation (average.py:920-947): the correlation and, per restart, its arg-max in the order the reference reads it in --
 * arg[b] = i_beta nb^2 + i_alpha nb + i_gamma of its np.argmax over mean_C (indexed [beta, alpha, gamma], tabulated at the angles
 * whose flip alpha -> 2 pi - alpha, gamma -> 2 pi - gamma is the aligning rotation; first maximum wins), vmax[b] the maximum;
 * C (B, nb, nb, nb) as mtip_op_so3_correlation returns it, or NULL */
int mtip_op_so3_find_rotation(mtip_ctx* ctx, const mtip_cdouble* ref, const mtip_cdouble* sig, int r_lo, int r_hi, int64_t* arg,
                              double* vmax, double* C);
/* rotate (average.py:948-960) by Euler angles (alpha[b], beta of grid sample beta_index[b], gamma[b]) -- what find_rotation hands
 * out; D^l_mn is built on the device from the Wigner table (host arrays of B entries) */
int mtip_op_rotate_coefficients_grid(mtip_ctx* ctx, const mtip_cdouble* coeff, const int32_t* beta_index, const double* alpha,
                                     const double* gamma, mtip_cdouble* out);

/* ---- grid arithmetic of the averaging worker (average.py:359-627, 721-727) between the transforms: csrc/k_average.hip.  Stacks of
 * n grids (n, Nq, n_theta, n_phi) complex128; every buffer may be host memory or memory of the context's device.
 * mtip_op_grid_stats: per grid 12 doubles -- [0] sum w Re, [1..3] sum w Re {x, y, z} (the centre of mass of misk.py:295-312 is
 *   [1..3] / [0]), [4] sum w Re^2, [5] sum w (Re ref - Re)^2 (0 without ref), [6] max Re, [7] min Re, [8], [9] the sum and [10] the
 *   count of the entries numpy calls > 0 (Re > 0, or Re == 0 and Im > 0; average.py:432-435), [11] 0; w = radial_w[q] theta_w[t]
 *   (the SphericalIntegrator's weights, mathLibrary.py:1223-1237, without its 1 / volume)
 * mtip_op_grid_phase_ramp: grid b *= exp(-i sign k . c_b), k the cartesian reciprocal grid vector, c_b = centers_cartesian[b]
 *   (generate_shift_by_operator, fxs_Projections.py:1419-1444; sign -1 = opposite direction), in place
 * mtip_op_grid_combine: op 0 dst[b] = conj(a[b]); 1 dst[b] = a[b] * scalars[b]; 2 dst = sum_b a[b] (one grid); 3 dst = sum_b |a[b]|^2;
 *   4 dst[b] = (a[b] - scalars[0]) * scalars[1] (average.py:721-727); dst may be a
 * mtip_op_prtf: resolution_metrics.py:62-78 -- nd = sqrt(a1 conj(a2) / (b1 b2)), b = sqrt(Re I), with the reference's rules for
 *   vanishing b; per shell the mean (complex, (Nq)) and the standard deviation ((Nq)) over the sphere */
int mtip_op_grid_stats(mtip_ctx* ctx, const mtip_cdouble* grids, int n, const mtip_cdouble* ref, const double* radial_w,
                       const double* theta_w, double* out);
int mtip_op_grid_phase_ramp(mtip_ctx* ctx, mtip_cdouble* grids, int n, const double* centers_cartesian, double sign);
int mtip_op_grid_combine(mtip_ctx* ctx, int op, mtip_cdouble* dst, const mtip_cdouble* a, int n, const mtip_cdouble* scalars);
int mtip_op_prtf(mtip_ctx* ctx, const mtip_cdouble* a1, const mtip_cdouble* a2, const mtip_cdouble* I1, const mtip_cdouble* I2,
                 mtip_cdouble* mean, double* std_dev);
/* _fsc (resolution_metrics.py:23-33) per shell of two grids: Re sum a1 conj(a2) / sqrt(sum |a1|^2 sum |a2|^2) over the sphere,
 * 1 where the denominator vanishes; fsc (Nq) */
int mtip_op_fsc(mtip_ctx* ctx, const mtip_cdouble* a1, const mtip_cdouble* a2, double* fsc);

/* ---- upstream step `extract`: B_l -> V_l (fxs_invariant_tools.py:1079-1131, 1171-1207) -------------------------------
 * eigen-decomposition of n_mat Hermitian n x n matrices A (row-major, only their Hermitian part matters): eigvals (n_mat, n)
 * unsorted, eigvecs (n_mat, n, n) with eigenvector i of matrix k in eigvecs[k][i][:] (one eigenvector per row).  Sorting,
 * the cut to min(2l+1, Nq) pairs, clipping of negative eigenvalues and V_l = eigvecs sqrt(eigvals) are host bookkeeping. */
int mtip_op_hermitian_eig(mtip_ctx* ctx, int n, int n_mat, const mtip_cdouble* A, double* eigvals, mtip_cdouble* eigvecs);
/* the same for REAL symmetric matrices up to 128 x 128 (B_l of a real intensity has no imaginary part; the rules of
 * fxs_invariant_tools.py:1114-1131 stay on the host): LDS-resident solver, eigenvalues accurate to eps |A|_F as LAPACK's */
int mtip_op_symmetric_eig(mtip_ctx* ctx, int n, int n_mat, const double* A, double* eigvals, double* eigvecs);
/* cross-correlation -> degree-2 invariants, the step in front of the two above (csrc/k_extract.hip):
 *   dimensions 3: ccd_to_deg2_invariant_3d_back_substitution (fxs_invariant_tools.py:578-645; 60-74 the Legendre products):
 *     C_m = rfft(C)_m / n_delta (mathLibrary.py:484-490) for m = 0, stride, 2 stride, .. <= max_order, then per pair (q1, q2) from the
 *     highest order down  B_l = C_l / c_l^l,  C_m -= B_l c_l^m,  c_l^m = P_l^m(q1) P_l^m(q2) / (2l + 1)
 *   dimensions 2: ccd_to_deg2_invariant_2d (813-839): B_m = C_m
 * The sizes are those of the data (not of the context's grid): cc (n_q, n_q, n_delta) float64 (the reference takes .real),
 * b_out (max_order + 1, n_q, n_q) complex128 with the orders that are not multiples of order_stride (1 or 2) written as zeros
 * (417-419).  flags: the modify_cc switches of modify_cross_correlation (235-289) for unmasked data, applied in its order while
 * cc is read -- MTIP_CC_SUBTRACT_AVERAGE needs average_intensity (n_q); MTIP_CC_PI_PERIODICITY needs an even n_delta and
 * bad_angles (n_delta): 1 where phi < pi/2 or phi >= 3 pi/2 (267); MTIP_CC_Q1Q2_SYMMETRIC.
 * legendre (dimensions 3): (n_q, n_m (n_m + 1) / 2), n_m = max_order / stride + 1: gsl_sf_legendre_sphPlm(li stride, mi stride,
 * cos theta_q) at li (li + 1) / 2 + mi, theta_q = ewald_sphere_theta_pi (physicsLibrary.py:94-95; line 602 takes it whatever pi_in_q
 * says).  Every buffer may be host memory or memory of the context's device.  Two entry points with one parameter list:
 *   mtip_op_cc_to_deg2:      n_q <= 4096, 2 max_order <= n_delta <= 4096 and at most 64 extracted orders (max_order <= 127 at
 *                            stride 2, <= 63 at stride 1): one harmonic per lane of a wave;
 *   mtip_op_cc_to_deg2_wide: n_q <= 4096, 2 max_order <= n_delta <= 4096, max_order <= 128 and at most 129 extracted orders (the
 *                            limits of the inverse, mtip_op_deg2_to_cc): up to three harmonics per lane, the kernel instantiation
 *                            chosen from the number of extracted orders; with at most 64 of them it launches the kernel of the
 *                            first entry and returns the same bits.
 * Beyond its limits either returns MTIP_EINVAL with a message in mtip_last_error (the entry, its limits, the values it got) and
 * leaves b_out untouched. */
#define MTIP_CC_SUBTRACT_AVERAGE 1u
#define MTIP_CC_PI_PERIODICITY 2u
#define MTIP_CC_Q1Q2_SYMMETRIC 4u
int mtip_op_cc_to_deg2(mtip_ctx* ctx, int n_q, int n_delta, int max_order, int order_stride, int dimensions, uint32_t flags,
                       const double* cc, const double* average_intensity, const uint8_t* bad_angles, const double* legendre,
                       mtip_cdouble* b_out);
int mtip_op_cc_to_deg2_wide(mtip_ctx* ctx, int n_q, int n_delta, int max_order, int order_stride, int dimensions, uint32_t flags,
                            const double* cc, const double* average_intensity, const uint8_t* bad_angles, const double* legendre,
                            mtip_cdouble* b_out);
/* The same step for MASKED data (csrc/k_extract_lsq.h); mtip_op_cc_to_deg2 above stays the unmasked operator.
 * mtip_op_cc_prepare_masked: modify_cross_correlation (235-289) with a mask.  cc, cc_out (n_q, n_q, n_delta) float64; cc_mask,
 * mask_out the same shape, uint8, 1 = keep; the outputs must not alias the inputs.  flags, in the reference's order:
 *   MTIP_CC_SUBTRACT_AVERAGE, MTIP_CC_PI_PERIODICITY (values as above, mask' = mask | roll(mask, n/2)), MTIP_CC_Q1Q2_SYMMETRIC
 *   (masked mean of C(q2, q1, -Delta) and C(q1, q2, Delta), mathLibrary.py:1346-1351; mask' = either valid),
 *   MTIP_CC_INTERPOLATE_MASKED (335-351; needs phis (n_delta)): per row with a valid sample every masked one becomes the linear
 *   interpolation between its nearest valid neighbours in index order; rows without a valid sample keep their values; mask_out is
 *   all 1 afterwards (287).  status[0] counts the rows that have a masked sample outside their valid ones (scipy's interp1d raises
 *   ValueError there; such samples keep their values and the caller must not use the result), status[1] is the first such pair
 *   (q1 n_q + q2; INT32_MAX when there is none).
 * mtip_op_cc_lstsq_deg2: ccd_to_deg2_invariant_3d_least_squares (452-517, 76-97).  Per pair B = argmin |F[valid] B - cc[valid]|_2,
 *   F[Delta, k] = P_{orders[k]}(cos t1 cos t2 + sin t1 sin t2 cos Delta) / 4 pi, by Householder reflections (no normal
 *   equations).  orders (n_orders) int32, strictly increasing, <= 127; cos_sin_theta (2, n_q): cos and sin of theta_q =
 *   ewald_sphere_theta_pi, and cos_delta (n_delta) = cos(phis), both as the host library rounds them (dP_l/dx reaches l (l+1) / 2:
 *   the tables are inputs so that F is the reference's to the last bit, which the kernel's recurrence then keeps);
 *   b_out (orders[n_orders - 1] + 1, n_q, n_q) complex128, the orders that are not listed as zeros; n_valid (n_q, n_q) int32;
 *   rcond (n_q, n_q): min |r_kk| / max |r_kk| of the triangle, 0 for a pair with fewer valid samples than orders.  A pair with
 *   rcond = 0 (no valid sample among them, 515-516) gets zeros; rank deficiency is the caller's to reject.
 * Both: n_q <= 4096, n_delta <= 4096, at most 64 orders, else MTIP_EINVAL with a message and untouched outputs; every buffer may
 * be host memory or memory of the context's device (a host array gets device scratch: MTIP_ENOMEM with a message if that fails). */
#define MTIP_CC_INTERPOLATE_MASKED 8u
int mtip_op_cc_prepare_masked(mtip_ctx* ctx, int n_q, int n_delta, uint32_t flags, const double* cc, const uint8_t* cc_mask,
                              const double* average_intensity, const uint8_t* bad_angles, const double* phis, double* cc_out,
                              uint8_t* mask_out, int32_t* status);
int mtip_op_cc_lstsq_deg2(mtip_ctx* ctx, int n_q, int n_delta, int n_orders, const int32_t* orders, const double* cc,
                          const uint8_t* cc_mask, const double* cos_sin_theta, const double* cos_delta, mtip_cdouble* b_out, int32_t* n_valid,
                          double* rcond);
/* mtip_op_cc_lstsq_deg2_minnorm: the same fit with LAPACK's answer for rank-deficient pairs (numpy.linalg.lstsq with rcond = None,
 * fxs_invariant_tools.py:513).  The kernel of mtip_op_cc_lstsq_deg2 runs first and unchanged: a pair it solves at full rank
 * (n_valid >= n_orders and rcond >= 1e-12) keeps the same bits and gets rank = n_orders.  The pairs it leaves, 0 < n_valid <
 * n_orders or rcond < 1e-12, are compacted into a list for a second kernel: the same Householder reduction, then a one-sided
 * Jacobi on the rows of the triangle (a trapezoid when n_valid < n_orders) with the right-hand side riding along, and
 *   x = sum_{sigma_i > cut} v_i (u_i^T c) / sigma_i,  cut = eps max(n_valid, n_orders) sigma_max;
 * rank (n_q, n_q) int32 counts the kept singular values there; a pair without a valid sample gets zeros and rank 0.  n_valid and
 * rcond come back as from mtip_op_cc_lstsq_deg2.  Known limit, unchanged: a pair whose unpivoted triangle estimate is >= 1e-12
 * while sigma_min / sigma_max lies below the cut counts as full rank.  Limits, buffers and errors as for mtip_op_cc_lstsq_deg2. */
int mtip_op_cc_lstsq_deg2_minnorm(mtip_ctx* ctx, int n_q, int n_delta, int n_orders, const int32_t* orders, const double* cc,
                                  const uint8_t* cc_mask, const double* cos_sin_theta, const double* cos_delta, mtip_cdouble* b_out,
                                  int32_t* n_valid, double* rcond, int32_t* rank);
/* The stages of modify_cross_correlation (235-289) around those of mtip_op_cc_prepare_masked (csrc/k_extract_cond.h), whole-array
 * passes over cc (n_q, n_q, n_delta) float64.  Shared: n_q <= 4096, n_delta <= 4096, else MTIP_EINVAL with a message and untouched
 * outputs; an output must not alias its input; every buffer may be host memory or memory of the context's device;
 * average_intensity (n_q) may be null, otherwise I(q1) I(q2) is subtracted while cc is read (245-247: the subtraction comes before
 * anything else, so the first stage that runs takes it).  None of the three reads or changes a mask, except the binned mean.
 * mtip_op_cc_lowpass_q: low_pass_order_in_q (248-252): scipy.signal.sosfilt of ONE second-order section, zero initial state,
 *   along axis 0 and then along axis 1.  sos: the six numbers b0 b1 b2 a0 a1 a2 with a0 = 1, as
 *   scipy.signal.butter(1, value, 'lp', fs = n_q, output = 'sos')[0] gives them.
 * mtip_op_cc_harmonic_filter: enforce_max_order / enforce_zero_odd_harmonics (253-263): per pair irfft(Z rfft(row) / n, n) n, Z
 *   zeroing the harmonics above max_order (max_order < 0: no such cut) and, with zero_odd != 0, the odd ones; at least one of the
 *   two must be asked for; n_delta >= 2, even or odd.
 * mtip_op_cc_binned_mean: apply_binned_mean (281-283, binned_mean 308-332).  The row is rolled by n_roll (numpy.roll) and cut
 *   into n_bins runs, bin b holding the rolled samples bin_start[b] .. bin_start[b + 1] - 1; bin_start (n_bins + 1) int32 must rise
 *   strictly from 0 to n_delta, and 0 <= n_roll < n_delta: the caller forms both with the reference's expressions (312-323), the
 *   kernel never recomputes a bin edge.  cc_out (n_q, n_q, n_bins): the mean of the valid samples of the bin; mask_out the same
 *   shape, uint8: 1 where the bin has a valid sample; a bin without one gets the value 0 and mask 0 (329). */
int mtip_op_cc_lowpass_q(mtip_ctx* ctx, int n_q, int n_delta, const double* sos, const double* cc, const double* average_intensity,
                         double* cc_out);
int mtip_op_cc_harmonic_filter(mtip_ctx* ctx, int n_q, int n_delta, int max_order, int zero_odd, const double* cc,
                               const double* average_intensity, double* cc_out);
int mtip_op_cc_binned_mean(mtip_ctx* ctx, int n_q, int n_delta, int n_bins, const int32_t* bin_start, int n_roll, const double* cc,
                           const uint8_t* cc_mask, const double* average_intensity, double* cc_out, uint8_t* mask_out);
/* The other back-substitution modes of ccd_to_deg2_invariant_3d (csrc/k_extract_psd.h; mode table fxs_invariant_tools.py:440).
 * mtip_op_nearest_psd: nearest_positive_semidefinite_matrix (mathLibrary.py:872-892, limit = 0) of a stack.  A, out (n_mat, n, n)
 *   complex128, row major, out must not alias A; only the Hermitian part H = (A + A^+) / 2 counts (878); n_clipped (n_mat) int32:
 *   the eigenvalues set to zero.  All on the device: H and sigma = |H|_F, the one-sided Jacobi of mtip_op_hermitian_eig on
 *   H + sigma 1 (positive semi-definite: no +x / -x eigenvalue pairs, so no repeat and nothing per matrix through the host;
 *   eigenvalues to eps |H|_F absolute, as LAPACK's), out = sum_k max(lambda_k, 0) v_k v_k^+, Hermitian to the bit.
 *   1 <= n <= 1024, else MTIP_EINVAL with the limit and the value in the message and untouched outputs.
 * mtip_op_cm_backsub: back-substitution on harmonic coefficients.  cm (max_order + 1, n_q, n_q) complex128, order major: what
 *   mtip_op_cc_to_deg2[_wide] writes with dimensions = 2 and order_stride = 1; qq_mask (n_q, n_q) uint8, 1 = keep, or null;
 *   b_out (max_order + 1, n_q, n_q), the orders that are not multiples of order_stride (1 or 2) as zeros; must not alias cm.
 *   mode MTIP_BS_PLAIN: back_substitution (mathLibrary.py:1509-1517) on the harmonics m = 0, stride, .. per pair, from the highest
 *     order down  B_l = C_l / c_l^l,  C_m -= B_l c_l^m;  masked pairs are zeroed first (fxs_invariant_tools.py:560): the mode
 *     back_substitution_memory_hungry (519-576).  With the flag MTIP_BS_HERMITIAN_MEAN  C_m = (C_m + C_m^+) / 2 over (q1, q2) before
 *     that (688-690): back_substitution_qqsym (646-694).  legendre as for mtip_op_cc_to_deg2 at order_stride; info is not touched.
 *     n_q <= 4096.
 *   mode MTIP_BS_PSD: back_substitution_psd (710-761).  Every C_m becomes its nearest PSD matrix (755), masked pairs are zeroed
 *     (759), then psd_back_substitution (mathLibrary.py:1499-1507) over ALL orders from max_order down:
 *     B_l = nearest_psd(C_l / c_l^l),  C_m -= B_l c_l^m (m < l);  b_out gets the orders that are multiples of order_stride (760).
 *     legendre is the table at stride 1, (n_q, (max_order + 1)(max_order + 2) / 2).  info (max_order + 1) int32: eigenvalues
 *     clipped at step l.  Per order two launches -- the eigen-decomposition and one kernel that rebuilds B_l, updates every lower
 *     harmonic and prepares the next input with its shift -- and nothing crosses to the host between the steps.  n_q <= 1024.
 *   Both: max_order <= 128; beyond the limits MTIP_EINVAL with the limit and the values in the message and untouched outputs;
 *   every buffer may be host memory or memory of the context's device. */
#define MTIP_BS_PLAIN 0
#define MTIP_BS_PSD 1
#define MTIP_BS_HERMITIAN_MEAN 1u
int mtip_op_nearest_psd(mtip_ctx* ctx, int n, int n_mat, const mtip_cdouble* A, mtip_cdouble* out, int32_t* n_clipped);
int mtip_op_cm_backsub(mtip_ctx* ctx, int n_q, int max_order, int order_stride, int mode, uint32_t flags, const mtip_cdouble* cm,
                       const double* legendre, const uint8_t* qq_mask, mtip_cdouble* b_out, int32_t* info);
/* degree-2 invariants -> cross-correlation, the inverse of mtip_op_cc_to_deg2 and the back half of the worker `simulate_ccd`
 * (csrc/k_simulate.h; fxs_invariant_tools.py:941-990 deg2_invariant_to_cc_3d, 934-939 deg2_invariant_to_cc_2d).
 * bl (max_order + 1, n_q, n_q) complex128.
 *   MTIP_SIM_BACK_SUBSTITUTION, dimensions 3 (979-988, 60-74): C_n = sum_{l >= n} B_l T_l^n(q1) T_l^n(q2) / (2l + 1), n = 0 .. max_order,
 *     then irfft(C_n 2 max_order, 2 max_order) (the imaginary parts of C_0 and C_max_order are dropped, as numpy does): cc_out
 *     (n_q, n_q, n_delta) float64 with n_delta = 2 max_order.  legendre_t ((max_order + 1) (max_order + 2) / 2, n_q):
 *     gsl_sf_legendre_sphPlm(l, n, cos theta_q) at row l (l + 1) / 2 + n, theta_q = ewald_sphere_theta_pi (962).
 *   MTIP_SIM_BACK_SUBSTITUTION, dimensions 2 (934-939): irfft(B_m size, size) along the order axis, size = n_delta = 2 max_order.
 *   MTIP_SIM_LSTSQ, dimensions 3 (963-971, 76-97, 992-1001): cc_out (n_q, n_q, n_delta) complex128 (Im B_l is kept),
 *     C = sum_l B_l / (4 pi) P_l(cos t1 cos t2 + sin t1 sin t2 cos Delta) for the first n_delta / 2 + 1 samples (Delta <= pi), sample
 *     j = 1 .. n_delta / 2 - 1 also written to n_delta - j (the mirror [1:-1][::-1] of 971; n_delta must be even).  cos_sin_theta
 *     (2, n_q), cos_delta (n_delta / 2 + 1) as the host library rounds them.
 * Built for n_q <= 4096, 1 <= max_order <= 128, n_delta <= 4096: beyond that MTIP_EINVAL with a message and untouched outputs.
 * Every buffer may be host memory or memory of the context's device; host bl / cc_out get device copies, and when these do not fit
 * the free device memory the call returns MTIP_ENOMEM with the sizes in the message before anything is allocated. */
#define MTIP_SIM_BACK_SUBSTITUTION 0
#define MTIP_SIM_LSTSQ 1
int mtip_op_deg2_to_cc(mtip_ctx* ctx, int n_q, int max_order, int n_delta, int dimensions, int mode, const mtip_cdouble* bl,
                       const double* legendre_t, const double* cos_sin_theta, const double* cos_delta, void* cc_out);

/* ---- correlate: polar patterns -> averaged two-point cross-correlation C(q1, q2, Delta) (csrc/k_correlate.h) ----------------
 * The first stage of the fxs chain (xframe/projects/fxs/correlate.py:401-452, 347-355, 249-270 and all of
 * projectLibrary/cross_correlation.py) from the polar resampling on: images (n_patterns, n_q, n_phi) float64 and masks
 * (n_patterns, n_q, n_phi) uint8 with values 0 / 1 are what process_image holds at line 398.  A handle owns the accumulators
 * sum (n_q1, n_q2, n_phi) float64 and count (same shape) int32 on the context's device; its size is checked against the free
 * device memory at create (a null return; the message in mtip_last_error names the size).
 * cfg: filter_kind 1 = intensity_radial_pixel_filter 'average_sigma' with filter_k sigmas, 2 = 'median_mad' with filter_k median
 * absolute deviations (correlate.py:405-406, 471-474; exact order statistics, csrc/k_ringfilter.h), 0: none; any other value is a
 * null return whose message names the three.  The ROI mean runs over the
 * rings [roi_lo, roi_hi) where mask == 1: roi_filter rejects a pattern whose mean is outside [roi_min, roi_max], roi_normalize
 * divides the image by it; factor (n_q, n_phi) or NULL: polarisation x solid-angle table (565-591) multiplied in afterwards.
 * shared_mask: the mask is the same for every pattern (ignored with a filter, which makes it per pattern): masks is then
 * (n_q, n_phi), the mask of the first batch is the handle's, and its pair counts M are computed once.
 * q1_pos (n_q1), q2_pos (n_q2): the selected rings.  n_phi: 16, 32, .. 1024 (a power of two; more through mtip_correlate_create_ex).
 * Per good pattern  sum += D / M, count += 1  where |M| >= 0.5, with D = irfft(conj F[q1] F[q2]), M = irfft(conj G[q1] G[q2]),
 * F = rfft(image), G = rfft(mask).  (The reference tests M != 0 on a rounded integer: the one deliberate deviation.)
 * Every buffer of add / get_partial / merge / finalize may be host memory or memory of the context's device. */
typedef struct mtip_correlate mtip_correlate;
typedef struct {
    int32_t n_q, n_phi, n_q1, n_q2;
    int32_t filter_kind, roi_lo, roi_hi, roi_filter, roi_normalize, shared_mask;
    double filter_k, roi_min, roi_max;
} mtip_correlate_cfg;
mtip_correlate* mtip_correlate_create(mtip_ctx* ctx, const mtip_correlate_cfg* cfg, const int32_t* q1_pos, const int32_t* q2_pos,
                                      const double* factor);
/* create with flags.  0: mtip_correlate_create.  MTIP_CORRELATE_GENERAL_NPHI: n_phi is any even length in 16 .. 2048 whose only prime
 * factors are 2, 3 and 5 (1536, the reference's default, 1920, 2000, 2048 ..): mixed-radix transforms (radices 4, 2, 3, 5) by a plan
 * made once per handle; a power of two up to 1024 runs the same kernels as without the flag and gives the same bits.  A refused
 * length (odd, below 16, above 2048, a prime factor above 5) is a null return whose message states the rule and the nearest accepted
 * lengths below and above; so is any other flag bit (the message names `flags`).  add, add_detector, get_partial, merge and finalize
 * take either kind of handle.
 * MTIP_CORRELATE_ANY_NPHI (alone or with the bit above: the same): n_phi is any even length in 16 .. 2048, the ring pixel counts of
 * phi_range's 'max' and 'min' modes among them (1256 = 2^3 157, 1030 = 2 5 103 ..).  A power of two up to 1024 and a length with
 * prime factors 2, 3, 5 only run the kernels and give the bits of the handles above; every other length runs chirp-z (Bluestein)
 * transforms: a circular convolution of the smallest 2-3-5-smooth length >= n_phi - 1 by the same mixed-radix stages, its tables
 * made once per handle.  Refused, with the rule and the value in the message, before anything is allocated: an odd length, one
 * below 16 or above 2048.  Partial results merge between handles of one shape whatever their kind. */
#define MTIP_CORRELATE_GENERAL_NPHI 1u
#define MTIP_CORRELATE_ANY_NPHI 4u
mtip_correlate* mtip_correlate_create_ex(mtip_ctx* ctx, const mtip_correlate_cfg* cfg, const int32_t* q1_pos, const int32_t* q2_pos,
                                         const double* factor, uint32_t flags);
void mtip_correlate_destroy(mtip_correlate* h);
/* one batch: flags and waxs rows are decided on the device and kept by the handle; patterns are accumulated in pattern order, so
 * the same patterns give bit-identical sum and count however they are split into batches */
int mtip_correlate_add(mtip_correlate* h, int n_patterns, const double* images, const uint8_t* masks);
/* patterns added or merged so far (a negative error code for a null handle) */
int mtip_correlate_num_patterns(mtip_correlate* h);
/* the additive partial result: sum, count (n_q1, n_q2, n_phi), is_good (n_patterns) int32, waxs (n_patterns, n_q); NULL: skipped */
int mtip_correlate_get_partial(mtip_correlate* h, double* sum, int32_t* count, int32_t* is_good, double* waxs);
/* add another handle's partial result (its patterns are appended) */
int mtip_correlate_merge(mtip_correlate* h, const double* sum, const int32_t* count, int n_patterns, const int32_t* is_good,
                         const double* waxs);
/* ccf = sum / count, NaN where count = 0; symmetrize != 0: symmetrize_ccf with the three positions; ccf (n_q1, n_q2, n_phi) and / or
 * fc = fft(ccf)[..., :fc_n_max] (n_q1, n_q2, fc_n_max); a NULL output is skipped */
int mtip_correlate_finalize(mtip_correlate* h, int symmetrize, int pos_pi2, int pos_pi, int pos_3pi2, int fc_n_max, double* ccf,
                            mtip_cdouble* fc);

/* The median_mad statistics and filter alone (csrc/k_ringfilter.h; correlate.py:471-474 i_median_and_mad, 412 the filter), row by
 * row: images (n_rows, n_phi) float64, masks (n_rows, n_phi) uint8.  Over a row's valid samples (mask != 0, value not NaN; n of them),
 * v sorted: median = v[n / 2] for odd n, (v[n / 2 - 1] + v[n / 2]) / 2 for even n, mad the same rule on |x - median|, NaN for n = 0:
 * np.nanmedian and scipy.stats.median_abs_deviation(nan_policy='omit') bit for bit.  masks_out = mask && !(|x - median| > k mad).
 * median, mad (n_rows) and masks_out (n_rows, n_phi): a NULL output is skipped.  1 <= n_phi <= 2048 (any length: there is no
 * transform) and n_rows >= 1, else MTIP_EINVAL with the limits in the message.  Valid samples are finite or NaN with |x| < 1e300;
 * infinities are out of contract.  Host or device buffers. */
int mtip_op_ring_median_mad(mtip_ctx* ctx, int n_rows, int n_phi, const double* images, const uint8_t* masks, double k, double* median,
                            double* mad, uint8_t* masks_out);

/* ---- correlate, the Cartesian stage: detector frames -> polar patterns (csrc/k_resample.h) ------------------------------------
 * process_image 377-398 of xframe/projects/fxs/correlate.py per pattern: mask = 0 where image < threshold_lo or image >
 * threshold_hi (threshold_on; tested on the raw image), mask *= (binary_mask != 0), image -= background, image *= mask, then
 * scipy.ndimage.map_coordinates(., [cart_x, cart_y], order, mode='constant', cval=0, prefilter=True) of the image (float64 out)
 * and of the mask (an integer array: rounded half away from zero, uint8 out).  cart_x indexes axis 0 (H), cart_y axis 1 (W); the
 * n_points points need not form a grid.  Orders 0 .. 5; 2 <= H, W <= 4096 (beyond: a null return from create with a message).
 * binary_mask (H, W) uint8, background (H, W) float64, each NULL unless its has_ flag is set; they and the coordinates are copied.
 * run: images (n_patterns, H, W) float32 (is_float32 != 0) or float64; masks (n_patterns, H, W) uint8 0 / 1: the initial masks, or
 * NULL for ones.  With the threshold off and masks NULL the Cartesian mask is the same for every pattern: it is resampled once per
 * handle by the same kernels.  images_out (n_patterns, n_points) float64 and masks_out (n_patterns, n_points) uint8 are what
 * mtip_correlate_add takes; *n_bad_mask (host memory, may be NULL) counts rounded mask values other than 0 / 1 (they are stored
 * as their low byte).  Every other buffer may be host memory or memory of the context's device; work runs on the context's stream. */
typedef struct mtip_resample mtip_resample;
typedef struct {
    int32_t H, W, order, threshold_on, has_binary_mask, has_background;
    int64_t n_points;
    double threshold_lo, threshold_hi;
} mtip_resample_cfg;
mtip_resample* mtip_resample_create(mtip_ctx* ctx, const mtip_resample_cfg* cfg, const double* cart_x, const double* cart_y,
                                    const uint8_t* binary_mask, const double* background);
void mtip_resample_destroy(mtip_resample* h);
int mtip_resample_run(mtip_resample* h, int n_patterns, const void* images, int is_float32, const uint8_t* masks, double* images_out,
                      uint8_t* masks_out, int64_t* n_bad_mask);
/* run into buffers on the device, then mtip_correlate_add of them: bit-identical to the two calls.  The resample handle's points are
 * the correlate handle's (n_q, n_phi) grid.  A rounded mask value other than 0 / 1 is MTIP_EINVAL and nothing is accumulated; so is
 * a shared_mask correlate handle where the mask is not static (threshold on, or masks given). */
int mtip_correlate_add_detector(mtip_correlate* h, mtip_resample* resample, int n_patterns, const void* images, int is_float32,
                                const uint8_t* masks, int64_t* n_bad_mask);

/* ---- the 2-D (polar) variant, operator level --------------------------------------
 * Grids (n_batch, Nq, n_phi) complex128 with n_phi = 2 M + 1 (harmonic_transforms.py:44-47); harmonic coefficients in numpy's
 * FFT order (orders 0..M, -M..-1); coefficients of the real transform (n_batch, Nq, M + 1).  Buffers: host or device memory. */
typedef struct mtip2d_ctx mtip2d_ctx;
mtip2d_ctx* mtip2d_create(int n_radial, int n_phi, int n_batch, int device);
void mtip2d_destroy(mtip2d_ctx* ctx);
const char* mtip2d_last_error(const mtip2d_ctx* ctx);
/* forward / inverse weights (Nq summed, Nq new, n_phi orders) as assemble_weights_mid returns them (hankel_transforms.py:300-362),
 * unused_orders (n_phi): 1 = zeroed by the transform pair (generate_polar_ht, 613-628) */
int mtip2d_set_hankel_weights(mtip2d_ctx* ctx, const mtip_cdouble* forward, const mtip_cdouble* inverse, const uint8_t* unused_orders);
/* the 2-D reciprocal projection (fxs_Projections.py:723-745, 803-826, 855-863): order_ids (n_used, ascending, 0 included),
 * projection vectors (n_used, Nq), their radial masks (n_used, Nq), reciprocal radial points (Nq), number of particles */
int mtip2d_set_projection(mtip2d_ctx* ctx, int n_used, const int32_t* order_ids, const mtip_cdouble* projection_vectors,
                          const uint8_t* radial_mask, const double* radial_points, double n_particles);
/* projections.reciprocal.SO_freedom for dimensions == 2 (fxs_Projections.py:744-750, 933-971): the unknown at `position` among the
 * used orders is set to 1 in every projection; -1 switches it off (mtip2d_set_projection resets it) */
int mtip2d_set_so_freedom(mtip2d_ctx* ctx, int position);
/* circularHarmonicTransform_complex_forward / _inverse (mathLibrary.py:469-483) */
int mtip2d_op_harmonic(mtip2d_ctx* ctx, const mtip_cdouble* in, mtip_cdouble* out, int inverse);
/* circularHarmonicTransform_real_forward (485-491: of the real part of a complex grid) / _real_inverse (493-496: real grid out) */
int mtip2d_op_real_harmonic_forward(mtip2d_ctx* ctx, const mtip_cdouble* grid, mtip_cdouble* coeff);
int mtip2d_op_real_harmonic_inverse(mtip2d_ctx* ctx, const mtip_cdouble* coeff, double* grid);
/* generate_polar_ht (hankel_transforms.py:629-640) and generate_ft for dimensions = 2 (fourier_transforms.py:57-88) */
int mtip2d_op_hankel(mtip2d_ctx* ctx, const mtip_cdouble* in, mtip_cdouble* out, int inverse);
int mtip2d_op_fourier_transform(mtip2d_ctx* ctx, const mtip_cdouble* in, mtip_cdouble* out, int inverse);
/* approximate_unknowns + mtip_projection + the number-of-particles rule on coefficients of the real transform; unknowns
 * (n_batch, n_used) or NULL */
int mtip2d_op_project(mtip2d_ctx* ctx, const mtip_cdouble* I, mtip_cdouble* I_projected, mtip_cdouble* unknowns);
/* ---- the operators of the 2-D phasing loop (the schedule, ramps, support bookkeeping and best tracking are host logic) ---- */
int mtip2d_set_real_constraints(mtip2d_ctx* ctx, uint32_t flags, double value_lo, double value_hi, double imag_threshold, uint32_t hio_flags);
/* (Nq, n_phi) weights of l2_projection_diff: PolarIntegrator weights (mathLibrary.py:1242-1265) times the metric's mask */
int mtip2d_set_error_weights(mtip2d_ctx* ctx, const double* weights);
/* one HIO (0) / ER (1) step, optionally with the ft_stab add-back (sketches reconstruct.py:518-528, 576-593): rho, support
 * (n_batch, Nq, n_phi) in; F' and the new density, the error per restart and the unknowns (n_batch, n_used; or NULL) out */
int mtip2d_op_step(mtip2d_ctx* ctx, int method, int ft_stab, double beta, const mtip_cdouble* rho, const uint8_t* support,
                   mtip_cdouble* F_new, mtip_cdouble* rho_new, double* err, mtip_cdouble* unknowns);
/* the same with the loop's sub-variants: method 2 / 3 = HIO_non_FXS / ER_non_FXS (sketch MTIP_start_non_FXS, reconstruct.py:530-535,
 * 899-904: F' = F sqrt(fixed / |F|^2) with fixed_intensity (n_batch, Nq, n_phi), no harmonic transform, no unknowns), and the inputs
 * of the reciprocal error metrics (fxs_IO_methods.py:301-310, 370-400) when asked for: F_out = FT(rho) (n_batch, Nq, n_phi), I_out =
 * the harmonic coefficients of |F|^2 (n_batch, Nq, M + 1; FXS methods only); any of fixed_intensity / F_out / I_out / unknowns
 * may be NULL */
int mtip2d_op_step_ex(mtip2d_ctx* ctx, int method, int ft_stab, double beta, const mtip_cdouble* rho, const uint8_t* support,
                      const double* fixed_intensity, mtip_cdouble* F_new, mtip_cdouble* rho_new, double* err, mtip_cdouble* unknowns,
                      mtip_cdouble* F_out, mtip_cdouble* I_out);
/* the SW sketch (reconstruct.py:598-605, fxs_Projections.py:245-258, 294-298): support mask (n_batch, Nq, n_phi) from rho */
int mtip2d_op_shrinkwrap(mtip2d_ctx* ctx, const mtip_cdouble* rho, double sigma, double threshold, uint8_t* mask);

/* ---- the resident 2-D loop (csrc/k_polar2d.hip, second half): the batch of restarts stays in HBM, a step is five fused kernels and
 * nothing crosses the host inside mtip2d_run*.  The calls mirror the 3-D ones above; the operator-level calls keep working beside
 * them (they share work grids on the context's stream, not the state).  A call in the wrong state returns MTIP_ESTATE with a
 * message and enqueues nothing. */
/* starting density of restart `batch` (Nq, n_phi) (reconstruct.py:957-966); mtip2d_init_state then starts the state from
 * F0 = FT(rho0), rho0' = IFT(F0) (962-963), best error = inf, supports = the initial support, empty histories */
int mtip2d_set_density(mtip2d_ctx* ctx, int batch, const mtip_cdouble* rho);
/* initial support S0 (Nq, n_phi) bytes, shared by the batch (fxs_Projections.py:60-93); resets every restart's support to it */
int mtip2d_set_initial_support(mtip2d_ctx* ctx, const uint8_t* support);
/* effective support of one restart (the support setter's result, fxs_Projections.py:53-58) */
int mtip2d_set_support(mtip2d_ctx* ctx, int batch, const uint8_t* support);
int mtip2d_init_state(mtip2d_ctx* ctx);
/* ft_stab per restart for the runs that follow with ft_stab = 1 (reconstruct.py:836-850: one decision per reconstruction
 * process); NULL = every restart.  Read inside the step: the step is not run twice. */
int mtip2d_set_ft_stab_mask(mtip2d_ctx* ctx, const uint8_t* mask);
/* reciprocal metrics evaluated in every step: which = 1 deg2_invariant_l2_diff (2-D flavour, fxs_IO_methods.py:370-400;
 * deg2_reference (n_used, Nq, Nq) with the number-of-particles rule already applied, deg2_norms (n_used): value -1 where 0) |
 * 2 l2_projection_diff of (F, F') (301-310) with l2_weights (Nq, n_phi); 0 switches them off */
int mtip2d_set_reciprocal_metrics(mtip2d_ctx* ctx, uint32_t which, const mtip_cdouble* deg2_reference, const double* deg2_norms,
                                  const double* l2_weights);
/* generate_main_error_routine (fxs_IO_methods.py:746-765): type 0 mean, 1 min, 2 max, 3 prod over the listed metrics, items[i] =
 * 0 real l2_projection_diff, 1 deg2_invariant_l2_diff (one value per used order), 2 reciprocal l2_projection_diff; a scalar next
 * to the per-order metric is refused (the reference raises, 758).  Default: the real metric alone. */
int mtip2d_set_main_error(mtip2d_ctx* ctx, int type, int n_items, const int32_t* items);
/* n_steps steps of method 0 HIO, 1 ER, 2 HIO_non_FXS, 3 ER_non_FXS (reconstruct.py:854-951) for every restart, betas[n_steps];
 * errors, reciprocal metrics, main error and best tracking (934-938) stay on the device.  The *_non_FXS methods take |F| of the
 * pair before the most recent step as their intensity, once per block of such runs (899-904: an FXS run or a new sub-loop drops it).
 * mtip2d_run returns after real_err (n_steps x n_batch, may be NULL) is on the host; mtip2d_run_async only enqueues. */
int mtip2d_run(mtip2d_ctx* ctx, int method, int ft_stab, int n_steps, const double* betas, double* real_err);
int mtip2d_run_async(mtip2d_ctx* ctx, int method, int ft_stab, int n_steps, const double* betas);
/* histories of the steps [first_step, first_step + n_steps): the real l2_projection_diff (fxs_IO_methods.py:97-128), the main
 * error (746-765), the reciprocal metrics (deg2 (n_steps, n_batch, n_used) and / or l2 (n_steps, n_batch); NULL = not wanted) */
int mtip2d_fetch_errors(mtip2d_ctx* ctx, int64_t first_step, int64_t n_steps, double* real_err);
int mtip2d_fetch_main_errors(mtip2d_ctx* ctx, int64_t first_step, int64_t n_steps, double* main_err);
int mtip2d_fetch_reciprocal_metrics(mtip2d_ctx* ctx, int64_t first_step, int64_t n_steps, double* deg2, double* l2);
/* one shrink-wrap update of the resident density (reconstruct.py:598-605, 877-885; fxs_Projections.py:245-258, 294-298):
 * enforce_b = last main error_b > error_limit, taken on the device (no step yet: not enforced); enforced[n_batch] or NULL */
int mtip2d_shrinkwrap(mtip2d_ctx* ctx, double sigma, double threshold, double error_limit, uint8_t* enforced);
/* 'SW_center' tail (reconstruct.py:606-613, 886-897), literally: the latest pair becomes (reciprocal, real) = (rho, FT(rho)) */
int mtip2d_refresh_reciprocal_density(mtip2d_ctx* ctx);
/* top of a sub-loop (reconstruct.py:852-866): the stale pair is re-read from the state, the *_non_FXS intensity forgotten */
int mtip2d_begin_sub_loop(mtip2d_ctx* ctx);
/* take the best pair and its support as the latest ones (reconstruct.py:945-949), for all restarts or those with select[b] != 0 */
int mtip2d_select_best(mtip2d_ctx* ctx);
int mtip2d_select_best_where(mtip2d_ctx* ctx, const uint8_t* select);
/* which = 0 latest, 1 best (reconstruct.py:934-938); (Nq, n_phi) per restart */
int mtip2d_get_density(mtip2d_ctx* ctx, int batch, int which, mtip_cdouble* rho);
int mtip2d_get_reciprocal_density(mtip2d_ctx* ctx, int batch, int which, mtip_cdouble* F);
int mtip2d_get_support(mtip2d_ctx* ctx, int batch, int which, uint8_t* support);
/* unknowns (n_used) of the last FXS step (fxs_Projections.py:723-745) */
int mtip2d_get_unknowns(mtip2d_ctx* ctx, int batch, mtip_cdouble* unknowns);
/* best main error per restart (n_batch doubles, reconstruct.py:934-938) and the number of steps done; either may be NULL */
int mtip2d_get_best_error(mtip2d_ctx* ctx, double* best_error, int64_t* n_steps_done);
int mtip2d_synchronize(mtip2d_ctx* ctx);

/* ---- averaging of 2-D reconstructions (average.py:123-358, run_2d; csrc/k_average2d.h).  Stacks are (n, n_radial, n_phi)
 *      complex128 of any length n; every array argument may be host or device memory. ---- */
/* radial points of the real and the reciprocal grid, and the PolarIntegrator's weights (mathLibrary.py:1254-1262) as factors:
 * w_r[q] = trapezoid weight x r on the real grid, w_q the same on the reciprocal grid, w_phi the trapezoid weights in phi */
int mtip2d_avg_set_grid(mtip2d_ctx* ctx, const double* rs, const double* qs, const double* w_r, const double* w_q, const double* w_phi);
/* out (n, 9) per grid: [0] integral of Re, [1], [2] integrals of Re x, Re y, [3] largest real part among the entries > 0 in
 * numpy's order on complex numbers (-inf if none), [4], [5] complex sum of those entries, [6] their count, [7] max Re,
 * [8] min Re */
int mtip2d_avg_grid_stats(mtip2d_ctx* ctx, const mtip_cdouble* grids, int n, double* out);
/* out (n, 2) per grid: integrals of |Im F - Im F_ref| and |Im F - Im conj(F_ref)| over the reciprocal grid (average.py:216-217) */
int mtip2d_avg_inversion_metric(mtip2d_ctx* ctx, const mtip_cdouble* F, int n, const mtip_cdouble* F_ref, double* out);
/* grids[b] *= exp(-i sign k . c_b) in place, c_b = centers_cartesian[2 b .. 2 b + 1] (fxs_Projections.py:1426-1434) */
int mtip2d_op_grid_phase_ramp(mtip2d_ctx* ctx, mtip_cdouble* grids, int n, const double* centers_cartesian, double sign);
/* op 0: dst[b] = conj(a[b]); 1: dst[b] = a[b] / scalars[b]; 2: dst = (sum over b of a[b]) / Re scalars[0];
 * 3: dst = (sum over b of |a[b]|^2) / Re scalars[0]; 4: dst[b] = (a[b] - Re scalars[0]) / Re scalars[1].
 * dst: a stack for 0, 1 and 4 (may be a itself), one grid for 2 and 3 */
int mtip2d_op_grid_combine(mtip2d_ctx* ctx, int op, mtip_cdouble* dst, const mtip_cdouble* a, int n, const mtip_cdouble* scalars);
/* per-shell curves of one averaged set (a_d = FT of the mean density, a_ft = mean reciprocal density, I_d, I_ft = mean
 * intensities, real values in complex grids): prtf_mean, prtf_std (4, n_radial) in the order PRTF, PRTF_from_density,
 * PRTF_from_ft_density, PRTF_ftI (average.py:250-263; resolution_metrics.py:63-79); fsc (n_radial) = _fsc(a_d, a_ft) (23-33) */
int mtip2d_avg_curves(mtip2d_ctx* ctx, const mtip_cdouble* a_d, const mtip_cdouble* a_ft, const mtip_cdouble* I_d, const mtip_cdouble* I_ft,
                      mtip_cdouble* prtf_mean, double* prtf_std, double* fsc);
/* FQCB_2D (resolution_metrics.py:146-187) of two sets of degree-2 invariants, each given as a coefficient table I_n(q) (kind 0:
 * n_radial rows of ld values, order n in column n < n_orders; B_n(q, q') = I_n(q) conj(I_n(q'))) or as a B_n stack (kind 1:
 * (n_orders, n_radial, n_radial), ld ignored): orders o_start, o_start + o_step, ... below min(n1, n2); mean, std_dev (n_radial) */
int mtip2d_avg_fqcb(mtip2d_ctx* ctx, const mtip_cdouble* in1, int kind1, int n1, int ld1, const mtip_cdouble* in2, int kind2, int n2,
                    int ld2, int o_start, int o_step, double* mean, double* std_dev);
/* out (n_orders, n_radial, n_radial): B_n(q, q') = I_n(q) conj(I_n(q')) of a coefficient table (fxs_invariant_tools.py:906-914) */
int mtip2d_op_deg2_from_table(mtip2d_ctx* ctx, const mtip_cdouble* table, int n_orders, int ld, mtip_cdouble* out);

/* ---- timing ----------------------------------------------------------------------------------- */
/* average duration (ms) and launch count of kernel family `name` ("sht_fwd", "sht_inv", "hankel",
 * "proj", "real_update", ...) measured with hipEvents on the ctx stream since the last reset;
 * enable with mtip_profile(ctx, 1). */
int mtip_profile(mtip_ctx* ctx, int enable);
int mtip_profile_get(mtip_ctx* ctx, const char* name, double* total_ms, int64_t* launches);
int mtip_profile_reset(mtip_ctx* ctx);
/* diagnostic of the last polar-factor solve, (n_batch, L+1) int32: bits 0-7 Jacobi sweeps used, bits 8+ the
 * number of columns of X_l that were still non-zero (not deflated) in the final sweep */
int mtip_debug_jacobi_sweeps(mtip_ctx* ctx, int32_t* out);
/* diagnostic: phase stamps of the chained inverse -> forward SHT kernel (csrc/k_sht_chain.hip), (3 kinds: store / modulus /
 * real-space epilogue, n_batch * n_radial shells, 18) int64 s_memtime ticks of the last launch of each kind: [0] start, [1]
 * tables staged, [2] / [3] Legendre synthesis done (wave 0 / all), then per FFT pass p (6 p + 4 ...): step 1 done, barrier,
 * epilogue + forward phase 1 done, barrier, forward phase 2 done, barrier; [16] Legendre sums done, [17] end.  The first call
 * switches the stamps on (out may be null). */
int mtip_debug_chain_timing(mtip_ctx* ctx, int64_t* out);
/* diagnostic: the launch plan of the Hankel kernel (build_hankel_tiles, csrc/k_hankel.hip): ct = 16-column MFMA tiles per
 * workgroup (1, 2, 3 or 5: the instantiation that runs), n_tiles = column tiles (grid x), n_row_blocks = blocks of 128 output
 * shells (grid y).  Any of the three may be NULL. */
int mtip_debug_hankel_tiles(mtip_ctx* ctx, int* ct, int* n_tiles, int* n_row_blocks);
/* diagnostic: the SHT kernel choice of the context (ShtPlan, csrc/mtip_internal.h; made by mtip_set_angular_grid), host only,
 * nothing is launched.  out (MTIP_SHT_PLAN_FIELDS) int32: [0] fwd (0 generic, 1 LDS, 2 register, 3 paired, 4 two-stage beyond
 * L = 63), [1] inv (0 generic, 1 LDS, 2 register, 3 wide, 4 two-stage), [2] fwd_rp, [3] fwd_th, [4] fwd_maxi, [5] inv_rp,
 * [6] inv_nsplit, [7] inv_jl, [8] real_update, [9] chain (0 off, 1 run-time tables, 2 tables in registers, 3 the L = 32
 * form), [10] chain_gsz, [11] chain_thg, [12] chain_maxi */
#define MTIP_SHT_PLAN_FIELDS 13
int mtip_debug_sht_plan(mtip_ctx* ctx, int32_t* out);
/* diagnostic: workgroups per restart of the real projection kernel (k_rproj: the host-packed slots of orders), 0 before the
 * first projection or when the general complex kernels are in use; negative = error code */
int mtip_debug_projection_slots(mtip_ctx* ctx);
/* diagnostic: in-kernel timers of the real projection kernel (k_rproj), (n_batch, L+1, MTIP_POLAR_TIMING_SLOTS = 40) int64
 * s_memtime ticks of the last projection per (restart, order): [0..4] phases X~ product, warm start, Jacobi, U, apply;
 * [5] rounds; [6], [7] start / end; [8] hardware id; [10..17] busy and [18..25] LDS drain + barrier per wave, [26..32] the
 * segments of a round of wave 0 and [33..39] of wave 5 (summed over the rounds; largest order of L = 32 only).  The first call
 * (out may be NULL) switches the timers on. */
#define MTIP_POLAR_TIMING_SLOTS 40
int mtip_debug_polar_timing(mtip_ctx* ctx, int64_t* out);
/* diagnostic: enqueue a one-workgroup kernel that spins for `microseconds` on the context's stream (asynchronous).  Used to
 * check that the streams of several engines of one process really execute side by side (HIP maps streams onto a limited
 * pool of hardware queues, GPU_MAX_HW_QUEUES; two streams on one queue serialise). */
int mtip_debug_spin(mtip_ctx* ctx, double microseconds);
/* diagnostic: build and verify the resident-column pairing schedule of the polar-factor kernel for every column
 * count 2..k_max <= 127 (every pair exactly once per sweep, no column twice in a round); MTIP_OK or MTIP_EINVAL */
int mtip_debug_check_jacobi_schedule(mtip_ctx* ctx, int k_max);

#ifdef __cplusplus
}
#endif
#endif /* MTIP_HIP_H */
