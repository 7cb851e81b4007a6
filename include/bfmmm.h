/*
 * bfmmm.h -- C ABI of the MI355X-native Gibbs sampler for the functional / multivariate
 * mixed-membership models of ndmarco/BayesFMMM.
 *
 * This is the drop-in boundary for the sampler's hot path.  The reference exposes that path to R
 * through Rcpp-generated `.Call` entry points
 *     _BayesFMMM_BFMMM_Nu_Z_multiple_try   src/RcppExports.cpp:358   (R/RcppExports.R:1604)
 *     _BayesFMMM_BFMMM_Theta_est           src/RcppExports.cpp:396   (R/RcppExports.R:1791)
 *     _BayesFMMM_BFMMM_warm_start          src/RcppExports.cpp:438   (R/RcppExports.R:2018)
 *     _BayesFMMM_BMVMMM_Nu_Z_multiple_try  src/RcppExports.cpp:680
 *     _BayesFMMM_BMVMMM_Theta_est          src/RcppExports.cpp:713
 *     _BayesFMMM_BMVMMM_warm_start         src/RcppExports.cpp:750
 * whose C++ bodies (src/UserFunctions.cpp:166, 684, 1341, 4579, 4995, 5540) build B-splines, run the
 * chain drivers of inst/include/BayesFMMM/BFMMM.h and return named lists of Armadillo arrays.
 * A `.Call` shim (shim/bfmmm_rcall.cpp) marshals SEXPs onto the plain-C entry
 * points below: ragged R lists become CSR arrays (values + offsets), matrices stay column-major,
 * results are copied into caller-allocated buffers laid out exactly like the reference's return
 * values.  No C++ types, no torch types, no exceptions cross this boundary.
 *
 * All functions return 0 on success and a non-zero code on failure; bfmmm_last_error() then gives
 * the message (the argument-validation messages are the reference's own, UserFunctions.cpp:198-286).
 * The library needs a HIP device: there is no CPU fallback.
 */
#ifndef BFMMM_H
#define BFMMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bfmmm_handle bfmmm_handle;

enum { BFMMM_MODEL_FUNCTIONAL = 0, BFMMM_MODEL_MULTIVARIATE = 1 };

/* Update mask bits: every reference driver applies its updates in this relative order
 * (BFMMM.h:1073-1107 Nu_Z, :1253-1292 Theta, :1502-1553 warm start). */
enum {
  BFMMM_U_Z = 1 << 0, BFMMM_U_PI = 1 << 1, BFMMM_U_ALPHA3 = 1 << 2, BFMMM_U_PHI = 1 << 3,
  BFMMM_U_DELTA = 1 << 4, BFMMM_U_A = 1 << 5, BFMMM_U_GAMMA = 1 << 6, BFMMM_U_NU = 1 << 7,
  BFMMM_U_TAU = 1 << 8, BFMMM_U_SIGMA = 1 << 9, BFMMM_U_CHI = 1 << 10,
  BFMMM_U_ETA = 1 << 11, BFMMM_U_TAU_ETA = 1 << 12, BFMMM_U_XI = 1 << 13, BFMMM_U_DELTA_XI = 1 << 14,
  BFMMM_U_A_XI = 1 << 15, BFMMM_U_GAMMA_XI = 1 << 16, BFMMM_U_LOGLIK = 1 << 17
};
/* sweeps of the three stages */
#define BFMMM_SWEEP_NU_Z  (BFMMM_U_Z | BFMMM_U_PI | BFMMM_U_ALPHA3 | BFMMM_U_NU | BFMMM_U_TAU | BFMMM_U_SIGMA | BFMMM_U_LOGLIK)
#define BFMMM_SWEEP_THETA (BFMMM_U_PHI | BFMMM_U_DELTA | BFMMM_U_A | BFMMM_U_GAMMA | BFMMM_U_TAU | BFMMM_U_SIGMA | BFMMM_U_CHI | BFMMM_U_LOGLIK)
#define BFMMM_SWEEP_WARM  (BFMMM_SWEEP_NU_Z | BFMMM_SWEEP_THETA)
/* covariate-adjusted drivers (BFMMM.h:3741-3780, 3944-4010, 4248-4312 / 4809-4894): the eta / Xi blocks run after chi */
#define BFMMM_COV_MEAN (BFMMM_U_ETA | BFMMM_U_TAU_ETA)
#define BFMMM_COV_XI   (BFMMM_U_XI | BFMMM_U_DELTA_XI | BFMMM_U_A_XI | BFMMM_U_GAMMA_XI)

/* Hyper-parameters and sizes; field names follow the reference's argument names
 * (UserFunctions.cpp:166-193, 684-715, 1341-1378).  bfmmm_config_defaults() fills in the
 * reference defaults of the functional entry points. */
typedef struct {
  int32_t model;             /* BFMMM_MODEL_* */
  int32_t n_funct;           /* number of curves (rows of Y for the multivariate model) */
  int32_t K;                 /* clusters */
  int32_t n_eigen;           /* M */
  int32_t basis_degree;      /* functional model only */
  int32_t n_internal_knots;  /* functional model only; P = n_internal_knots + basis_degree + 1 */
  int32_t P;                 /* multivariate model: dimension of the observations */
  int32_t tot_mcmc_iters;    /* chain slots to allocate (r_stored_iters == tot_mcmc_iters) */
  double c[8];               /* Dirichlet hyper-parameter of pi (length K) */
  double b, nu_1;
  double alpha1l, alpha2l, beta1l, beta2l;
  double a_Z_PM, a_pi_PM, var_alpha3, var_epsilon1, var_epsilon2;
  double alpha_nu, beta_nu, alpha_eta, beta_eta, alpha_0, beta_0;
} bfmmm_config;

void bfmmm_config_defaults(bfmmm_config* cfg);

/* Creates a sampler for one data set and uploads it to the GPU `device`.
 *   functional:   y, t are the concatenated observations / time points of all curves,
 *                 offsets[n_funct+1] delimits curve i as [offsets[i], offsets[i+1]) -- the CSR form
 *                 of the R lists `Y` and `time` (arma::field<arma::vec>, UserFunctions.cpp:169-170);
 *                 internal_knots[n_internal_knots], boundary_knots[2] as in UserFunctions.cpp:174-175.
 *   multivariate: y is the n_funct x P column-major matrix `Y` (UserFunctions.cpp:4582);
 *                 t, offsets, knots are ignored (may be NULL).
 * The B-spline basis S(t_i) and the per-curve statistics S_i S_i', S_i y_i, y_i'y_i are computed on
 * the device (replacing BFMMM.h:1017-1025).  The caller's arrays are not retained. */
int bfmmm_create(const bfmmm_config* cfg, int device, const double* y, const double* t, const int64_t* offsets,
                 const double* internal_knots, const double* boundary_knots, bfmmm_handle** out);

/* The functional model over a basis supplied by the caller instead of univariate B-splines: B holds one row of P basis
 * values per observation (row-major, curve i's rows at offsets[i] .. offsets[i+1]), `band` is the half-bandwidth of
 * B_i'B_i (|p - q| > band => zero), Pmat (P x P, column-major) the penalty of the nu prior and pen_band its
 * half-bandwidth.  This is how the high-dimensional functional model enters (BHDFMMM_*: tensor-product basis and
 * penalty of inst/include/BayesFMMM/BSplines.h:18-120, bfmmm_tensor_bspline / bfmmm_tensor_penalty in bfmmm_entry.h);
 * the drivers of that model (BFMMM.h:2892, :3041, :3210) run the same updates.  band <= 31, P <= 64. */
int bfmmm_create_from_basis(const bfmmm_config* cfg, int device, const double* y, const double* B, const int64_t* offsets,
                            int P, int band, const double* Pmat, int pen_band, bfmmm_handle** out);
void bfmmm_destroy(bfmmm_handle* h);

/* Chain batches.  The multi-try entry points run 1 + n_try independent chains on the same data
 * (src/UserFunctions.cpp:302-325, sequentially in the reference).  bfmmm_create_batch / bfmmm_create_from_basis_batch make
 * ONE sampler that holds n_chains such chains over one copy of the per-curve statistics: bfmmm_run advances all of them
 * in lockstep (the chain index is a grid dimension of every kernel launch), chain q drawing from RNG chain id
 * `chain + q * stride` (bfmmm_set_chain_id_stride, default 1), so that chain q of a batch is bit-identical to a
 * stand-alone sampler run with that chain id.  bfmmm_select_chain picks the chain that bfmmm_set_state, bfmmm_get_state,
 * bfmmm_init_state, bfmmm_get_chain and bfmmm_debug_get address (default 0).  bfmmm_set_covariates applies to every chain.
 * bfmmm_tempered_transition needs a batch of one chain. */
int bfmmm_create_batch(const bfmmm_config* cfg, int device, const double* y, const double* t, const int64_t* offsets,
                       const double* internal_knots, const double* boundary_knots, int n_chains, bfmmm_handle** out);
int bfmmm_create_from_basis_batch(const bfmmm_config* cfg, int device, const double* y, const double* B, const int64_t* offsets,
                                  int P, int band, const double* Pmat, int pen_band, int n_chains, bfmmm_handle** out);
int bfmmm_select_chain(bfmmm_handle* h, int q);
int bfmmm_n_chains(const bfmmm_handle* h);
int bfmmm_selected_chain(const bfmmm_handle* h);      /* the chain bfmmm_select_chain chose last (0 before any call); -1 for a null handle */
int bfmmm_set_chain_id_stride(bfmmm_handle* h, uint32_t stride);

/* Final gather of a multi-GPU multi-try (the reference keeps the best of its 1 + n_try chains, src/UserFunctions.cpp:302-325,
 * :861-885).  handles[g], g < n_handles, live on distinct devices of THIS process, were created with the same configuration
 * and have their best chain selected (bfmmm_select_chain); scores[g] / chain_ids[g] are that chain's score and chain index
 * (NaN score: the device holds no valid chain).  One RCCL communicator over the devices: ncclAllGather of the
 * (score, chain index) pairs, then the winner's chain (state and every chain slot) is sent over xGMI (ncclSend / ncclRecv)
 * into the selected chain of handles[0].  *winner = index of the winning handle (largest score, lowest chain index on
 * ties).  This is the only inter-GPU exchange of the library: nothing is communicated inside a chain. */
int bfmmm_gather_best(bfmmm_handle* const* handles, int n_handles, const double* scores, const int32_t* chain_ids, int* winner);

/* Covariate adjustment (the `X` argument of the reference's entry points, UserFunctions.cpp:176): X is the
 * n_funct x D column-major covariate matrix; covariance_adj != 0 enables the Xi block (BFMMM.h:4602 vs :4067).
 * Call once, right after bfmmm_create.  Adds the state / chain names "eta" (P x D x K), "xi" and "gamma_xi"
 * (K arrays P x D x M), "tau_eta" (K x D), "delta_xi" (K x M x D), "A_xi" (K x 2 x D). */
int bfmmm_set_covariates(bfmmm_handle* h, const double* X, int D, int covariance_adj);

/* Basis matrices "B" returned by the reference's entry points (UserFunctions.cpp:327): the rows of
 * all curves concatenated, each row P doubles (row-major: out[(offsets[i]+l)*P + p] = B_i(l,p)). */
int bfmmm_get_basis(bfmmm_handle* h, double* out, int64_t capacity);

/* Current state (the chain's working slot).  Names and layouts are the reference's
 * (column-major Armadillo objects):
 *   "nu" K x P, "Phi" K x P x M, "chi" n x M, "Z" n x K, "pi" K, "alpha_3" 1, "delta" K x M,
 *   "A" K x 2, "gamma" K x P x M, "tau" K, "sigma_sq" 1 (a variance, as everywhere in the reference). */
int bfmmm_set_state(bfmmm_handle* h, const char* name, const double* values, int64_t count);
int bfmmm_get_state(bfmmm_handle* h, const char* name, double* out, int64_t capacity);

/* Initial states of the chain drivers, drawn from the keyed RNG:
 *   stage 0: BFMMM_Nu_Z   (BFMMM.h:1039-1071)  nu ~ N(0,1), chi = 0, Phi = 0, pi ~ Dir(c), Z_i ~ Dir(100 pi), rest 1
 *   stage 1: BFMMM_Theta  (BFMMM.h:1210-1235)  as stage 0 but chi ~ N(0,1), Phi ~ N(0,1)
 * (the caller then pins Z / nu with bfmmm_set_state as BFMMM.h:1244-1250 does). */
int bfmmm_init_state(bfmmm_handle* h, int stage, uint64_t seed, uint32_t chain);

/* Runs n_iters Gibbs iterations with the updates selected by `mask`, starting at chain iteration
 * `first_iter` (which is also the chain slot written, and the RNG counter word).  `phi_chi_zero`
 * != 0 declares Phi = 0 and chi = 0 (stage 1 of the pipeline, BFMMM.h:1040,1063) so that their
 * directions are skipped.  beta = tempering temperature of the *Tempered kernels (1 = untempered). */
int bfmmm_run(bfmmm_handle* h, uint32_t mask, int first_iter, int n_iters, uint64_t seed, uint32_t chain,
              int phi_chi_zero, double beta);

/* Set-up half of bfmmm_run: captures and instantiates the HIP graphs a run with the same arguments replays (a caller that
 * times bfmmm_run, or needs its first call to return quickly, pays the capture here).  Every graph this call instantiates is
 * also launched repeatedly for about 10 ms ("dry launch") between a snapshot and a restore of the chains' work state: the
 * first launch of a graph costs the device 13 - 20 us more than later ones, and the clocks of a device that idled through the
 * capture take milliseconds to come up.  The state a later bfmmm_run starts from is bit-identical with and without the call
 * (tests/test_gpu_prepare.py); the chain SLOTS of that run, first_iter .. first_iter + n_iters - 1, hold scratch values until
 * the run rewrites them. */
int bfmmm_prepare_run(bfmmm_handle* h, uint32_t mask, int first_iter, int n_iters, uint64_t seed, uint32_t chain,
                      int phi_chi_zero);

/* Chain iteration i is written to slot i - base (default 0).  The reference keeps r_stored_iters draws in memory and
 * reuses the slots for every on-disk batch (`i % r_stored_iters`, BFMMM.h:1500-1746): a driver that saves batches
 * moves the base to the first iteration of the next batch; the RNG counter word stays the iteration index, so a
 * batched run draws exactly what an unbatched one does. */
int bfmmm_set_slot_base(bfmmm_handle* h, int base);

/* Tempered-transition block of BFMMM_MTT_warm_start (inst/include/BayesFMMM/BFMMM.h:1556-1657, ladder :1452-1460,
 * acceptance CalculateTTAcceptance.h:22-97) for chain iteration `iter`, to be called right after bfmmm_run has
 * produced that iteration: 2 N_t tempered sweeps of the updates in `mask` (temperatures up and down the geometric
 * ladder ending at beta_N_t), then the Metropolis test.  Chain slot `iter` and the working state end up holding the
 * accepted or the original draw; *logA / *accepted report the test.  Functional model without covariates only. */
int bfmmm_tempered_transition(bfmmm_handle* h, uint32_t mask, int iter, int N_t, double beta_N_t, uint64_t seed,
                              uint32_t chain, double* logA, int* accepted);

/* Copies chain draws to the host: slots [0, n_slots) of `name`, laid out as the reference returns
 * them: "nu" K x P x T, "chi" n x M x T, "Z" n x K x T, "pi" K x T, "alpha_3" T, "A" K x 2 x T,
 * "delta" K x M x T, "sigma_sq" T, "tau" T x K, "gamma"/"Phi" T arrays of K x P x M, "loglik" T. */
int bfmmm_get_chain(bfmmm_handle* h, const char* name, int n_slots, double* out, int64_t capacity);

/* Convergence diagnostics of chain slots [first_slot, first_slot + n_slots) of `name` (the names of bfmmm_get_chain) over
 * EVERY chain of the batch (bfmmm_select_chain is ignored), on the device: split R-hat, bulk / tail ESS, ESS and MCSE of the
 * mean, mean and sd.  One entry per element of one draw, in bfmmm_get_chain's per-draw order ("tau": K
 * entries); capacity >= that count.  The slots are gathered on the sampler's stream into a workspace of at most
 * max_workspace_bytes (0: 256 MiB), in several chunks where a block does not fit.  At most 2^22 draws per row
 * (n_chains x n_slots).  Only the statistics are copied to the host. */
int bfmmm_chain_diagnostics(bfmmm_handle* h, const char* name, int first_slot, int n_slots, int64_t max_workspace_bytes,
                            double* rhat, double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean,
                            double* mean, double* sd, int64_t capacity);

/* The marginal log-density of every curve under the draws of chain slots [first_slot, first_slot + n_slots) of EVERY chain
 * of the batch, scores integrated out: y_i ~ N(B_i c, sigma^2 I + U U'), c = sum_k Z_ik (nu_k + eta_k x_i),
 * U = B_i [V_1 .. V_M], V_m = sum_k Z_ik (phi_km + xi_km x_i).  It does not depend on the components' labels or on the signs
 * of the eigenfunctions, and is computed on the device from the resident per-curve statistics and the chain slots alone.
 *   bfmmm_chain_curve_loglik       copies the matrix to the host: out[i C S + q S + (t - first_slot)] (curve i, chain q, S =
 *                                  n_slots; draw fastest, then chain, then curve), capacity >= n C S.
 *   bfmmm_chain_curve_diagnostics  the seven statistics of bfmmm_chain_diagnostics of each curve's log-density, n entries each.
 *   bfmmm_chain_loo                PSIS-LOO and WAIC over curves with the chains pooled (a curve's row is its C S draws,
 *                                  chain-major; relative efficiency 1), n entries each.
 * The last two keep the matrix on the device and work in chunks of consecutive curves under max_workspace_bytes (0: 256 MiB);
 * at most 2^22 draws per row (n_chains x n_slots).  capacity >= n. */
int bfmmm_chain_curve_loglik(bfmmm_handle* h, int first_slot, int n_slots, double* out, int64_t capacity);
int bfmmm_chain_curve_diagnostics(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes,
                                  double* rhat, double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean,
                                  double* mean, double* sd, int64_t capacity);
int bfmmm_chain_loo(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes, double* lppd, double* elpd_loo,
                    double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic, int64_t capacity);

/* Pooled per-curve fitted functions of chain slots [first_slot, first_slot + n_slots) of EVERY chain of the batch, on the rows
 * E_g of an evaluation basis E (G x P, row-major, in the sampler's basis), and their credible bands:
 *   which = 0   mean_i(g) = E_g . c_i,                        c_i  = sum_k Z_ik (nu_k + sum_d x_id eta_kd)
 *   which = 1   fit_i(g)  = E_g . (c_i + sum_m chi_im V_im),  V_im = sum_k Z_ik (phi_km + sum_d x_id xi_kmd)  (xi: covariance-adjusted)
 * Neither depends on the components' labels or on the signs of the eigenfunctions, so the chains pool as they are.
 * curves: NULL for all n curves, or n_curves indices in [0, n) in any order; result row r is curve curves[r] (m rows).
 *   bfmmm_chain_curve_fit    copies the values to the host: out[((r G + g) C + q) S + s] (chain q, s = t - first_slot, S =
 *                            n_slots), capacity >= m G C S.  For a handful of curves.
 *   bfmmm_chain_curve_bands  mean[r G + g], sd[r G + g] (N - 1; NaN for one draw) and quantiles[(r G + g) nq + q] of each row's
 *                            C S values at probs[0 .. nq) in [0, 1], nq <= 16, by arma::quantile's rule (Hyndman and Fan
 *                            definition 5); capacity >= m G rows.  The values stay on the device; chunks of consecutive result
 *                            rows keep everything the call allocates within max_workspace_bytes (0: 256 MiB).
 *   bfmmm_chain_curve_bands_sim  the simultaneous band of each result row, the reference's rule (FMeanCI's `simultaneous`) with the
 *                            chains pooled.  With mean(g), sd(g) as above over the N = C S draws,
 *                              C(cs) = max over g with sd(g) != 0 of |(v(g, cs) - mean(g)) / sd(g)|, from 0.0,
 *                              crit  = the (1 - alpha) quantile of the N values C(.) by the same rule,
 *                              lower(g) = mean(g) - crit sd(g),  upper(g) = mean(g) + crit sd(g):
 *                            the band holds whole curves of the posterior, not each grid point's values separately.  A grid point
 *                            whose sd is exactly 0 is left out of the maximum and its band is its mean; crit is 0 where every sd
 *                            is 0; for one draw sd, crit, lower and upper are NaN.  mean, sd, lower, upper [r G + g], crit [r];
 *                            capacity >= m G rows; crit, lower and upper are required, mean and sd may be NULL; alpha inside
 *                            (0, 1); G <= 4096 (mean and sd of a curve's grid points stay in LDS, 16 G bytes, beside the 64 KiB
 *                            row that sorts C).  No value is stored: one workgroup per curve forms them three times.  Chunks of
 *                            consecutive result rows keep the call within max_workspace_bytes (0: 256 MiB): shared the table, E
 *                            and the curve list, per curve 8 (4 G + 1) bytes and, for rows above 8192 draws, the row of C and
 *                            its sort workspace.  mean and sd are bfmmm_chain_curve_bands' bit for bit; the result does not
 *                            depend on the chunk or on repeated calls.
 * At most 2^22 draws per row (n_chains x n_slots).  All run on the sampler's stream and leave its state and slots untouched.
 * bfmmm_set_curve_fit_route(1) sends rows of up to 8192 draws through the workspace route of the longer ones as well
 * (a measurement switch; 0, the default: they are formed, sorted and reduced in LDS). */
int bfmmm_chain_curve_fit(bfmmm_handle* h, int which, const double* E, int G, const int32_t* curves, int n_curves, int first_slot,
                          int n_slots, double* out, int64_t capacity);
int bfmmm_chain_curve_bands(bfmmm_handle* h, int which, const double* E, int G, const int32_t* curves, int n_curves, int first_slot,
                            int n_slots, const double* probs, int nq, int64_t max_workspace_bytes, double* mean, double* sd,
                            double* quantiles, int64_t capacity);
int bfmmm_chain_curve_bands_sim(bfmmm_handle* h, int which, const double* E, int G, const int32_t* curves, int n_curves,
                                int first_slot, int n_slots, double alpha, int64_t max_workspace_bytes,
                                double* mean, double* sd, double* crit, double* lower, double* upper, int64_t capacity);
void bfmmm_set_curve_fit_route(int route);

/* Pooled co-membership of curves under chain slots [first_slot, first_slot + n_slots) of EVERY chain of the batch:
 *   d_ij(q, t) = sum_k Z_ik(q, t) Z_jk(q, t)      (0 <= d <= 1; d_ii = sum_k Z_ik^2)
 * the posterior similarity of two curves under a draw.  A sum over k: it does not depend on the components' labels, so the chains
 * pool as they are.  curves: NULL for all n curves, or n_curves >= 0 indices in [0, n) in any order, repeats allowed; result row r
 * is curve curves[r] (m rows), column j curve j (all n).  With N = C n_slots draws:
 *   mean[r n + j]               the mean of d over the N draws; capacity >= m n entries.
 *   sd[r n + j]                 the sample sd (N - 1; NaN for one draw), by a second pass over the draws.  NULL: not computed.
 *   chain_mean[(r C + q) n + j] the mean over the slots of chain q alone.  NULL: not computed.
 * Every sum has a fixed order (slots in order within a chain, then chains in order), so the result does not depend on the chunk
 * or on repeated calls, and the full matrix is symmetric bit for bit.  Chunks of consecutive result rows keep everything the call
 * allocates (the chunk's rows of the three results and its curve indices) within max_workspace_bytes (0: 256 MiB); a budget
 * below one row is refused with the bytes needed.  At most 2^22 draws (n_chains x n_slots).  Runs on the sampler's stream and
 * leaves its state and slots untouched.
 * bfmmm_set_similarity_block: the kernel's workgroups own blocks of 64 x 64 entries where that makes enough of them and of
 * 16 x 64 otherwise (0, the default); 1 / 2 make later calls use the first / second always (a measurement and test switch:
 * the results are the same bits).  Process-wide. */
int bfmmm_chain_similarity(bfmmm_handle* h, const int32_t* curves, int n_curves, int first_slot, int n_slots,
                           int64_t max_workspace_bytes, double* mean, double* sd, double* chain_mean, int64_t capacity);
void bfmmm_set_similarity_block(int block);

/* The least-squares draw of the clustering (Dahl 2006): of the N = C n_slots draws of chain slots [first_slot,
 * first_slot + n_slots) of EVERY chain of the batch, the one whose own co-membership matrix is closest to the pooled mean,
 *   loss(q, t) = sum_i sum_j (d_ij(q, t) - m_ij)^2      over all n^2 ordered pairs, the diagonal included,
 * with d as above and m the mean bfmmm_chain_similarity returns for the full matrix, bit for bit (it is formed again on the
 * device and never stored).  A sum over k inside a sum over pairs: label-invariant, so the minimiser is a real draw in one
 * consistent labelling whose nu, Phi and chi can be read next to its Z (bfmmm_get_slot), and loss(q, .) is a scalar trace of the
 * whole clustering whose split R-hat says whether the chains agree on it.
 *   loss[q n_slots + (t - first_slot)]   capacity >= C n_slots entries.
 *   best_chain, best_slot (may be NULL)  the draw of smallest loss, the slot as an absolute slot index; ties go to the lowest
 *                                        chain, then the lowest slot.
 *   stats (NULL, or 7 doubles)           rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd of the loss trace over the chains,
 *                                        as bfmmm_chain_diagnostics computes them, from the copy on the device.
 * Only the 64 x 64 blocks on and above the diagonal of the matrix are visited; a block's sum counts twice above the diagonal
 * (d_ij and d_ji are the same bits).  Every sum has a fixed order that depends on the position in the block and on the block's
 * number alone, so the result does not depend on the chunk or on repeated calls.  Chunks of consecutive blocks keep everything the
 * call allocates within max_workspace_bytes (0: 256 MiB): 8 N bytes per block, and shared by all blocks the 8 N bytes of the loss
 * vector and, with stats, 56 bytes and the workspace of its row; a budget below one block is refused with the bytes needed.  At
 * most 2^22 draws (n_chains x n_slots).  Runs on the sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_similarity_loss(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes, double* loss,
                                int64_t capacity, int32_t* best_chain, int32_t* best_slot, double* stats);

/* One slot of `name` (a bfmmm_get_chain name) of the selected chain: what bfmmm_get_chain returns for that slot, without the
 * others ("tau": its K entries); capacity >= the entries of one draw. */
int bfmmm_get_slot(bfmmm_handle* h, const char* name, int slot, double* out, int64_t capacity);

/* The mirror of bfmmm_get_chain: writes n_slots draws of `name` into chain slots [first_slot, first_slot + n_slots) of the selected
 * chain (bfmmm_select_chain), so that draws that were made elsewhere -- an earlier run, the reference's on-disk batches, a chain on
 * another device -- can be read by every chain-slot call.
 *   values   n_slots draws in exactly the layout bfmmm_get_chain returns for n_slots slots: draw after draw, each as the reference
 *            lays it out ("tau": n_slots x K column-major, slot fastest)
 *   count    the entries of values: (entries of one draw) x n_slots, anything else is refused
 * Every bfmmm_get_chain name is accepted, "loglik" included and, once bfmmm_set_covariates was called, the covariate blocks.
 * Refused with a message: a null argument, an unknown name, a slot range outside [0, T), a wrong count, a value that is not finite
 * (the message names its slot and entry) and a "sigma_sq" that is not positive.  There is no simplex check on "Z": rescaled
 * memberships may leave it.  The call synchronises the sampler's stream before and after the copy and touches nothing else: the
 * working state, the iteration counter, the slot base, the RNG keys and the other slots stay as they are, and a later bfmmm_run
 * overwrites slots as it always did. */
int bfmmm_set_chain(bfmmm_handle* h, const char* name, int first_slot, int n_slots, const double* values, int64_t count);

/* The log-likelihood given the scores of chain slots [first_slot, first_slot + n_slots) of EVERY chain of the batch, from the
 * resident per-curve records and the slots alone; nothing is uploaded.  With x_i the covariates (xi only where the
 * sampler is covariance-adjusted)
 *   theta_i = sum_k Z_ik (nu_k + eta_k x_i) + sum_m chi_im sum_k Z_ik (phi_km + xi_km x_i)
 *   rss_i   = yy_i - 2 theta_i's_i + theta_i'G_i theta_i
 *   l_i     = -n_i (0.5 log 2 pi + log sqrt(sigma^2)) - rss_i / (2 sigma^2)              (functional)
 *   l_i     = -((P / 2) log(2 pi sigma^2)) - rss_i / (2 sigma^2), P / 2 an integer division (multivariate, as the reference has it)
 * and loglik(q, t) = sum_i l_i, formed as the sweep forms what it stores in "loglik": from sum_i rss_i, added in curve order.
 *   loglik[q n_slots + (t - first_slot)]                       capacity >= C n_slots entries (C chains)
 *   curve (may be NULL)  l_i at [i C n_slots + q n_slots + (t - first_slot)], the layout of bfmmm_chain_curve_loglik;
 *                        capacity >= n C n_slots entries where it is given
 *   store != 0           the totals are also written into the "loglik" slots of the range of every chain, and nowhere else
 * For a loaded chain (bfmmm_set_chain) it supplies the one array the reference's files do not carry; for a chain the sampler ran
 * it is an independent check of the stored "loglik".  Chunks of consecutive curves keep what the call allocates within
 * max_workspace_bytes (0: 256 MiB): 8 C n_slots bytes per curve and as much shared by all curves; a budget below one curve is
 * refused with the bytes needed.  fp64, every sum in a fixed order, no atomics: the bits do not depend on the budget or on repeated
 * calls.  Runs on the sampler's stream; without store it leaves state and slots untouched.  bfmmm_get_timing: "slot_loglik", the
 * device time and launches (one per chunk) of k_slot_rss, and "slot_loglik_reduce", those of the kernel that adds a chunk's rows. */
int bfmmm_chain_slot_loglik(bfmmm_handle* h, int first_slot, int n_slots, int store, int64_t max_workspace_bytes, double* loglik,
                            double* curve, int64_t capacity);

/* Pooled per-curve covariance surfaces under chain slots [first_slot, first_slot + n_slots) of EVERY chain of the batch, on the
 * rows of two evaluation bases E1 (G1 x P) and E2 (G2 x P), row-major in the sampler's basis.  With the scores
 * chi_im ~ N(0, 1), the covariance function of curve i under a draw is
 *   C_i(g, h) = sum_m (E1_g . V_im)(E2_h . V_im),   V_im = sum_k Z_ik (phi_km + sum_d x_id xi_kmd)   (xi: covariance-adjusted)
 *             = sum_k sum_k' Z_ik Z_ik' C^(k,k')(g, h)
 * a sum over k and k' of products of two factors that change sign together: it depends neither on the components' labels nor on
 * the signs of the eigenfunctions, so the chains pool as they are.  The second moment that goes with which = 0 of
 * bfmmm_chain_curve_bands.  E2 NULL: E2 = E1 and G2 = G1 (the argument G2 is ignored).  curves: NULL for all n curves, or
 * n_curves >= 0 indices in [0, n) in any order, repeats allowed; result row r is curve curves[r] (m rows).  With N = C n_slots draws:
 *   mean[(r G1 + g) G2 + h]                the mean of C_i(g, h) over the N draws; capacity >= m G1 G2 entries.
 *   sd[(r G1 + g) G2 + h]                  the sample sd (N - 1; NaN for one draw), by a second pass over the draws.  NULL: not computed.
 *   chain_mean[((r C + q) G1 + g) G2 + h]  the mean over the slots of chain q alone.  NULL: not computed.
 * diagonal != 0 (E2 must be NULL): only the entries g = h, the curve's variance function, at mean[r G1 + g], sd[r G1 + g] and
 * chain_mean[(r C + q) G1 + g], capacity >= m G1; they are the diagonal of the surface bit for bit.
 * Every sum has a fixed order (slots in order within a chain, then chains in order), so the result does not depend on the chunk
 * or on repeated calls, a selected row is the full result's row, and with E2 NULL the surface is symmetric, all bit for bit.
 * Chunks of consecutive result rows keep everything the call allocates (the projection tables, E1, E2, the curve list and the
 * chunk's rows of the three results) within max_workspace_bytes (0: 256 MiB); a budget below what is shared plus one curve is
 * refused with the bytes needed.  At most 2^22 draws (n_chains x n_slots).  Runs on the sampler's stream and leaves its state and
 * slots untouched. */
int bfmmm_chain_curve_cov(bfmmm_handle* h, const double* E1, int G1, const double* E2, int G2, int diagonal, const int32_t* curves,
                          int n_curves, int first_slot, int n_slots, int64_t max_workspace_bytes, double* mean, double* sd,
                          double* chain_mean, int64_t capacity);

/* Label alignment of the draws against a pivot (the pivot method, Marin, Mengersen & Robert 2005).  Independent
 * chains, and a chain that switches, label the components differently; against one reference membership matrix Zref (host, n x K
 * column-major: a real draw such as the least-squares one above, or any matrix of that shape, finite) every draw (q, t) of chain
 * slots [first_slot, first_slot + n_slots) of EVERY chain of the batch gets
 *   A[c][l] = sum_i Z_ic(q, t) Zref_il,     perm(q, t) = the maximiser over all K! permutations p of sum_l A[p(l)][l],
 * so that column l of the aligned draw is column perm[l] of the draw; that trace is largest where |Z P - Zref|_F is smallest.  The
 * maximum is exact over the device's own A (a recursion over the 2^K subsets, not greedy); among equal sums the
 * lexicographically smallest permutation.  Labels only: signs and rotations of the eigenfunctions are not identified and not touched.
 *   perm[(q n_slots + s) K + l]   capacity >= C n_slots K entries.
 *   score[q n_slots + s]          that sum, A[p0][0] + (A[p1][1] + (..)).  NULL: not returned.
 * The sum over i has a fixed order, so repeated calls give the same bits.  At most 2^22 draws (n_chains x n_slots).  Runs on the
 * sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_align(bfmmm_handle* h, const double* Zref, int first_slot, int n_slots, int32_t* perm, double* score, int64_t capacity);

/* bfmmm_chain_diagnostics of `name` with the components of every draw relabelled by its row of perm (from bfmmm_chain_align, or
 * any rows that are permutations of 0 .. K - 1): where element e of a draw has component index k, the value is read from
 * component perm[k] of the same draw.  Arrays without a component axis (chi, sigma_sq, alpha_3, loglik) are summarised as they
 * are.  The seven arrays are those of bfmmm_chain_diagnostics, capacity >= the entries of one draw; with the identity
 * permutation they are its results bit for bit.  quant[q + nq e]: the nq <= 16 quantiles probs (inside [0, 1]) of element e over
 * the pooled C n_slots draws by arma::quantile's rule, as bfmmm_post_col_quantiles computes them; nq = 0: probs and quant may be
 * NULL.  Chunks of consecutive elements keep the gathered rows, their workspaces and results within max_workspace_bytes (0: 256
 * MiB; rows of more than 8192 draws sort in a workspace from the same budget); the call also holds the 4 C n_slots K bytes of perm
 * on the device.  A budget below one row is refused with the bytes needed.  At most 2^22 draws.  The results do not depend on the
 * chunk.  Runs on the sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_aligned_summary(bfmmm_handle* h, const char* name, const int32_t* perm, int first_slot, int n_slots, const double* probs,
                                int nq, int64_t max_workspace_bytes, double* rhat, double* ess_bulk, double* ess_tail, double* ess_mean,
                                double* mcse_mean, double* mean, double* sd, double* quant, int64_t capacity);

/* The cluster mean functions on the rows of E (G x P, row-major in the sampler's basis) with the labels aligned and the chains
 * pooled: of v_kg(q, s) = sum_p E_gp nu_{perm[k], p}(q, s) (p in order from 0) over the C n_slots draws,
 *   mean[k + K g], sd[k + K g] (N - 1)   and   quant[q + nq (k + K g)]   (arma::quantile's rule; nq = 0: probs, quant may be NULL);
 * capacity >= K G rows.  The coefficient table of the reference's FMeanCI, without its rescale / trans_mats.  With covariates
 * set this is the mean function at x = 0 (eta is not added).  Chunks of consecutive rows keep the values, the sort workspace of
 * rows of more than 8192 draws and the results within max_workspace_bytes (0: 256 MiB); E and perm are held beside them.  At
 * most 2^22 draws.  Runs on the sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_cluster_mean_bands(bfmmm_handle* h, const int32_t* perm, const double* E, int G, int first_slot, int n_slots,
                                   const double* probs, int nq, int64_t max_workspace_bytes, double* mean, double* sd, double* quant,
                                   int64_t capacity);

/* The cluster covariance surfaces with the labels aligned and the chains pooled, with pointwise and simultaneous credible bands
 * (the reference's FCovCI, without its rescale / trans_mats).  For draw cs = q n_slots + s of chain slots
 * [first_slot, first_slot + n_slots) of EVERY chain of the batch, its row perm[cs K + .] (from bfmmm_chain_align, or any rows that
 * are permutations of 0 .. K - 1), rows E1_g, E2_h of two evaluation bases (G1 x P and G2 x P, row-major in the sampler's basis;
 * E2 NULL: E2 = E1 and G2 = G1, the argument G2 is ignored) and pair r = (k_r, l_r) of aligned components
 *   theta_km   = phi_{perm[k], m} + sum_d x_d xi_{perm[k], m, d}       (x: D entries, one covariate setting; NULL: phi alone)
 *   W1_k[g][m] = sum_p E1_gp theta_km,p,   W2 likewise with E2
 *   c_r(g, h)  = sum_m W1_k[g][m] W2_l[h][m],
 * which does not change when the eigenfunctions change sign or are rotated jointly over the components: once the labels are
 * aligned the chains pool as they are.  pairs: n_pairs >= 0 pairs pairs[2 r], pairs[2 r + 1], 0-based, in any order, repeats
 * allowed (m = n_pairs; 0: returns at once and writes nothing), or NULL for all m = K (K + 1) / 2 pairs with k <= l in the order
 * (0, 0), (0, 1), .., (0, K - 1), (1, 1), ...  With e = (r G1 + g) G2 + h and N = C n_slots draws:
 *   mean[e], sd[e] (N - 1; NaN for one draw)   required;
 *   quant[q + nq e]                            the nq <= 16 quantiles probs (inside [0, 1]) by arma::quantile's rule, as
 *                                              bfmmm_post_col_quantiles computes them; nq = 0: probs and quant may be NULL;
 *   trace[e N + cs]                            the values themselves (the reference's cov_trace).  NULL: not copied;
 *   crit[r], lower[e], upper[e]                all NULL or all set: the simultaneous (1 - alpha) band of pair r by DESIGN.md 7h's
 *                                              rule, crit the (1 - alpha) quantile over the draws of the largest |(c - mean) / sd|
 *                                              over the pair's entries with sd != 0 (from 0.0; a NaN is kept), lower / upper =
 *                                              mean -/+ crit sd.  alpha inside (0, 1), checked only where the band is asked for.
 * diagonal != 0 (E2 must be NULL): only the entries g = h, the variance function for k = l, at e = r G1 + g; they are the diagonal
 * of the surface bit for bit.  capacity >= m G1 G2 entries (diagonal: m G1); trace holds capacity N doubles.
 * x requires a covariance-adjusted sampler and must be finite.
 * A value's bits depend on (draw, pair, g, h) alone, so the results do not depend on the chunk or on repeated calls, a selected
 * pair equals its rows of the full result, and with E2 NULL pair (l, k) is the transpose of pair (k, l), all bit for bit.
 * Chunks of consecutive result rows keep the values, the sort workspace of rows of more than 8192 draws and the chunk's results
 * within max_workspace_bytes (0: 256 MiB); the projection tables, E1, E2, x, perm, the pairs and the band's per-draw maxima are
 * shared by all rows and count against it; a budget below what is shared plus one row is refused with the bytes needed.  With
 * the band and more than one chunk a second sweep over the chunks forms the values again.  At most 2^22 draws.  Runs on the
 * sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_cluster_cov_bands(bfmmm_handle* h, const int32_t* perm, const double* E1, int G1, const double* E2, int G2,
                                  int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot, int n_slots,
                                  const double* probs, int nq, double alpha, int64_t max_workspace_bytes,
                                  double* mean, double* sd, double* quant, double* crit, double* lower, double* upper,
                                  double* trace, int64_t capacity);

/* The reference's `rescale` step per draw (its ZCI, FMeanCI, FCovCI, MVMeanCI and MVCovCI rescale by default): a
 * mixed-membership model is identified only up to an invertible K x K map of the simplex, and the reference reports Z A^-1, A nu,
 * A Phi_m, A eta and A xi, with A the map under which the purest curve of every component is a vertex.  For draw cs = q n_slots + s
 * of chain slots [first_slot, first_slot + n_slots) of EVERY chain of the batch:
 *   rule mode (transform NULL): for the aligned component k, curve[cs K + k] = the smallest i that attains max_i Z[i, perm[k]]
 *     (arma::index_max: the first maximum; a NaN is never the maximum) and A[k][c] = Z[curve, c] over the raw components c, copied.
 *     perm: the draw's row of bfmmm_chain_align (NULL: the identity).  The reference refuses the rule for K > 2, where Z A^-1 may
 *     leave the simplex; here it is allowed for every K <= 8 and z_min reports by how much.
 *   given mode: A = transform[(cs K + k) K + c] (N K K doubles; the reference's trans_mats, already in the aligned labelling);
 *     perm is not read and curve is -1.
 *   mix[(cs K + k) K + c] = A,  mix_inv[(cs K + c) K + k] = A^-1      capacity >= N K K entries each, N = C n_slots
 *   rcond[cs] = 1 / (|A|_1 |A^-1|_1),  z_min[cs] = min_{i,k} sum_c Z[i, c] A^-1[c][k]      N entries each; curve: N K
 *   *n_singular (may be NULL): the singular draws -- a pivot exactly zero, A not finite or, under the rule, two components that
 *     share their pure curve.
 *     Such a draw gets A^-1 = NaN, rcond = 0 and z_min = NaN; it is counted, never dropped and never an error, and the pooled rows
 *     of the calls below then carry the NaN.  A NaN among the rescaled memberships of a draw that is not singular is kept in z_min.
 * A^-1 by Gauss-Jordan elimination with partial pivoting in one fixed order without fused multiply-adds, so repeated calls give the
 * same bits.  At most 2^22 draws.  Runs on the sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_rescale(bfmmm_handle* h, const int32_t* perm, const double* transform, int first_slot, int n_slots, double* mix,
                        double* mix_inv, int32_t* curve, double* rcond, double* z_min, int64_t* n_singular, int64_t capacity);

/* bfmmm_chain_aligned_summary under the transform of every draw (mix, mix_inv of bfmmm_chain_rescale for the same slots) in place of
 * its permutation: for nu, Phi, eta and xi the element with aligned component k is sum_c A[k][c] (the element of component c), for
 * Z it is sum_c Z[i, c] A^-1[c][k], c = 0 .. K - 1 in order without fused multiply-adds; with permutation matrices these are
 * bfmmm_chain_aligned_summary's results bit for bit.  Any other name is refused: the reference defines no rescale for it.  The
 * other arguments, the budget rule and the limits are those of bfmmm_chain_aligned_summary; the call holds 8 C n_slots K K bytes of
 * the transform on the device. */
int bfmmm_chain_rescaled_summary(bfmmm_handle* h, const char* name, const double* mix, const double* mix_inv, int first_slot, int n_slots,
                                 const double* probs, int nq, int64_t max_workspace_bytes, double* rhat, double* ess_bulk,
                                 double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd, double* quant,
                                 int64_t capacity);

/* bfmmm_chain_cluster_mean_bands under the transform of every draw, the reference's FMeanCI with rescale / trans_mats:
 *   v_kg(q, s) = sum_p E_gp sum_c A[k][c] (nu_c,p + sum_d x_d eta_c,p,d)      (p, c and d in order from 0)
 * x: one covariate setting of D finite entries, which the reference's FMeanCI with X rescales too; it requires covariates to be
 * set.  NULL: nu alone.  The other arguments are those of bfmmm_chain_cluster_mean_bands. */
int bfmmm_chain_cluster_mean_bands_rescaled(bfmmm_handle* h, const double* mix, const double* E, int G, const double* x, int first_slot,
                                            int n_slots, const double* probs, int nq, int64_t max_workspace_bytes, double* mean,
                                            double* sd, double* quant, int64_t capacity);

/* bfmmm_chain_cluster_cov_bands under the transform of every draw, the reference's FCovCI with rescale / trans_mats: the tables
 * are filled for the raw components and a second pass forms W~_k = sum_c A[k][c] W_c (c in order from 0); the values, the bands,
 * the chunks and every other argument are those of bfmmm_chain_cluster_cov_bands, and with permutation matrices so are the bits. */
int bfmmm_chain_cluster_cov_bands_rescaled(bfmmm_handle* h, const double* mix, const double* E1, int G1, const double* E2, int G2,
                                           int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot,
                                           int n_slots, const double* probs, int nq, double alpha, int64_t max_workspace_bytes,
                                           double* mean, double* sd, double* quant, double* crit, double* lower, double* upper,
                                           double* trace, int64_t capacity);

/* Contrasts of cluster mean functions and covariate effects with pointwise and simultaneous bands, the chains pooled:
 * where clusters k and l differ, what covariate d does to cluster k's mean function, f_k(x) - f_k(x'), differences of differences.
 * For draw cs = q n_slots + s of chain slots [first_slot, first_slot + n_slots) of EVERY chain of the batch, its K x K label map
 * A = mix[(cs K + k) K + c] (N K K doubles: the transform of bfmmm_chain_rescale, or the permutation matrix of the draw's row of
 * bfmmm_chain_align, A[k][c] = 1 where c = perm[k]), rows E_g of an evaluation basis (G x P, row-major in the sampler's basis; the
 * identity for the multivariate model) and contrast r < R with weights w_nu[r K + k] and w_eta[(r K + k) D + d] (NULL: nu alone;
 * it requires covariates to be set, at most 8)
 *   a_c    = sum_k w_nu[r, k] A[k][c],   a'_cd = sum_k w_eta[r, k, d] A[k][c]                  (k in order from 0)
 *   b_r[p] = sum_c ( a_c nu_c,p + sum_d a'_cd eta_c,p,d )                                      (c, then d, in order from 0)
 *   v_r(g) = sum_p E_gp b_r[p]                                                                 (p in order from 0)
 * without fused multiply-adds.  With e = r G + g and N = C n_slots draws:
 *   mean[e], sd[e] (N - 1)                     required;
 *   quant[q + nq e]                            the nq <= 16 quantiles probs by arma::quantile's rule; nq = 0: probs, quant and
 *                                              norm_quant may be NULL;
 *   n_positive[e]                              required: the draws with v_r(g) > 0, strictly;
 *   crit[r], lower[e], upper[e], n_exceed[r]   all NULL or all set: the simultaneous (1 - alpha) band of contrast r by the rule of
 *                                              bfmmm_chain_cluster_cov_bands over the G grid points (dev_r(cs) = max_g |v - mean| / sd,
 *                                              sd = 0 skipped, a NaN kept), and n_exceed[r] = #{cs : dev_r(cs) >= t_r} with t_r the
 *                                              largest |mean| / sd over the grid points with sd > 0 (0 where there is none):
 *                                              n_exceed / N is the smallest level at which the band excludes the zero function somewhere.
 *                                              alpha inside (0, 1), checked only where the band is asked for;
 *   norm_stats[s R + r]                        required: the seven statistics of bfmmm_chain_diagnostics (s = rhat, ess_bulk,
 *                                              ess_tail, ess_mean, mcse_mean, mean, sd) of norm_r(cs) = sqrt(sum_g weights[g] v_r(g)^2),
 *                                              g in order from 0, each term weights[g] (v v); weights: G finite entries >= 0 (NULL:
 *                                              1 / G each);  norm_quant[q + nq r]: its pooled quantiles;
 *   trace[e N + cs], norm_trace[r N + cs]      the values and the norms themselves.  NULL: not copied.
 * capacity >= R G rows; trace holds capacity N doubles.  R in 1 .. 64; a contrast whose weights are all zero and a weight that is
 * not finite are refused.  A value's bits depend on (draw, contrast, g) alone and a norm is summed in the order of g across the
 * chunks, so the results do not depend on the chunk, on repeated calls or on the other contrasts of the call.  With permutation
 * matrices and w_nu = e_k the values are those of bfmmm_chain_cluster_mean_bands bit for bit (but for the sign of a zero).
 * Chunks of consecutive result rows keep the values, the sort workspace of rows of more than 8192 draws and the chunk's results
 * within max_workspace_bytes (0: 256 MiB); the coefficient table (8 R P N bytes), E, mix, the weights, the norm rows with their
 * statistics and the band's per-draw maxima are shared by all rows and count against it; a budget below what is shared plus one
 * row is refused with the bytes needed.  With the band and more than one chunk a second sweep over the chunks forms the values
 * again.  At most 2^22 draws.  Runs on the sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_cluster_contrast_bands(bfmmm_handle* h, const double* mix, const double* E, int G, const double* w_nu,
                                       const double* w_eta, int R, const double* weights, int first_slot, int n_slots,
                                       const double* probs, int nq, double alpha, int64_t max_workspace_bytes, double* mean,
                                       double* sd, double* quant, int32_t* n_positive, double* crit, double* lower, double* upper,
                                       int32_t* n_exceed, double* norm_stats, double* norm_quant, double* trace, double* norm_trace,
                                       int64_t capacity);

/* The eigenvalues and eigenfunctions of the cluster covariance operators with the labels aligned and the chains pooled (DESIGN.md
 * 7l): the principal components of the surfaces of bfmmm_chain_cluster_cov_bands.  For draw cs = q n_slots + s of chain slots
 * [first_slot, first_slot + n_slots) of EVERY chain of the batch, its row perm[cs K + .], a grid basis E (G x P, row-major in the
 * sampler's basis; the identity for the multivariate model), quadrature weights w (G entries, finite and >= 0; NULL: all 1) and
 * aligned component k
 *   theta_km = phi_{perm[k], m} + sum_d x_d xi_{perm[k], m, d}       (x: D entries, one covariate setting; NULL: phi alone)
 *   Q        = E' diag(w) E                                          (P x P, once per call, g in order from 0)
 *   S_k      = Theta_k' Q Theta_k = V diag(lambda) V'                (M x M, Theta_k = [theta_k1 .. theta_kM]; cyclic Jacobi)
 *              lambda_1 >= .. >= lambda_M >= 0                       (ties in index order; negative rounding noise clamped to 0)
 *   total_k  = trace S_k = sum_g w_g C^(k,k)(g, g)                   (summed from the diagonal before the rotations)
 *   pve_kj   = lambda_kj / total_k                                   (0 where total_k == 0)
 *   b_kj     = Theta_k v_j / sqrt(lambda_kj)                         (0 where lambda_kj <= M 2^-53 lambda_k1)
 *   psi_kj(g)= sgn_kj E_g . b_kj,   sgn_kj = +1 if b_kj . (E' diag(w) ref_kj) >= 0 else -1,   j < n_functions,
 * the eigenpairs of the w-discretised covariance operator of cluster k: ordinary PCA of Phi_k Phi_k' with E = I and w = 1.  They do
 * not change when the eigenfunctions of the sampler change sign or are rotated jointly over m, so once the labels are aligned the
 * chains pool.  ref (K x n_functions x G, row (k J + j) G + g, finite) fixes the signs; NULL: the sign makes the entry of largest
 * |sqrt(w_g) psi(g)| positive, lowest g first on ties.  Only the upper triangle of S_k is read.  The Jacobi iteration takes its
 * pairs in a round-robin order fixed by M alone, skips a pair with |s_pq| <= u max(sqrt(|s_pp s_qq|), u ||S_k||_F of the start),
 * u = 2^-53, and stops after a sweep without a rotation; a problem still rotating in its 40th sweep makes the call fail naming the
 * chain, the slot and the component.  With N = C n_slots draws, J = n_functions in 0 .. M and nq <= 16 quantiles probs by
 * arma::quantile's rule (nq = 0: probs and every *_quant may be NULL):
 *   val_diag[i K M + k M + j]                    i = 0 .. 6: split R-hat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd of
 *                                                lambda_kj as bfmmm_chain_diagnostics computes them;  val_quant[q + nq (k M + j)];
 *   pve_mean, pve_sd [k M + j], pve_quant[q + nq (k M + j)];   tot_mean, tot_sd [k], tot_quant[q + nq k]   (sd: N - 1);
 *   fn_mean, fn_sd [e], fn_quant[q + nq e]       of psi at row e = (k J + j) G + g; capacity >= K J G rows; J = 0: may be NULL,
 *                                                and no row, no ref and no values launch is made (E and w are still held for Q);
 *   val_trace[(k M + j) N + cs], fn_trace[e N + cs]   the values themselves.  NULL: not copied;
 *   *max_sweeps                                  the largest number of sweeps a problem took, the last, rotation-free one included.
 * x requires a covariance-adjusted sampler and must be finite.  A value's bits depend on (draw, component) alone (a function's: and
 * on j, g), so the results do not depend on the chunk or on repeated calls, lambda, pve and total do not depend on n_functions,
 * ref or trace, and J < M gives the first J functions of J = M, all bit for bit.
 * Chunks of consecutive eigenfunction rows keep the values, the sort workspace of rows of more than 8192 draws and the chunk's
 * results within max_workspace_bytes (0: 256 MiB); Q, E, w, x, perm, ref and its projection, and the per-draw outputs of the solve
 * (lambda, pve, total, the signed b of K J P doubles a draw, the status words) with the results of the lambda, pve and total rows
 * are shared by all rows and count against it; a budget below what is shared plus one row is refused with the bytes needed.  At
 * most 2^22 draws.  Runs on the sampler's stream and leaves its state and slots untouched. */
int bfmmm_chain_cluster_eigen(bfmmm_handle* h, const int32_t* perm, const double* E, int G, const double* w, const double* x,
                              int n_functions, const double* ref, int first_slot, int n_slots, const double* probs, int nq,
                              int64_t max_workspace_bytes, double* val_diag, double* val_quant, double* pve_mean, double* pve_sd,
                              double* pve_quant, double* tot_mean, double* tot_sd, double* tot_quant, double* fn_mean, double* fn_sd,
                              double* fn_quant, double* val_trace, double* fn_trace, int32_t* max_sweeps, int64_t capacity);

/* k_ceig_solve forms S_k either by plain multiplies and additions or by v_mfma_f64_16x16x4_f64 on zero-padded tiles;
 * the launcher takes the form that measured faster.  1 makes later calls of bfmmm_chain_cluster_eigen take the plain form, 2 the MFMA
 * form, 0 (and anything else) the launcher's choice again -- the tests and tests/perf/bench_cluster_eig.py run both.  The two
 * forms round differently; each keeps every promise of the call.  Process-wide; default 0. */
void bfmmm_set_cluster_eig_form(int form);

/* Prediction of held-out curves from the chain slots: for every new curve r, with the chains pooled, the log
 * predictive density log p(y_r | data) and the predictive law of its memberships Z_new ~ Dir(alpha_3 pi), integrated over by
 * staged importance sampling on the device.  For draw cs = q n_slots + s of chain slots [first_slot, first_slot + n_slots) of
 * EVERY chain of the batch the integrand is the marginal density l(z) of bfmmm_chain_curve_loglik, evaluated from the new
 * curve's record and the A x A table Gamma_ab = theta_a' G theta_b, tau_a = theta_a' s of the draw's A = K (M + 1) directions
 * (x folded in), which the kernel forms once per (curve, draw) and keeps on chip.
 * Input forms.  A spline handle takes y, t, offsets (n_new + 1 entries; curve r is [offsets[r], offsets[r + 1])) with B NULL and
 * uses the handle's knots and degree; a handle of bfmmm_create_from_basis takes y, B (rows of P, row-major), offsets with t NULL
 * and the handle's band; the multivariate model takes y as n_new x P column-major with t, B, offsets NULL.  X: n_new x D
 * column-major, required exactly when the sampler has covariates, finite.  No curve may be empty.
 * The estimator, per (r, cs), runs n_stages = R rounds of n_samples = J samples; the results are the last round's.
 *   stage 0 proposes from the prior, a = alpha_3 pi of the draw; stage st draws z_j ~ Dir(a) from gamma variates keyed by
 *   (seed, the RNG chain id of chain q, the slot) with index ((r R + st) J + j) K + k, r the curve's position in the call, every
 *   variate clamped below at the smallest normal double;
 *   lw_j = l(z_j) + sum_k (alpha_3 pi_k - a_k) log z_jk + lB(a) - lB(alpha_3 pi)      (stage 0: lw_j = l(z_j));
 *   w_j = exp(lw_j - max lw), lpd = max + log(sum w / J), ess = (sum w)^2 / sum w^2, m_k = sum w z_k / sum w,
 *   q_k = sum w z_k^2 / sum w, v_k = sum w (z_k - m_k)^2 / sum w (a second pass);
 *   next proposal: r_k = m_k (1 - m_k) / v_k - 1 over v_k > 0, a0 their median (the mean of the middle two of an even count;
 *   1e4 where no v_k > 0) clipped to [1, 1e4], a_k = max(a0 m_k, 0.5).
 * ess is a result: rows with a low ess are not to be trusted.  Pooled over the N = C n_slots draws:
 *   lpd[r] = log mean_cs exp(lpd_trace[r, cs]);  z_mean[r K + l] = mean_cs m_perm[l];  z_sd[r K + l] = sqrt(mean_cs q - z_mean^2),
 *   the sd of the whole predictive law;  ess_mean[r], ess_min[r];   capacity >= n_new rows, all five required.
 * perm (N K entries as from bfmmm_chain_align; NULL: the identity) relabels the membership columns of every draw; lpd and ess do
 * not depend on it.  Optional traces (NULL: not copied): lpd_trace, ess_trace [r N + cs]; z_trace[(r N + cs) K + l], the last
 * stage's m relabelled; prop_trace[((r N + cs) R + st) K + k], the proposal of every stage; samples[(((r N + cs) R + st) J + j) K + k],
 * the z of every stage (tests and small shapes).
 * zs: NULL, or a host table [(cs J + j) K + k] that every curve takes as its stage-0 samples; no variate is drawn, n_stages must be
 * 1 and lw = l (the deterministic hook).
 * Refused by name: a null handle or required pointer, n_new < 0 (0 returns at once), an empty curve, n_samples < 1, n_stages < 1,
 * a slot range outside the storage, more than 2^22 draws, n_new R J K above 2^32 (the RNG index), a perm row that is no
 * permutation, a shape whose on-chip tables (Gamma, the samples of a stage) exceed 160 KiB of LDS.  A value's bits depend on
 * (curve, chain, slot, seed, J, R) alone.  Chunks of consecutive new curves keep the traces within max_workspace_bytes (0: 256
 * MiB); the new curves' data and records, X, perm and zs are shared by all curves and count against it; a budget below what is
 * shared plus one curve is refused with the bytes needed.  Runs on the sampler's stream and leaves its state, its slots and its
 * resident records untouched. */
int bfmmm_chain_predict(bfmmm_handle* h, const double* y, const double* t, const double* B, const int64_t* offsets,
                        int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                        int n_stages, uint64_t seed, const double* zs, int64_t max_workspace_bytes,
                        double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min,
                        double* lpd_trace, double* z_trace, double* ess_trace, double* prop_trace, double* samples,
                        int64_t capacity);

/* Marginal PSIS-LOO over the training curves with the memberships integrated out.  bfmmm_chain_loo runs PSIS on
 * log p(y_i | Z_i, draw); this call runs it on log p(y_i | draw) = log of the integral of exp l_i(z) Dir(z; alpha_3 pi) dz, which
 * bfmmm_chain_predict estimates per (curve, draw), here from the resident records of the n training curves (nothing is copied or
 * recomputed): the first pass is bfmmm_chain_predict's with n_samples = J, n_stages = R and r = the curve's index in the data,
 * so its traces are that call's on the same data, seed, J and R, bit for bit.
 * Refinement (refine != 0).  A pair (curve, draw) is selected where its ess < ess_floor or its lpd is not finite.  Each selected
 * pair runs once more: refine_stages = R2 rounds of refine_samples = J2 samples by the rule of bfmmm_chain_predict, except that
 * stage 0 proposes from the last proposal a of the pair's first pass in place of the prior, so that
 *   lw_j = l(z_j) + sum_k (alpha_3 pi_k - a_k) log z_jk + lB(a) - lB(alpha_3 pi)   in stage 0 as well (zero where a is the prior);
 * variates keyed by (seed, the RNG chain id of the chain, the slot) under an update id of its own, index ((i R2 + st) J2 + j) K + k
 * with i the curve's index.  The pair's lpd and ess are overwritten; there is one such run, not a loop until the floor is met.
 * Then PSIS-LOO and WAIC as bfmmm_chain_loo on the n x N matrix of lpd, N = C n_slots (the chains pooled).
 * Outputs (capacity >= n rows): the six pointwise arrays of bfmmm_chain_loo; ess_mean, ess_min [i] over the curve's N pairs
 * after refinement; n_refined [i], the pairs of the curve that were refined; n_below [i], the pairs the selection rule still
 * picks afterwards (reported, not dropped).  Optional (NULL: not copied): lpd_trace, ess_trace [i N + cs] after refinement,
 * ess_trace_first [i N + cs] before it; and for the *n_ref refined pairs in increasing (curve, chain, slot) order, e their
 * position: refined_index [3 e + .] = (curve, chain, slot relative to first_slot), refine_prop [(e R2 + st) K + k] the proposal
 * of every refinement stage, refine_samples_out [((e R2 + st) J2 + j) K + k] its samples (tests and small shapes); these three
 * hold ref_capacity pairs, and a call that refines more is refused.  n_ref may be NULL where none of the three is given.
 * Refused by name: a null handle or required pointer, a slot range outside the storage, more than 2^22 draws, n_samples,
 * n_stages, refine_samples or refine_stages below 1, ess_floor negative or not finite, n R J K or n R2 J2 K above 2^32 (the RNG
 * index), what bfmmm_chain_predict's kernel cannot take, J2 samples whose on-chip tables exceed 160 KiB of LDS (with the bytes),
 * a negative max_workspace_bytes or one below what one curve needs.  A value's bits depend on (curve, chain, slot, seed, J, R,
 * J2, R2, ess_floor) alone.  Chunks of consecutive curves keep the traces, the list and the optional outputs within
 * max_workspace_bytes (0: 256 MiB).  All chains of the batch, on one device; leaves the sampler's state and slots untouched. */
int bfmmm_chain_loo_marginal(bfmmm_handle* h, int first_slot, int n_slots, int n_samples, int n_stages, uint64_t seed, int refine,
                             double ess_floor, int refine_samples, int refine_stages, int64_t max_workspace_bytes,
                             double* lppd, double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic,
                             double* ess_mean, double* ess_min, int32_t* n_refined, int32_t* n_below,
                             double* lpd_trace, double* ess_trace, double* ess_trace_first,
                             int32_t* refined_index, double* refine_prop, double* refine_samples_out, int64_t* n_ref,
                             int64_t capacity, int64_t ref_capacity);

/* The Laplace mixture proposal for the same integral.  bfmmm_chain_predict_laplace is bfmmm_chain_predict without
 * n_stages and zs: per (curve r, chain q, slot t) log p(y_r | draw) = log int exp g(eta) d eta over the log-ratios eta (d = K - 1,
 * z_k = e^eta_k / (1 + sum e^eta), z_K = 1 / (1 + sum e^eta)) of g(eta) = l(z) + sum_k alpha_k log z_k - lB(alpha), alpha = alpha_3 pi,
 * by one round of n_samples = J importance samples from a mixture of Student-t components with 4 degrees of freedom.  Component 0 is
 * always there: centre the log-ratios of alpha / alpha_0, scale [alpha_0 (diag p - p p')]^-1, J_0 = max(1, J / 16) samples.  The
 * others are the modes a damped Newton ascent finds from K + 1 starts (alpha / alpha_0, and for each k 0.9 at k with 0.1 / (K - 1)
 * elsewhere; a start counts where -H is positive definite and grad'(-H)^-1 grad < 1e-6 within 40 steps; a mode within 1e-3 of an
 * earlier one is dropped): centre eta_c, scale (-H_c)^-1 = L_c L_c', J_c = floor((J - J_0) w_c) with w_c ~ exp(g_c) prod diag L_c and
 * the remainder to the heaviest.  Samples are contiguous by component: eta_j = eta_c + L_c eps_j sqrt(4 / chi2_j), chi2 = -2 log(U1
 * U2), keyed by (seed, the RNG chain id, the slot) under an update id of its own, index (r J + j)(d + 2) + i.  lw_j = g(eta_j) - log
 * sum_c (J_c / J) t4(eta_j; eta_c, L_c); lpd, ess, z_mean and z_sd as bfmmm_chain_predict forms them.  Where no start converges only
 * component 0 is left (J_0 = J): a valid estimate with a low ess, which ess_min shows.
 * Outputs of bfmmm_chain_predict (without prop_trace and samples) and, optional (NULL: not copied): n_modes [r N + cs], the modes
 * kept; components [((r N + cs)(K + 2) + c) CD + .], CD = d + d (d + 1) / 2 + 2: centre, L packed by rows, g_c and J_c of slot c
 * (unused slots are zero); eta_samples [((r N + cs) J + j) d + i].
 * Refused by name: what bfmmm_chain_predict refuses, n_new J (K + 1) above 2^32 (the RNG index) and tables, search scratch and
 * samples above 160 KiB of LDS (with the bytes).  A value's bits depend on (curve, chain, slot, seed, J) alone.
 * bfmmm_chain_loo_marginal_laplace is bfmmm_chain_loo_marginal with that kernel on the resident records as its only pass: no
 * stages and no refinement; ess_mean, ess_min and n_below (pairs with ess < ess_floor or a lpd that is not finite) by the same
 * counting kernel, then the same PSIS pass.  Its lpd_trace is bfmmm_chain_predict_laplace's on the same data, seed and J. */
int bfmmm_chain_predict_laplace(bfmmm_handle* h, const double* y, const double* t, const double* B, const int64_t* offsets,
                                int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                                uint64_t seed, int64_t max_workspace_bytes,
                                double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min,
                                double* lpd_trace, double* z_trace, double* ess_trace,
                                int32_t* n_modes, double* components, double* eta_samples, int64_t capacity);
int bfmmm_chain_loo_marginal_laplace(bfmmm_handle* h, int first_slot, int n_slots, int n_samples, uint64_t seed, double ess_floor,
                                     int64_t max_workspace_bytes,
                                     double* lppd, double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic,
                                     double* p_waic, double* ess_mean, double* ess_min, int32_t* n_below,
                                     double* lpd_trace, double* ess_trace, int32_t* n_modes, double* components,
                                     double* eta_samples, int64_t capacity);

/* Observation-level PSIS-LOO and LOO-PIT from the chain slots: every single observation y_ij of the selected curves
 * (curves null: all n; otherwise n_curves indices, repeats allowed) is left out in turn, the rest of its curve kept and the scores
 * chi_i integrated out.  Under draw t the law of y_ij given y_i,-j is N(m_ij(t), v_ij(t)) by a leverage formula on the M x M system of
 * bfmmm_chain_curve_loglik; PSIS (relative efficiency 1, the chains pooled: n_chains x n_slots draws a row) on
 * l_ij(t) = log p(y_ij | y_i,-j, draw t) gives the six arrays of bfmmm_chain_loo per observation, and from the same smoothed weights
 * pit = E_loo[Phi(z_ij)] (uniform under a calibrated model), mean = E_loo[m_ij] and sd = sqrt(E_loo[m_ij^2 + v_ij] - mean^2), the LOO
 * predictive mean and sd of the observation.  All nine arrays hold one entry per observation, in the order of the selected curves and
 * then of the observations of a curve (the multivariate model: the P coordinates); `capacity` entries each, at least the number of
 * such observations.  The traces (null: not wanted) hold n_chains x n_slots values an observation, draw fastest, then chain:
 * l_ij(t), Phi(z_ij(t)), m_ij(t) and v_ij(t).  The work is done in chunks of row tiles (up to 64 consecutive observations of a curve)
 * whose four device matrices, with the dense basis rows, fit max_workspace_bytes (0: 256 MiB); the results do not depend on it, bit
 * for bit.  One device; at most 2^22 draws a row. */
int bfmmm_chain_loo_pointwise(bfmmm_handle* h, const int32_t* curves, int n_curves, int first_slot, int n_slots,
                              int64_t max_workspace_bytes, double* lppd, double* elpd_loo, double* p_loo, double* pareto_k,
                              double* elpd_waic, double* p_waic, double* pit, double* mean, double* sd, double* loglik_trace,
                              double* pit_trace, double* mean_trace, double* var_trace, int64_t capacity);

/* PSIS-LOO and WAIC separately for every chain of the batch: the six arrays of bfmmm_chain_loo with PSIS run on the
 * n_slots draws of each chain by itself, relative efficiency 1.  unit 0: the rows are the curves, as bfmmm_chain_loo's (all n;
 * `curves` must be null); unit 1: the observations of the selected curves, as bfmmm_chain_loo_pointwise's, in its order, without
 * its pit, mean, sd and traces.  A row of those calls holds its n_chains x n_slots draws chain-major, so the same device matrix is
 * n_chains rows of n_slots draws per unit and goes through the same PSIS pass: entry r n_chains + c of every array is what
 * bfmmm_post_psis gives for chain c's draws of row r, bit for bit.  `capacity` entries each, at least rows x n_chains.  The chunks
 * and max_workspace_bytes are those of the pooled call; the results do not depend on them.  The timers are the pooled calls':
 * "curve_ll_ms" (unit 0), "loo_pointwise" and "loo_pointwise_psis" (unit 1).  Refused by name: a null pointer, a unit other than
 * 0 or 1, `curves` with unit 0, the curve list, the slot range, the capacity, the budget sign, more than 2^22 draws a chain. */
int bfmmm_chain_loo_by_chain(bfmmm_handle* h, int unit, const int32_t* curves, int n_curves, int first_slot, int n_slots,
                             int64_t max_workspace_bytes, double* lppd, double* elpd_loo, double* p_loo, double* pareto_k,
                             double* elpd_waic, double* p_waic, int64_t capacity);

/* Leave-block-out PSIS cross-validation within curves from the chain slots: every listed block of observations of a
 * training curve is left out in turn, the rest of its curve kept, Z_i at the draw's value and the scores chi_i integrated out.  Block k
 * is the observations block_obs[block_offsets[k] .. block_offsets[k + 1]) of curve block_curve[k], given as indices within the curve
 * (the multivariate model: coordinates), 1 to 64 distinct ones in any order; blocks may overlap and a curve may appear at several
 * places of the list.  Under draw t the joint law of y_b given the rest of the curve is Gaussian in closed form on the M x M system of
 * bfmmm_chain_loo_pointwise, A_-b = A - W_b'W_b; PSIS (relative efficiency 1, the chains pooled) on l_b(t) = log p(y_b | y_i,-b, draw t)
 * gives the six arrays of bfmmm_chain_loo per BLOCK (block_capacity entries each, at least n_blocks), and from the block's smoothed
 * weights, per listed OBSERVATION in the order of block_obs (row_capacity entries each, at least block_offsets[n_blocks]):
 * pit = E[Phi(z_j)], mean = E[m_j] and sd = sqrt(max(0, E[m_j^2 + v_j] - mean^2)), m_j, v_j, z_j the marginals of the joint law.
 * The traces (null: not wanted) hold n_chains x n_slots values, draw fastest, then chain: loglik_trace l_b(t) per block; pit_trace
 * Phi(z_j(t)), mean_trace m_j(t) and var_trace v_j(t) per listed observation.  With one observation a block this is
 * bfmmm_chain_loo_pointwise's law; with the whole curve as the block l_b is bfmmm_chain_curve_loglik's value.
 * The work is done in chunks of row tiles: consecutive blocks of the list that belong to the same curve share a tile while they fit 64
 * rows, a block never straddles tiles; a chunk's four device matrices (one row per listed observation), tables and basis rows fit
 * max_workspace_bytes (0: 256 MiB).  A block's results depend on (block, chain, slot) alone, bit for bit: not on the budget, the
 * other blocks or its place in the list.  PSIS runs on every row of a block (with the same bits), which the block's first row reports.
 * Refused by name before anything is allocated: a null required pointer, n_blocks < 1, offsets that do not start at 0 or do not
 * increase (an empty block), a block above 64, a curve outside 0 .. n - 1, an index outside 0 .. n_i - 1, a repeated index within a
 * block, the two capacities, and the slot range, budget sign and row limit as elsewhere.  One device; at most 2^22 draws a row. */
int bfmmm_chain_loo_blocks(bfmmm_handle* h, const int32_t* block_curve, const int64_t* block_offsets, const int32_t* block_obs,
                           int64_t n_blocks, int first_slot, int n_slots, int64_t max_workspace_bytes,
                           double* lppd, double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic,
                           double* pit, double* mean, double* sd, double* loglik_trace,
                           double* pit_trace, double* mean_trace, double* var_trace, int64_t block_capacity, int64_t row_capacity);

/* The fitted function of held-out, partly observed curves from the chain slots: bfmmm_chain_predict with the same
 * arguments -- the same samples, and lpd, z_mean, z_sd, ess_mean, ess_min and their traces bit for bit -- and, on the G rows of an
 * evaluation basis E (G x P row-major, rows in the sampler's basis as in bfmmm_chain_curve_bands; the identity for the
 * multivariate model), where the new curve runs: its predictive mean function, the sd of its predictive law and quantile bands.
 * Per (curve r, draw cs) and last-stage sample z_j with weight w_j, the curve's scores have the law
 *   chi | y_r, z_j, draw ~ N(A^-1 u, sigma^2 A^-1),  A = sigma^2 I_M + W (u, W of bfmmm_chain_predict's l(z_j)), so with
 *   e_g,(k,mt) = E_g . theta_(k,mt):  c_j(g) = sum_k z_jk e_g,(k0),  v_j(g)_m = sum_k z_jk e_g,(km),
 *   mu_j(g) = c_j(g) + (A^-1 u)' v_j(g),  s_j(g) = sigma^2 v_j(g)' A^-1 v_j(g)  (+ sigma^2 with noise != 0),
 *   mean_trace = mu_t(g) = sum_j w_j mu_j(g) / sum w,  var_trace = v_t(g) = sum_j w_j [s_j(g) + (mu_j(g) - mu_t(g))^2] / sum w.
 * The N = C n_slots draws are pooled with equal weights, as z_mean pools them: the new curve does not reweight the parameter
 * draws.  fit_mean[r G + g] = mean_cs mu_t(g);  fit_sd[r G + g] = sqrt(mean_cs v_t(g) + mean_cs (mu_t(g) - fit_mean)^2), in two passes.
 * Every (curve, draw) also gives one path from the mixture: j* the first j with sum_{i <= j} w_i > U sum w (the sum in sample
 * order; the last j should rounding leave none), xi ~ N(0, I_M),
 *   path_trace(g) = c_j*(g) + (A^-1 u + sigma L^-T xi)' v_j*(g)  (+ sigma eps_g with noise),  A = L L',
 * and fit_q[(r G + g) nq + q] is quantile probs[q] of the N paths at (r, g) by the rule of bfmmm_chain_curve_bands (nq 0 .. 16).
 * Variates: the key of bfmmm_chain_predict (seed, the RNG chain id of chain q, the slot) under an update id of this call, index
 * r (1 + M + G) + i with r the curve's position in the call: i = 0 the uniform U, i = 1 + m the normal xi_m, i = 1 + M + g the
 * normal eps_g.
 * Outputs: the five pooled arrays of bfmmm_chain_predict, fit_mean, fit_sd (required), fit_q (required where nq > 0); optional
 * traces (NULL: not copied): those of bfmmm_chain_predict, mean_trace, var_trace, path_trace [(r G + g) N + cs], path_index (j*)
 * and path_u (U) [r N + cs], path_xi [(r N + cs) M + m].
 * Refused by name: everything bfmmm_chain_predict refuses, a null or non-finite E, G < 1, nq outside 0 .. 16 or a probability
 * outside [0, 1], n_new (1 + M + G) above 2^32, a shape whose on-chip tables (those of bfmmm_chain_predict, e of G rounded up to 16
 * rows, M x 256 values where M > 8) exceed 160 KiB of LDS, with the bytes.  A value's bits depend on (curve, chain, slot, seed, J, R, E, noise)
 * alone, not on the chunk or a repeated call.  The fit's traces of a chunk count against max_workspace_bytes.  Multivariate rows
 * are fully observed; missing coordinates, simultaneous bands and reweighting the draws by p(y_r | draw) are not provided. */
int bfmmm_chain_predict_fit(bfmmm_handle* h, const double* y, const double* t, const double* B, const int64_t* offsets,
                            int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                            int n_stages, uint64_t seed, const double* zs, const double* E, int G, int noise,
                            const double* probs, int nq, int64_t max_workspace_bytes,
                            double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min,
                            double* fit_mean, double* fit_sd, double* fit_q,
                            double* lpd_trace, double* z_trace, double* ess_trace, double* prop_trace, double* samples,
                            double* mean_trace, double* var_trace, double* path_trace, int32_t* path_index, double* path_u,
                            double* path_xi, int64_t capacity);

/* Diagnostics for the parity tests, of the selected chain after the last bfmmm_run: "rec" (n x LREC per-curve statistics),
 * "H" (R x LG pair-weighted Gram blocks, band-packed), "H2" (the same blocks as the factorisation and the sweep read them:
 * R x P x (2 BW + 2), piece-major), "tvec" (A x P), "Cmat" (A x P x P: C_a = Prec_a^-1 as k_factor left it), "Lz" (A x P: L_a z_a of the sampled directions),
 * "rvec" and "hq" (A x P each: r_a = t_a - sum_b H_ab theta_b and H_aa theta_a at the start of the sweep, as k_factor wrote
 * them -- the sweep updates copies of its own), "theta" (K (M + 1) x P), "dims" (as doubles; the last entry is BWP, the band
 * half-width of the conditional precisions), "curve_ll_ms" (device
 * milliseconds of k_chain_curve_ll in the last bfmmm_chain_curve_loglik / bfmmm_chain_curve_diagnostics / bfmmm_chain_loo) and
 * "pg_route": how sub-batch 0 of the last bfmmm_run ran its pair-Gram contraction, {packed (0 / 1), KS, NKS,
 * body (0 general, 1 single-chain, 2 chain loop, 3 chain loop with staged groups; -1 packed), G (chains per group; 0 packed),
 * tail (single-chain body only, a sum of flags: 4 the s-part workgroup runs its single-chain body, 8 the deferred
 * log-likelihood has a workgroup of its own; 0 otherwise)} as doubles, recorded on the host;
 * "sweep_route": which sweep kernel the last bfmmm_run launched, {kernel (0 k_sweep_diag, 1 k_sweep_chain, 2 k_sweep),
 * template argument (directions per lane of k_sweep_diag, band half-width of k_sweep_chain, 0 for k_sweep), mv (the model's flag:
 * k_sweep_diag's second template argument), direct (k_sweep without LDS staging), block threads} as doubles, recorded on the
 * host from the decision the launcher reads (also right for a run that replays cached graphs); "rss" (1): the residual sum of
 * squares in the chain's device state -- the sweep's YY - sum_a theta_a'(t_a + r_a) after a run whose mask has U_SIGMA, unless
 * the run also had a chi pass (U_CHI with n_eigen > 0, or U_LOGLIK without U_SIGMA, or covariates), whose per-curve sums
 * replace it;
 * "curve_route" (14): the per-curve instances of the last bfmmm_run, recorded on the host from the decision the launcher reads:
 *   its last Z update {form (0 none, 1 stand-alone k_curve_z, 2 its lean trailing form, 3 fused into k_curve_chi), BW, LPC, COV,
 *   KT, KEX}, then its last k_curve_chi launch {BW, LPC, COV, SMALL, KX, MX, mode (0 scalar job only, 1 residual sums, 2 chi
 *   update), whether the run's earlier k_curve_chi launches ran the next iteration's Z update};
 * "chi_norm" (n x M): the standard normals of the chi update as the device holds them;
 * "zprep" ((3 K + 5) x n): the Z proposals prepared for the NEXT iteration (field-major: Znew, lo, ln, pr_old, pr_new, lpn, lpo, log_uu);
 * "rss_part" (curve workgroups): k_curve_chi's block sums of the per-curve residual sums of squares;
 * "logz_part" (curve workgroups x K): the block sums of log Z_ik of the last Z update;
 * "stil" (n x P): s_i - G_i o_i (covariates set);
 * "yyp_part" (curve workgroups): block sums of yy_i - 2 o_i's_i + o_i'G_i o_i (covariates set);
 * "cfull" (n x P): the fitted coefficient c_i (covariates set): k_curve_chi's value, which the eta / Xi steps update when the mask has them;
 * "gfull" (n x P): G_i c_i likewise (covariates set);
 * what the eta / Xi block of the last iteration left (covariates set; an error otherwise), A2 = K D (+ K M D with the Xi block)
 * directions in the order of the sweep (eta: d outer, j inner; then Xi: (j, m, d)), groups of D consecutive directions:
 *   "Wdir" (n x A2, direction fastest): w_{a,i} = Z_ij x_id (chi_im);
 *   "H2aa" (NPAIR x LG): sum_i w_u w_v G_i, band rows, of in-group pair (u <= v) of group g at row g D(D+1)/2 + v(v+1)/2 + u
 *     (only groups the mask updates are written);
 *   "C2" (A2 x P x P) and "Lz2" (A2 x P): the conditional covariance C_a and L_a z_a of every updated direction;
 *   "gstd2" (K D + K M D + K D P M): the standard gamma variates of tau_eta, delta_xi, gamma_xi;
 *   "thetaX" (K (M + 1) D x P, row (j (M + 1) + mt) D + d; A2 x P with the Xi block): the committed eta (mt = 0) and xi rows;
 * "cov_route" (11): what the eta / Xi block of every iteration of the last bfmmm_run launches, recorded on the host from the
 *   decision the launcher reads: {BW and LPC of k_cov_group, its exact-D instance (0: general), the D instance of k_cov_w2, PP of
 *   k_cov_factor, NB2 (curve chunks of k_cov_w2), NBS (workgroups of k_cov_group), NPG (in-group pairs), k_cov_group launches
 *   (the closing residual pass included), do_eta, do_xi};
 * "z_record" ((6 + K) x n, field-major): acceptance, log_uu, pr_old, pr_new, lpo, lpn, Znew of the last Z update of the last run
 *   (bfmmm_set_curve_record; fails when that run stored none);
 * "z_prepared" (1): whether that update took the proposals prepared ahead by k_factor (1) or evaluated them in place (0);
 * "gstd" (K P M + K M + 13 K + 8, as allocated): what job_hyper_draws left for the last iteration's scalar job -- the standard gamma
 *   variates of gamma (index (k P + p) M + m), delta (k M + i) and tau (k), the A proposals and uniforms (2 j + i), the sigma^2
 *   variate, four log(tgamma) / log terms per A cell -- and, while bfmmm_set_curve_record is on, the acceptance values of the last
 *   pi and alpha_3 steps in the two doubles behind;
 * "ni" (n): the record builder's per-curve observation counts (an int array on the device, widened to double on the host;
 *   multivariate model: P each);
 * "piprep" (9 KMAX + 16): the pi / alpha_3 tables k_factor prepared for the next iteration (scalar_jobs.hpp: pi_alpha_layout);
 * "pi_prepared" (1): whether the last pi / alpha_3 job took prepared tables (bfmmm_set_curve_record; fails when the last run's mask
 *   had neither U_PI nor U_ALPHA3, or recording was off);
 * "hyper_route" (3): where the scalar jobs of the last bfmmm_run rode, recorded on the host from the decisions the launchers read:
 *   {delta / A / gamma / tau: 0 k_curve_chi, 1 the lean k_curve_z (k_curve_chi in the closing iteration), 2 deferred to the next
 *   k_pair_gram and k_loglik_flush; pi / alpha_3: 0 k_pair_gram, 1 k_pair_gram with the deferred log-likelihood in a workgroup of its
 *   own, 2 k_factor; whether k_factor prepares the next iteration's pi / alpha_3 tables};
 * "tt_trace" (7 N_t + 6): what the last bfmmm_tempered_transition computed on the host, {N_t, ladder[0 .. N_t - 1], the beta of sweep
 *   l = 1 .. 2 N_t, sigma^2 before the block and after every sweep (2 N_t + 1), RSS likewise (2 N_t + 1), log u, logA, accepted}
 *   (fails before the first block);
 * "dyn" (18): the scalars of the chain's device state a hand-over between runs depends on, {iter, slot, tt_step, status, slot_base,
 *   beta, zprep_valid, zprep_iter, zprep_tt, znorm_valid, znorm_iter, znorm_tt, piprep_valid, piprep_iter, sigma^2, alpha_3, rss,
 *   loglik} as doubles.
 * Returns the number of doubles written through *count. */
int bfmmm_debug_get(bfmmm_handle* h, const char* name, double* out, int64_t capacity, int64_t* count);

/* For the tests: sweep l = tt_step of a tempered-transition block on its own -- the call the loop of bfmmm_tempered_transition makes
 * (one iteration of the updates in `mask` and the log-likelihood at temperature beta, RNG counter word tt_step, written to the chain
 * slot of `iter`), through the same helper.  Every "last run" name of bfmmm_debug_get then describes that sweep. */
int bfmmm_debug_run_tt(bfmmm_handle* h, uint32_t mask, int iter, uint64_t seed, uint32_t chain, double beta, uint32_t tt_step);

/* Timing of the last bfmmm_run: milliseconds between HIP events recorded on the sampler's stream
 * around the whole run and, per kernel family, accumulated over iterations when `profile` was
 * enabled with bfmmm_set_profile (which disables graph replay).
 * names: "total", "curve_z", "pair_gram", "factor", "sweep", "curve_chi", "loglik".
 * Of the last bfmmm_chain_curve_fit / bfmmm_chain_curve_bands (always measured): "curve_fit" (the sum of the following),
 * "curve_fit_project", "curve_fit_rows", "curve_fit_values", "curve_fit_reduce" (quantiles and moments of the workspace route).
 * Of the last bfmmm_chain_curve_bands_sim (always measured): "curve_sim", the device time and launches of k_fit_sim (and, for rows
 * above 8192 draws, of the kernel that writes the band ends), and "curve_sim_reduce", those of the long rows' sort.
 * Of the last bfmmm_chain_similarity (always measured): "similarity", the device time and launches of its kernel.
 * Of the last bfmmm_chain_similarity_loss (always measured): "similarity_loss", the device time and launches (one per chunk) of
 * k_similarity_loss, and "similarity_loss_reduce", those of the kernel that adds a chunk's blocks into the loss vector.
 * Of the last bfmmm_chain_curve_cov (always measured): "curve_cov", the device time and launches (one per chunk) of k_curve_cov,
 * and "curve_cov_project", those of the projection that precedes them.
 * Of the last bfmmm_chain_align / bfmmm_chain_aligned_summary / bfmmm_chain_cluster_mean_bands (always measured): "align_gram"
 * (one launch), "align_gather" and "align_project" (one launch per chunk), the device time and launches of their own kernels.
 * Of the last bfmmm_chain_cluster_cov_bands (always measured): "cluster_cov_project", the device time of k_ccov_project and the
 * tables it filled (1, or 2 with E2); "cluster_cov", the device time and launches of k_ccov_values (one per chunk, and one more
 * per chunk where the band takes a second sweep); "cluster_cov_maxdev", those of k_ccov_maxdev (one per chunk; 0 without the band).
 * Of the last bfmmm_chain_cluster_eigen (always measured): "cluster_eig_gram", the device time of k_ceig_gram (one launch);
 * "cluster_eig", that of k_ceig_solve (one launch); "cluster_eig_values", the device time and launches of k_ceig_values (one per
 * chunk; 0 with n_functions = 0).
 * Of the last bfmmm_chain_predict (always measured): "predict_stats", the device time and launches of the kernel that forms the
 * new curves' records (0 launches for a handle of bfmmm_create_from_basis, whose records are formed on the host); "predict", the
 * device time and launches of k_predict and the pooling kernel after it (two per chunk).
 * Of the last bfmmm_chain_predict_fit (always measured): "predict_stats" as above; "predict_fit", the device time and launches of
 * k_predict_fit, the two pooling kernels and, where nq > 0, the quantiles of the paths (three or four per chunk).
 * Of the last bfmmm_chain_loo_marginal (always measured): "loo_marginal", the device time and launches of the first pass, the
 * counting kernel (twice) and, where pairs are refined, the list and refinement kernels (three to five per chunk);
 * "loo_marginal_psis", those of the PSIS pass (one per chunk).
 * Of the last bfmmm_chain_predict_laplace: "predict_stats" as above; "predict_laplace", k_predict_lap and the pooling kernel (two
 * per chunk).  Of the last bfmmm_chain_loo_marginal_laplace: "loo_marginal_laplace", k_predict_lap and the counting kernel (two per
 * chunk); "loo_marginal_psis" as above.
 * Of the last bfmmm_chain_loo_pointwise (always measured): "loo_pointwise", the device time and launches of the dense basis rows (one
 * launch a call, spline handles only), k_loo_pointwise (one per chunk) and, where var_trace is asked for, the variance kernel (one per
 * chunk); "loo_pointwise_psis", those of the PSIS pass with its three expectations (one per chunk).
 * Of the last bfmmm_chain_loo_blocks (always measured): "loo_blocks", the device time and launches of the dense basis rows (one launch
 * a call, spline handles only), k_loo_blocks (one per chunk) and, where var_trace is asked for, the variance kernel (one per chunk);
 * "loo_blocks_psis", those of the PSIS pass with its three expectations (one per chunk).
 * Of the last bfmmm_chain_rescale / bfmmm_chain_rescaled_summary / bfmmm_chain_cluster_mean_bands_rescaled (always measured):
 * "rescale_transform" (one launch), "rescale_gather" and "rescale_project" (one launch per chunk), the device time and launches of
 * their own kernels.  bfmmm_chain_cluster_cov_bands_rescaled: the timers of bfmmm_chain_cluster_cov_bands, "cluster_cov_project"
 * with the mixing pass in it.
 * Of the last bfmmm_chain_cluster_contrast_bands (always measured): "contrast_coef" (k_contrast_coef, one launch a call),
 * "contrast_values" (k_contrast_values, one launch per chunk, and one more per chunk where the band takes a second sweep) and
 * "contrast_norm" (k_contrast_norm, one launch per chunk), next to "rescale_project"; the reductions, the counts and the band's
 * launches are not timed.
 * Of the last bfmmm_chain_slot_loglik (always measured): "slot_loglik" (k_slot_rss) and "slot_loglik_reduce" (k_slot_ll_reduce), the
 * device time and launches of each, one per chunk. */
int bfmmm_set_profile(bfmmm_handle* h, int enable);
int bfmmm_get_timing(bfmmm_handle* h, const char* name, double* ms, int64_t* launches);

/* The per-curve and covariate kernels are also built in exact-shape instances (K, M, D compile-time: DESIGN.md section 5) that
 * the launchers pick when the model's shape is on the list.  0 makes every later launch (of samplers created afterwards) use the
 * general instances instead -- the parity tests run both and compare.  Process-wide; default 1. */
void bfmmm_set_exact_instances(int enable);

/* 1 makes the Z updates of every later run store, per curve, the values their accept / reject decision was made from (the
 * acceptance value itself never leaves the kernel otherwise): bfmmm_debug_get "z_record", which fails while this is off.  With
 * 0 the kernels get a null pointer and skip the stores behind one uniform test.  For the tests.  Process-wide; default 0. */
void bfmmm_set_curve_record(int enable);

/* Single chains run the G workgroups of the pair-Gram contraction through a body of their own where the shape allows (DESIGN.md
 * section 5); 0 makes later runs use the general body instead -- the parity tests run both and compare bit for bit.
 * Process-wide; default 1. */
void bfmmm_set_solo_pair_gram(int enable);

/* On the same route the s-part workgroup of the contraction has a single-chain body too, and the deferred log-likelihood
 * of the previous iteration runs in an extra workgroup of its own instead of in front of pi / alpha_3;
 * 0 makes later runs keep the general s-part body and the shared workgroup -- tests/test_gpu_pair_gram_solo_s.py compares
 * the two bit for bit.  What a run took is the last entry of "pg_route".  Process-wide; default 1. */
void bfmmm_set_solo_pair_gram_tail(int enable);

const char* bfmmm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
