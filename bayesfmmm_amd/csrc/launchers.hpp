// Host interface of the kernel files to the host files (bfmmm_capi.hip, the driver, capi_chain.hip and capi_loo.hip): every launcher,
// geometry and prepare_* function they call.  Included by them and by every file that defines one of them, so that a
// declaration and its definition cannot drift apart.
#pragma once
#include "model.hpp"
#include <string>

// ---- kernels_diag.hip ----
long long diag_row_max();                      // C S of the longest row
size_t diag_row_ws_doubles(int C, int S);      // workspace doubles a row of the global tier needs (0 in the LDS tier)
std::string diag_launch(const double* d_x, long long rows, int C, int S, double* d_out, long long ld_out, double* ws, long long ws_rows,
                        hipStream_t st);
std::string diag_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S, int C, int p0, int P,
                        double* ws, hipStream_t st);

// ---- kernels_loo.hip ----
int post_psis_device(const double* d_ll, long long ld, int n, int S, double* const out[6]);
int post_psis_expect_device(const double* d_ll, long long ld, int n, int S, const double* d_aux, int n_aux, long long aux_stride,
                            double* const out[6], double* expect_host);

// ---- kernels_stacking.hip ----
// Stacking weights of the Q x n log densities at d_L (candidate-major; overwritten) on the current device: the
// results of bfmmm_post_stacking to the host.  init: Q host weights on the simplex, or null.  The geometry: one grid-stride pass of
// k_stack_em covers threads x max_workgroups units.
int post_stacking_device(double* d_L, long long n, int Q, const double* init, int max_iter, int check_every, double tol, double* weights,
                         double* pointwise, double* objective, double* gap, int* n_iter, int* converged);
void post_stacking_geometry(int* threads, int* max_workgroups);

namespace bfmmm {

// ---- kernels_stats.hip ----
int launch_stats_functional(int degree, int n, int P, int LREC, const int64_t* off, const double* t, const double* y,
                            const double* knots, int n_knots, double* rec, int* ni, double* B_dense, int* err,
                            hipStream_t st);
void launch_stats_multivariate(int n, int P, int LREC, const double* Y, double* rec, int* ni, hipStream_t st);
void launch_stats_totals(int n, int LREC, int yy_off, const double* rec, const int* ni, double* out_yy,
                         long long* out_counts, hipStream_t st);

// ---- kernels_curve.hip ----
// Which instance of k_curve_z (which 0) or k_curve_chi (which 1) a launch takes: everything curve_route_decide decides, and all
// launch_curve reads.  arg is launch_curve's third argument: k_curve_z: bit 0 do_update, bit 1 the lean trailing form;
// k_curve_chi: the mode (0 / 1 / 2) | 16 where it also runs the next iteration's Z update.
struct CurveRoute {
  int which = 0;
  int BW = -1;              // band class (template argument); -1: none is built for Dims::BW
  int LPC = 0;              // lanes per curve: 32 or 64
  bool COV = false;
  int KT = 0;               // k_curve_z: the compile-time bound on K (4 / KMAX; the exact K where KEX)
  bool LEAN = false, KEX = false;
  bool SMALL = false;       // k_curve_chi: K <= 4 and M <= 8 (exact instances included)
  int KX = 0, MX = 0;       // k_curve_chi: the exact (K, M) instance, or 0, 0
  int nblk = 0;             // curve workgroups (the grid has 8 more in front of them for k_curve_chi and the lean k_curve_z)
  size_t lds = 0;           // dynamic LDS bytes
};
CurveRoute curve_route_decide(const Dims& d, int which, int arg);
int launch_curve(const Ctx& c, int which, int do_update, hipStream_t st);
int curve_blocks(int n, int P);
void prepare_curve_kernels();

// ---- kernels_pair_gram.hip ----
// How a (sub-)batch runs its pair-Gram contraction: everything pg_route_decide decides, and all the two launchers read.
struct PgRoute {
  bool packed = false;      // k_pair_gram_pack + k_pg_reduce_pack (geometry pk, tiles in pack); otherwise k_pair_gram + k_pg_reduce
  int KS = 0, NKS = 0;      // curves per k-slice and k-slices of either
  int body = -1;            // k_pair_gram: 0 the general body (one chain), 1 the single-chain body of the G workgroups (pg_solo_g),
                            // 2 the chain loop, 3 the chain loop with G chains staged together; packed: -1
  int G = 0;                // chains k_pair_gram stages together (packed: 0)
  int tail = 0;             // what else a body-1 launch runs in bodies of its own: PG_SOLO_S | PG_SOLO_LL (do_pg flag bits)
  int do_pg = 0;            // k_pair_gram's flag word: 0 = only the extra workgroups' scalar jobs run
  size_t lds = 0;           // dynamic LDS bytes of the contraction's launch
  PgPack pk;
  double* pack = nullptr;   // packed partial tiles, pgp_pack_doubles(pk) doubles: owned and filled in by the driver
};
void pg_geometry(const Dims& d, int& NKS, int& KS);
PgRoute pg_route_decide(const Dims& d, int nch_handle, int nch, bool pg, bool defer_loglik, size_t pg_part_doubles, bool may_pack);
bool pg_route_solo_ll(const PgRoute& r);      // the launch gives the deferred log-likelihood a workgroup of its own (job_pi_alpha runs without it)
size_t pgp_pack_doubles(const PgPack& g);
void launch_pair_gram(const Ctx& c, const PgRoute& r, hipStream_t st);
void launch_pg_reduce(const Ctx& c, int NKS, hipStream_t st);
void launch_pair_gram_pack(const Ctx& c, const PgRoute& r, hipStream_t st);
void prepare_pair_gram_kernels();

// ---- kernels_factor.hip ----
void launch_factor(const Ctx& c, hipStream_t st);
void prepare_factor_kernels();

// ---- kernels_sweep.hip ----
// Which sweep kernel a run's Dims (MD set) take: everything sweep_route_decide decides, and all launch_sweep reads.
struct SweepRoute {
  int kernel = -1;          // 0 k_sweep_diag, 1 k_sweep_chain, 2 k_sweep; -1: the problem fits none of them
  int targ = 0;             // k_sweep_diag: RPL (directions per lane); k_sweep_chain: BW; k_sweep: 0
  int direct = 0;           // k_sweep: the column blocks and C_a are read from L2 at every step (no LDS staging)
  int threads = 0;          // workgroup size
  size_t lds = 0;           // dynamic LDS bytes
};
SweepRoute sweep_route_decide(const Dims& d);
int launch_sweep(const Ctx& c, hipStream_t st);
void launch_sweep_tables(const Ctx& c, hipStream_t st);
size_t sweep_tab_ints(int A);
void launch_loglik(const Ctx& c, int use_rss_part, int r_stored, hipStream_t st);
void launch_loglik_flush(const Ctx& c, hipStream_t st, uint32_t* status_out);
void launch_fill_slots(const Ctx& c, double* chain, const double* cur, size_t len, int s0, int s1, hipStream_t st);
void prepare_sweep_kernels();

// ---- kernels_cov.hip ----
// What the eta / Xi block of a run's Dims (MD set) and mask launches: everything cov_route_decide decides, and all
// launch_cov_block reads to choose an instance.
struct CovRoute {
  int BW = 0;               // band class of k_cov_group (template argument)
  int LPC = 0;              // lanes per curve of k_cov_group: 32 or 64
  int DX = 0;               // its exact-D instance, or 0: the general one
  int W2D = 0;              // the D instance of k_cov_w2
  int PP = 0;               // k_cov_factor<PP>
  int NB2 = 0, NBS = 0, NPG = 0;      // curve chunks of k_cov_w2, workgroups of k_cov_group, in-group pairs
  int launches = 0;         // k_cov_group launches of one iteration (the closing residual pass included)
  bool do_eta = false, do_xi = false;
  size_t lds_group = 0;     // dynamic LDS bytes of k_cov_group
};
CovRoute cov_route_decide(const Ctx& c);
void launch_cov_block(const Ctx& c, hipStream_t st);
int cov_step_blocks(int nblk_curve);
int cov_w2_chunks(int n);
void prepare_cov_kernels();
bool cov_block_fits(const Ctx& c);

// ---- kernels_curve_ll.hip ----
// per-curve marginal log-density of curves [i0, i0 + rows), every chain, slots [first_slot, first_slot + n_slots) into
// out[(i - i0) C S + q S + (t - first_slot)] (device); "" or what the kernel cannot take
std::string launch_chain_curve_ll(const Ctx& c, int first_slot, int n_slots, int i0, int rows, double* out, hipStream_t st);

// ---- kernels_slot_ll.hip ----
// Log-likelihood of the chain slots given the scores.  launch_slot_rss: rss_i of curves [i0, i0 + rows), every chain,
// slots [first_slot, first_slot + n_slots) into part[(i - i0) C S + q S + (t - first_slot)] (device).  launch_slot_ll_reduce: those
// rows added in curve order to acc[q S + t], which holds the sums of curves [0, i0); per_curve: the rows become l_i; the chunk that
// ends at curve n leaves loglik(q, t) in acc and, with store, in the "loglik" slots of the range of every chain.  The chunks of a
// call must come in ascending order.  "" or what the kernel cannot take.
std::string launch_slot_rss(const Ctx& c, int first_slot, int n_slots, int i0, int rows, double* part, hipStream_t st);
std::string launch_slot_ll_reduce(const Ctx& c, int first_slot, int n_slots, int i0, int rows, int per_curve, int store, double* part,
                                  double* acc, hipStream_t st);

// ---- kernels_loo_pointwise.hip ----
// A row tile of bfmmm_chain_loo_pointwise: `rows` <= LP_ROWS consecutive observations of `curve`, the first of them at
// y[y0] and at basis row b0 of the launch's B (the multivariate model reads neither), their values in rows out_row .. of the chunk's
// matrices.  The host lists the tiles of a chunk in the order of the result.
constexpr int LP_ROWS = 64;
struct LpTile { int32_t curve, rows; int64_t y0, b0, out_row; };
std::string loo_pointwise_check(const Ctx& c);
std::string launch_loo_pointwise(const Ctx& c, const LpTile* tiles, long long n_tiles, const double* B, const double* y, int first_slot,
                                 int n_slots, double* out, size_t out_stride, hipStream_t st);
std::string launch_loo_pointwise_var(const double* mean, double* second, size_t count, hipStream_t st);

// ---- kernels_loo_blocks.hip ----
// bfmmm_chain_loo_blocks.  A row of a tile is one listed observation: `obs` its index within the curve, b its basis row
// in the launch's B (the multivariate model reads none), bpos the tile row at which its block begins and blen the block's length.
// A tile: `rows` <= LP_ROWS such rows of `curve`, whole blocks only, at rows row0 .. of the chunk's row table and of its matrices;
// y0: the curve's first observation in y.  The host lists tiles and rows in the order of the result.
struct LbRow { int64_t b; int32_t obs; int16_t bpos, blen; };
struct LbTile { int32_t curve, rows; int64_t y0, row0; };
std::string loo_blocks_check(const Ctx& c);
std::string launch_loo_blocks(const Ctx& c, const LbTile* tiles, long long n_tiles, const LbRow* rows, const double* B, const double* y,
                              int first_slot, int n_slots, double* out, size_t out_stride, hipStream_t st);

// ---- kernels_curve_fit.hip ----
// One call of bfmmm_chain_curve_fit / _bands: which (0 mean, 1 fit), the G x P evaluation basis E, the curve of every result
// row (null: curve r), the slot range and the call's projection table of G fit_directions() C n_slots doubles (all device).
struct FitCall {
  int which = 0, G = 0, first_slot = 0, n_slots = 0;
  const double* E = nullptr;
  const int* curves = nullptr;
  double* tab = nullptr;
};
long long fit_directions(const Dims& d, int which);
int fit_lds_rows();                 // C S of the last row k_fit_rows sorts in LDS
std::string fit_check(const Ctx& c, const FitCall& f);
std::string launch_fit_project(const Ctx& c, const FitCall& f, hipStream_t st);
// result rows [r0, r0 + rows): mean / sd [r G + g] and quant [(r G + g) nq + q] of the chunk (r from 0), rows of <= fit_lds_rows() draws
std::string launch_fit_rows(const Ctx& c, const FitCall& f, int r0, int rows, const double* probs, int nq, double* mean, double* sd,
                            double* quant, hipStream_t st);
// the values out[((r G + g) C + q) S + s] of the chunk
std::string launch_fit_values(const Ctx& c, const FitCall& f, int r0, int rows, double* out, hipStream_t st);
// the quantile rule read off ncol sorted rows W[col NP + .] of T values: quant[col nq + q]
std::string launch_fit_quantiles(const double* W, int NP, int T, long long ncol, const double* probs, int nq, double* quant, hipStream_t st);
// Simultaneous bands (bfmmm_chain_curve_bands_sim) of result rows [r0, r0 + rows), p = 1 - alpha, one workgroup per row, G <=
// fit_sim_gmax(): mean / sd [r G + g] of the chunk; rows of <= fit_lds_rows() draws also crit [r], lower / upper [r G + g].  Longer
// rows: C [r CS + cs] into cw; once it is sorted and crit read off it (launch_bands_quantiles, launch_fit_quantiles),
// launch_fit_sim_band writes lower and upper.
int fit_sim_gmax();
std::string launch_fit_sim(const Ctx& c, const FitCall& f, int r0, int rows, double p, double* mean, double* sd, double* crit, double* lower,
                           double* upper, double* cw, hipStream_t st);
std::string launch_fit_sim_band(const double* mean, const double* sd, const double* crit, int G, int rows, double* lower, double* upper,
                                hipStream_t st);

// ---- kernels_similarity.hip ----
// Pooled co-membership d_ij = sum_k Z_ik Z_jk of result rows [r0, r0 + rows) against all n curves over every chain and slots
// [first_slot, first_slot + n_slots): mean[r n + j], sd[r n + j] (null: no second pass) and chain_mean[(r C + q) n + j] (null:
// not written) of the chunk (r from 0, device).  curves: the chunk's curve list on the device, or null: row r is curve r0 + r.
std::string launch_similarity(const Ctx& c, int first_slot, int n_slots, const int* curves, int r0, int rows, double* mean, double* sd,
                              double* chain_mean, hipStream_t st);
extern int g_similarity_block;      // bfmmm_set_similarity_block: 0 the launcher decides, 1 blocks of 64 x 64, 2 of 16 x 64
// The least-squares loss of every draw against that mean over the 64 x 64 blocks (rb, cb), rb <= cb, of the full
// matrix, numbered rows first: similarity_loss_blocks(n) of them.  launch_similarity_loss: partial[b N + q S + t], the sum of
// (d - mean)^2 over block b0 + b of draw (q, t), for b < nb (N = C n_slots; device).  launch_similarity_loss_reduce:
// loss[q S + t] = sum of w partial over those blocks in order, w = 1 for rb = cb and 2 above, continued from what loss holds
// where b0 > 0.
long long similarity_loss_blocks(int n);
std::string launch_similarity_loss(const Ctx& c, int first_slot, int n_slots, long long b0, long long nb, double* partial, hipStream_t st);
std::string launch_similarity_loss_reduce(const Ctx& c, int first_slot, int n_slots, long long b0, long long nb, const double* partial,
                                          double* loss, hipStream_t st);

// ---- kernels_align.hip ----
// Label alignment against a pivot.  launch_align_gram: of every draw (q, t) of every chain and slots [first_slot,
// first_slot + n_slots), perm[(q S + s) K + l], the exact maximiser of sum_l A[perm(l)][l], A = Z(q, t)' Zref (Zref n x K
// column-major), and score[q S + s] (null: not written) that sum (all device).  launch_align_gather: diag_gather with the
// component index k of element e = a + inner (k + K b) read from perm[k] of the draw (inner 0: no component axis).
// launch_align_project: rows [r0, r0 + rows) (<= 65535) of the K G cluster mean functions on E (G x P), row = k + K g, into
// V[q S + s + C S (row - r0)].
std::string launch_align_gram(const Ctx& c, const double* Zref, int first_slot, int n_slots, int32_t* perm, double* score, hipStream_t st);
std::string launch_align_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S, int C, int p0, int P,
                                const int32_t* perm, int K, long long inner, double* ws, hipStream_t st);
std::string launch_align_project(const Ctx& c, const double* E, int G, const int32_t* perm, int first_slot, int n_slots, int r0, int rows,
                                 double* V, hipStream_t st);

// ---- kernels_rescale.hip ----
// The reference's rescale step per draw.  launch_rescale_transform: of every draw cs = q S + s of every chain and
// slots [first_slot, first_slot + n_slots), mix[(cs K + k) K + c] = A, mix_inv[(cs K + c) K + k] = A^-1, curve[cs K + k], rcond[cs]
// z_min[cs] and singular_flag[cs] (1: singular; all device).  given null: the rule, A[k][.] = the Z row of the first curve that attains max_i Z[i, perm[k]] (perm
// null: the identity); else A = given (N K K) and curve = -1.  A singular draw: A^-1 and z_min NaN, rcond 0.
// launch_rescale_gather: launch_align_gather with element e = a + inner (k + K b) = sum_c W[cs K K + k sk + c sc] src[a + inner (c +
// K b)], inner >= 1.  launch_rescale_project: launch_align_project of sum_c A[k][c] (nu_c + sum_d x_d eta_c,d), x of D entries or null.
std::string launch_rescale_transform(const Ctx& c, const int32_t* perm, const double* given, int first_slot, int n_slots, double* mix,
                                     double* mix_inv, int32_t* curve, double* rcond, double* z_min, int32_t* singular_flag, hipStream_t st);
std::string launch_rescale_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S, int C, int p0, int P,
                                  const double* W, int sk, int sc, int K, long long inner, double* ws, hipStream_t st);
std::string launch_rescale_project(const Ctx& c, const double* E, int G, const double* mix, const double* x, int first_slot, int n_slots,
                                   int r0, int rows, double* V, hipStream_t st);

// ---- kernels_curve_cov.hip ----
// One call of bfmmm_chain_curve_cov: the evaluation bases E1 (G1 x P) and E2 (G2 x P; null: E2 = E1, G2 = G1), whether only the
// diagonal g = h is wanted (E2 null), the curve of every result row of the call (null: curve r), the slot range and the call's
// projection tables of cov_table_doubles(.., 0 / 1) doubles (tab2 null where E2 is; all device).
struct CovCall {
  int G1 = 0, G2 = 0, diagonal = 0, first_slot = 0, n_slots = 0;
  const double *E1 = nullptr, *E2 = nullptr;
  const int* curves = nullptr;
  double *tab1 = nullptr, *tab2 = nullptr;
};
std::string cov_check(const Ctx& c, const CovCall& f);
size_t cov_table_doubles(const Ctx& c, const CovCall& f, int which);
std::string launch_cov_project(const Ctx& c, const CovCall& f, hipStream_t st);
// result rows [r0, r0 + rows) of the call: mean / sd [(r G1 + g) G2 + h] and chain_mean [((r C + q) G1 + g) G2 + h] of the chunk
// (r from 0; diagonal: [r G1 + g], [(r C + q) G1 + g]); sd, chain_mean may be null
std::string launch_curve_cov(const Ctx& c, const CovCall& f, int r0, int rows, double* mean, double* sd, double* chain_mean, hipStream_t st);

// ---- kernels_cluster_cov.hip ----
// One call of bfmmm_chain_cluster_cov_bands: the evaluation bases E1 (G1 x P) and E2 (G2 x P; null: E2 = E1, G2 =
// G1), whether only the diagonal g = h is wanted (E2 null), the permutation rows perm[(q S + s) K + .], the n_pairs pairs
// pairs[2 r], pairs[2 r + 1] of aligned components, the covariate setting x (D entries; null: phi alone), the slot range and the
// call's projection tables of ccov_table_doubles(.., 0 / 1) doubles (tab2 null where E2 is; all device).
struct CcovCall {
  int G1 = 0, G2 = 0, diagonal = 0, first_slot = 0, n_slots = 0;
  long long n_pairs = 0;
  const double *E1 = nullptr, *E2 = nullptr, *x = nullptr;
  const int32_t *perm = nullptr, *pairs = nullptr;
  const double* mix = nullptr;      // bfmmm_chain_cluster_cov_bands_rescaled: A[(cs K + k) K + c] of every draw, in place of perm
  double *tab1 = nullptr, *tab2 = nullptr;
};
std::string ccov_check(const Ctx& c, const CcovCall& f);
size_t ccov_table_doubles(const Ctx& c, const CcovCall& f, int which);
std::string launch_ccov_project(const Ctx& c, const CcovCall& f, hipStream_t st);
// the values V[cs + N (e - r0)] of result rows e in [r0, r0 + rows), e = (r G1 + g) G2 + h (diagonal: r G1 + g), N = C n_slots
std::string launch_ccov_values(const Ctx& c, const CcovCall& f, long long r0, long long rows, double* V, hipStream_t st);
// dev[r N + cs] = max(dev, |(v - mean) / sd|) over the entries of pair r among those rows (sd = 0 skipped, NaN kept); V, mean and
// sd are the chunk's (entry r0 first), dev the call's
std::string launch_ccov_maxdev(const CcovCall& f, long long N, long long r0, long long rows, const double* V, const double* mean,
                               const double* sd, double* dev, hipStream_t st);
// crit[r] = quantile p of dev[r N + .] for r < m, rows of at most ccov_sort_rows() draws, interpolated without an fma
int ccov_sort_rows();
std::string launch_ccov_crit(const double* dev, long long N, long long m, double p, double* crit, hipStream_t st);

// ---- kernels_cluster_contrast.hip ----
// One call of bfmmm_chain_cluster_contrast_bands: the evaluation basis E (G x P), the label map of every draw
// mix[(cs K + k) K + c], the R contrasts w_nu[r K + k] and w_eta[(r K + k) D + d] (null: nu alone), the quadrature weights w (G), the
// slot range and the call's coefficient table tab[(r P + p) N + cs], N = C n_slots.  All device.
struct ContrastCall {
  int G = 0, R = 0, first_slot = 0, n_slots = 0;
  const double *E = nullptr, *mix = nullptr, *w_nu = nullptr, *w_eta = nullptr, *w = nullptr;
  double* tab = nullptr;
};
std::string contrast_check(const Ctx& c, const ContrastCall& f);
// tab: b_r[p] of every draw
std::string launch_contrast_coef(const Ctx& c, const ContrastCall& f, hipStream_t st);
// the values V[cs + N (e - r0)] of result rows e = r G + g in [r0, r0 + rows), rows <= 65535
std::string launch_contrast_values(const Ctx& c, const ContrastCall& f, long long r0, long long rows, double* V, hipStream_t st);
// acc[r N + cs] += w_g v^2 over the chunk's rows of contrast r, g ascending; where the chunk holds the contrast's last row the
// square root takes the sum's place.  The chunks of a call must come in ascending order, acc starts from 0.0
std::string launch_contrast_norm(const Ctx& c, const ContrastCall& f, long long r0, long long rows, const double* V, double* acc, hipStream_t st);
// count[row] = #{cs < N : V[row N + cs] > thr[row]} (ge: >=) for row < rows; thr null: 0.0 for every row
std::string launch_rows_count(const double* V, long long N, long long rows, const double* thr, int ge, int32_t* count, hipStream_t st);

// ---- kernels_cluster_eig.hip ----
// One call of bfmmm_chain_cluster_eigen: the grid basis E (G x P), the weights w (G; null: 1), the covariate
// setting x (D entries; null: phi alone), the reference functions ref (K J G; null: the largest-entry rule), the permutation
// rows perm[(q S + s) K + .], the J leading eigenfunctions wanted, the slot range, and what the kernels fill: Q (P P), R (K J P;
// with ref), the rows lam / pve [cs + N (k M + j)] and tot [cs + N k], the signed b [((cs K + k) J + j) P + p] and the status
// words [cs K + k] (the sweeps; bit 0x100: the cap of ceig_sweep_cap() sweeps was reached).  All device.
struct CeigCall {
  int G = 0, J = 0, first_slot = 0, n_slots = 0;
  const double *E = nullptr, *w = nullptr, *x = nullptr, *ref = nullptr;
  const int32_t* perm = nullptr;
  double *Q = nullptr, *R = nullptr, *lam = nullptr, *pve = nullptr, *tot = nullptr, *b = nullptr;
  int32_t* status = nullptr;
};
extern int g_cluster_eig_form;      // bfmmm_set_cluster_eig_form: 0 the launcher decides, 1 plain multiplies and additions, 2 MFMA
std::string ceig_check(const Ctx& c, const CeigCall& f);
int ceig_sweep_cap();
std::string launch_ceig_gram(const Ctx& c, const CeigCall& f, hipStream_t st);
std::string launch_ceig_solve(const Ctx& c, const CeigCall& f, hipStream_t st);
// the values V[cs + N (e - r0)] of result rows e in [r0, r0 + rows), e = (k J + j) G + g, N = C n_slots
std::string launch_ceig_values(const Ctx& c, const CeigCall& f, long long r0, long long rows, double* V, hipStream_t st);

// ---- kernels_predict.hip ----
// One call of bfmmm_chain_predict: the records rec (n_new x LREC) and point counts ni of the new curves, their
// covariates X (n_new x D column-major; null without covariates), the permutation rows perm[(q S + s) K + .] (null: identity), the
// sample table zs[(cs J + j) K + k] (null: variates are drawn), J samples in each of R stages, the seed and the slot range.  All
// device.
struct PredictCall {
  int n_new = 0, J = 0, R = 0, first_slot = 0, n_slots = 0;
  unsigned long long seed = 0;
  const double *rec = nullptr, *X = nullptr, *zs = nullptr;
  const int* ni = nullptr;
  const int32_t* perm = nullptr;
};
// "" or what k_predict cannot take; *lds_bytes: the dynamic LDS a workgroup needs
std::string predict_check(const Ctx& c, const PredictCall& f, size_t* lds_bytes);
// new curves [r0, r0 + rows) of the call into the chunk's traces (r from 0, N = C n_slots): lpd_t, ess_t [r N + cs], m_t, q_t
// [(r N + cs) K + l] (relabelled by perm), prop [((r N + cs) R + st) K + k] and samples [(((r N + cs) R + st) J + j) K + k] (either
// may be null; so may m_t and q_t, together) and a_last [(r N + cs) K + k], the proposal of the last stage (null: not stored)
std::string launch_predict(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                           double* prop, double* samples, hipStream_t st, double* a_last = nullptr);
// the pooled results of the chunk's rows from its traces: lpd, ess_mean, ess_min [r], z_mean, z_sd [r K + l]
std::string launch_predict_pool(int K, long long N, int rows, const double* lpd_t, const double* ess_t, const double* m_t, const double* q_t,
                                double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min, hipStream_t st);

// ---- kernels_predict_fit.hip ----
// One call of bfmmm_chain_predict_fit: the call of 7m, the evaluation basis E (G x P, device) and whether the
// observation noise is added to the variance and the paths.
struct PredictFitCall {
  PredictCall p;
  const double* E = nullptr;
  int G = 0, noise = 0;
};
// "" or what k_predict_fit cannot take (what k_predict cannot take included, under its name); *lds_bytes: the dynamic LDS of a workgroup
std::string predict_fit_check(const Ctx& c, const PredictFitCall& f, size_t* lds_bytes);
// launch_predict's traces of the chunk, bit for bit, and with them mu_t, var_t, path_t [(r G + g) N + cs], path_idx, path_u [r N + cs]
// and path_xi [(r N + cs) M + m]
std::string launch_predict_fit(const Ctx& c, const PredictFitCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                               double* prop, double* samples, double* mu_t, double* var_t, double* path_t, int32_t* path_idx, double* path_u,
                               double* path_xi, hipStream_t st);
// mean and sd [col] of the ncol = rows G columns of N draws: the draws pooled with equal weights, sd of the whole mixture (N, not N - 1)
std::string launch_predict_fit_pool(long long N, long long ncol, const double* mu_t, const double* var_t, double* mean, double* sd, hipStream_t st);

// ---- kernels_loo_marginal.hip ----
// The refinement of bfmmm_chain_loo_marginal over a chunk of `rows` curves from r0 on, whose traces lpd_t, ess_t
// [r N + cs] and a_last [(r N + cs) K + k] launch_predict left (r from 0, N = C n_slots).  A pair is selected where ess_t < floor
// or lpd_t is not finite.
// "" or what k_lz_refine cannot take with J2 samples in each of R2 stages; *lds_bytes: the dynamic LDS of a workgroup
std::string lz_check(const Ctx& c, int J2, int R2, size_t* lds_bytes);
// cnt[r]: the selected pairs of row r; where given, ess_mean[r] and ess_min[r] of the row
std::string launch_lz_count(long long N, int rows, const double* lpd_t, const double* ess_t, double ess_floor, int32_t* cnt, double* ess_mean,
                            double* ess_min, hipStream_t st);
// the selected pairs of row r as (curve r0 + r, chain, slot relative to first_slot) at list + 3 off[r], in increasing cs; off: the
// exclusive prefix of the counts, n_list their sum, the entries the list holds
std::string launch_lz_list(long long N, int S, int r0, int rows, const double* lpd_t, const double* ess_t, double ess_floor, const int64_t* off,
                           long long n_list, int32_t* list, hipStream_t st);
// One workgroup per listed pair runs pred_draw once more with f.J = J2 and f.R = R2 from the pair's a_last and overwrites its lpd_t
// and ess_t; prop [(e R2 + st) K + k] and samples [((e R2 + st) J2 + j) K + k] of list entry e (either may be null)
std::string launch_lz_refine(const Ctx& c, const PredictCall& f, int r0, int rows, const int32_t* list, long long n_list, double* lpd_t,
                             double* ess_t, const double* a_last, double* prop, double* samples, hipStream_t st);

// ---- kernels_predict_laplace.hip ----
// The Laplace mixture proposal for the integral of bfmmm_chain_predict: f.R and f.zs are not read.
// "" or what k_predict_lap cannot take; *lds_bytes: the dynamic LDS a workgroup needs
std::string predict_lap_check(const Ctx& c, const PredictCall& f, size_t* lds_bytes);
// the doubles of one slot of `comps`: the centre (K - 1), the packed lower L ((K - 1) K / 2), g_c and J_c
int predict_lap_comp_doubles(int K);
// launch_predict's lpd_t, ess_t, m_t and q_t of the chunk under the mixture proposal, and n_modes [r N + cs], comps
// [((r N + cs)(K + 2) + c) predict_lap_comp_doubles(K) + .] and eta [((r N + cs) J + j)(K - 1) + i] (the last two may be null)
std::string launch_predict_lap(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                               int32_t* n_modes, double* comps, double* eta, hipStream_t st);

// ---- kernels_bands.hip ----
// The column reductions of the credible-band entry points on device tables V[t + T col], on stream st.  quantiles: LDS sort
// for T <= 8192 (W unused), else k_bands_quantiles_big over the workspace W of NP ncol doubles, NP = bands_sort_pad(T), which
// it leaves holding the sorted columns; out[q + nq col].  moments: mean and sd (N - 1) per column.
int bands_sort_pad(int T);
std::string launch_bands_quantiles(const double* V, int T, long long ncol, double* W, const double* probs, int nq, double* out, hipStream_t st);
std::string launch_bands_moments(const double* V, int T, long long ncol, double* mean, double* sd, hipStream_t st);

#ifdef BFMMM_TIMELINE
void fetch_wgtrace(unsigned long long* out);      // kernels_pair_gram.hip
void fetch_ztrace(unsigned long long* out);       // kernels_curve.hip
void fetch_zphase(unsigned long long* out);       // kernels_curve.hip
void fetch_fct(unsigned long long* out);          // kernels_factor.hip
#endif

}  // namespace bfmmm
