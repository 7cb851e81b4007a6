// What the host files share (bfmmm_capi.hip, the driver, and capi_chain.hip, capi_cluster.hip and capi_loo.hip, the chain-slot post-processing): the handle,
// the kernel-family ids of its timing tables, the HIP error check and three helpers the driver defines.
#pragma once
#include "../../include/bfmmm.h"
#include "model.hpp"

#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#define HIPCHK(x)                                                                                   \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) {                                                                         \
      (void)hipGetLastError(); /* (not sticky: a caller that retries with a smaller batch starts clean) */ \
      char buf_[512];                                                                               \
      snprintf(buf_, sizeof buf_, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #x); \
      return bfmmm::fail(buf_);                                                                     \
    }                                                                                               \
  } while (0)

enum { FAM_TOTAL = 0, FAM_Z, FAM_PG, FAM_FACTOR, FAM_SWEEP, FAM_CHI, FAM_LOGLIK, FAM_REDUCE, FAM_COUNT };

// The timers of the chain-slot calls (capi_chain.hip, capi_cluster.hip, capi_loo.hip), from HIP events around their launches, and their public names: PT_CURVE_LL
// is read by bfmmm_debug_get, the others by bfmmm_get_timing ("curve_fit": the sum of the four PT_FIT_*).  PT_SIM: k_fit_sim and
// k_fit_sim_band, PT_SIM_REDUCE: the long-row sort; PT_COV_PROJECT counts the tables filled (1 or 2), not its launches;
// PT_SIM_LOSS: k_similarity_loss, PT_SIM_LOSS_REDUCE: k_similarity_loss_reduce, one launch each per chunk; PT_ALIGN_GRAM:
// k_align_gram (one launch), PT_ALIGN_GATHER: k_align_gather, PT_ALIGN_PROJECT: k_align_project, one launch each per chunk;
// PT_CCOV_PROJECT: k_ccov_project, counting the tables filled (1 or 2), PT_CCOV: k_ccov_values, one launch per chunk and sweep
// over the chunks, PT_CCOV_MAXDEV: k_ccov_maxdev, one launch per chunk; PT_CEIG_GRAM: k_ceig_gram, PT_CEIG: k_ceig_solve, one launch
// each per call, PT_CEIG_VALUES: k_ceig_values, one launch per chunk; PT_PREDICT_STATS: the records of the new curves (one launch,
// none for a from-basis handle), PT_PREDICT: k_predict and k_predict_pool, one launch each per chunk; PT_PREDICT_FIT: what
// bfmmm_chain_predict_fit launches in their place, k_predict_fit, k_predict_pool, k_predict_fit_pool and the quantiles of the paths;
// PT_LOO_POINTWISE: what bfmmm_chain_loo_pointwise launches on the sampler's stream (the dense basis rows once, k_loo_pointwise and,
// where the variance trace is asked for, k_loo_pointwise_var per chunk), PT_LOO_POINTWISE_PSIS: its PSIS pass, one per chunk;
// PT_LOO_MARGINAL: what bfmmm_chain_loo_marginal launches on the sampler's stream, per chunk k_predict, k_lz_count twice and, where
// pairs are refined, k_lz_list and k_lz_refine; PT_LOO_MARGINAL_PSIS: its PSIS pass, one launch per chunk; PT_LOO_BLOCKS: what
// bfmmm_chain_loo_blocks launches on the sampler's stream (the dense basis rows once, k_loo_blocks and, where the variance trace is
// asked for, k_loo_pointwise_var per chunk), PT_LOO_BLOCKS_PSIS: its PSIS pass, one per chunk; PT_CONTRAST_COEF: k_contrast_coef (one
// launch a call), PT_CONTRAST_VALUES: k_contrast_values, one launch per chunk and sweep over the chunks, PT_CONTRAST_NORM:
// k_contrast_norm, one launch per chunk; PT_SLOT_LL: k_slot_rss, PT_SLOT_LL_REDUCE: k_slot_ll_reduce, one launch each per chunk.
enum { PT_CURVE_LL = 0, PT_FIT_PROJECT, PT_FIT_ROWS, PT_FIT_VALUES, PT_FIT_REDUCE, PT_SIM, PT_SIM_REDUCE, PT_SIMILARITY,
       PT_COV_PROJECT, PT_COV, PT_SIM_LOSS, PT_SIM_LOSS_REDUCE, PT_ALIGN_GRAM, PT_ALIGN_GATHER, PT_ALIGN_PROJECT,
       PT_CCOV_PROJECT, PT_CCOV, PT_CCOV_MAXDEV, PT_CEIG_GRAM, PT_CEIG, PT_CEIG_VALUES, PT_PREDICT_STATS, PT_PREDICT, PT_PREDICT_FIT,
       PT_LOO_MARGINAL, PT_LOO_MARGINAL_PSIS, PT_PREDICT_LAPLACE, PT_LOO_MARGINAL_LAPLACE, PT_LOO_POINTWISE, PT_LOO_POINTWISE_PSIS,
       PT_RESCALE_TRANSFORM, PT_RESCALE_GATHER, PT_RESCALE_PROJECT, PT_LOO_BLOCKS, PT_LOO_BLOCKS_PSIS, PT_CONTRAST_COEF,
       PT_CONTRAST_VALUES, PT_CONTRAST_NORM, PT_SLOT_LL, PT_SLOT_LL_REDUCE, PT_COUNT };
inline constexpr const char* kPostNames[PT_COUNT] = {"curve_ll_ms", "curve_fit_project", "curve_fit_rows", "curve_fit_values",
                                                     "curve_fit_reduce", "curve_sim", "curve_sim_reduce", "similarity",
                                                     "curve_cov_project", "curve_cov", "similarity_loss", "similarity_loss_reduce",
                                                     "align_gram", "align_gather", "align_project",
                                                     "cluster_cov_project", "cluster_cov", "cluster_cov_maxdev",
                                                     "cluster_eig_gram", "cluster_eig", "cluster_eig_values",
                                                     "predict_stats", "predict", "predict_fit",
                                                     "loo_marginal", "loo_marginal_psis", "predict_laplace",
                                                     "loo_marginal_laplace", "loo_pointwise", "loo_pointwise_psis",
                                                     "rescale_transform", "rescale_gather", "rescale_project",
                                                     "loo_blocks", "loo_blocks_psis",
                                                     "contrast_coef", "contrast_values", "contrast_norm",
                                                     "slot_loglik", "slot_loglik_reduce"};

struct bfmmm_handle {
  bfmmm_config cfg;
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t evA = nullptr;
  bfmmm::Ctx c;                // template context (full MD); its per-chain pointers are those of chain 0 of the batch
  int nch = 1;                 // chains in the batch (bfmmm_create_batch), all advanced in lockstep by bfmmm_run
  int sel = 0;                 // the chain the state / chain accessors address (bfmmm_select_chain)
  int T = 0;
  int64_t n_obs = 0;
  // raw inputs kept on the device for bfmmm_get_basis
  double* d_t = nullptr; double* d_y = nullptr; int64_t* d_off = nullptr; double* d_knots = nullptr; int n_knots = 0;
  std::vector<void*> allocs;
  char* arena = nullptr;               // base of the per-chain arena (chain q at arena + q * c.chain_bytes)
  char* arena_cov = nullptr;           // the same for the covariate buffers (c.chain_bytes_cov)
  uint32_t* status_host = nullptr;     // pinned, host-mapped: the chains' status words after a run
  uint32_t* status_dev = nullptr;      // its device address (written by the run's last kernel)
  size_t pg_part_doubles = 0;
  static constexpr int MAX_SUB = 4;
  // snapshot of the chains' work state for the dry launch of freshly captured graphs (bfmmm_prepare_run)
  char* dry_snap = nullptr;
  size_t dry_snap_bytes = 0;
  // packed partial tiles of k_pair_gram_pack, one buffer per sub-batch stream (+ one for the whole batch on one stream)
  double* pg_pack[MAX_SUB + 1] = {};
  size_t pg_pack_doubles[MAX_SUB + 1] = {};
  hipStream_t sub_st[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr};     // [0] = st
  hipEvent_t sub_ev[MAX_SUB] = {nullptr, nullptr, nullptr, nullptr};
  // Captured graphs of runs with the key below, oldest first: (sub-batch, kind, repetitions) -> graph (run_impl)
  struct CachedGraph { int sub, kind, reps; hipGraphExec_t g; };
  std::vector<CachedGraph> graphs;
  using GraphKey = std::tuple<uint32_t, int, uint64_t, uint32_t, int, int>;      // (mask, MD, seed, chain, nsub, instance switches)
  GraphKey g_key;
  bool g_valid = false;                // the cached graphs were captured for g_key
  int last_md = -1;
  double last_route[6] = {0, 0, 0, -1, 0, 0};  // bfmmm_debug_get("pg_route"): {packed, KS, NKS, body, G, tail} of sub-batch 0 of the last run
  double last_sweep[5] = {-1, 0, 0, 0, 0};     // bfmmm_debug_get("sweep_route"): {kernel, template argument, mv, direct, block threads} of the last run
  // bfmmm_debug_get("curve_route"): the last Z update of the last run {form (0 none, 1 stand-alone, 2 lean trailing, 3 fused into
  // k_curve_chi), BW, LPC, COV, KT, KEX}, then its last k_curve_chi launch {BW, LPC, COV, SMALL, KX, MX, mode, whether the
  // run's earlier chi launches ran the next Z update} (BW -1: no such launch)
  double last_curve[14] = {0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0};
  // bfmmm_debug_get("cov_route"): what launch_cov_block launches in every iteration of the last run {BW, LPC, DX (0 general), the D
  // instance of k_cov_w2, PP of k_cov_factor, NB2, NBS, NPG, k_cov_group launches, do_eta, do_xi} (BW -1: no covariates)
  double last_cov[11] = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // bfmmm_debug_get("hyper_route"): where the scalar jobs of the last run ride (scalar_jobs.hpp) {job_hyper: 0 k_curve_chi, 1 the lean
  // k_curve_z of the bodies and k_curve_chi of the closing iteration, 2 deferred to the next k_pair_gram and k_loglik_flush;
  // job_pi_alpha: 0 k_pair_gram, 1 k_pair_gram with the deferred log-likelihood in a workgroup of its own, 2 k_factor;
  // job_pi_prepare workgroups launched} (-1: no run yet)
  double last_hyper[3] = {-1, -1, 0};
  bool pi_flag_stored = false;         // the last run's job_pi_alpha stored its prepared flag (bfmmm_debug_get "pi_prepared")
  int64_t tab_key = -1;                // (MD, mask) the step tables of k_sweep_chain were built for
  int launch_error = 0;                // set while a run's launches are queued: 1 the sweep does not fit, 2 no per-curve instance
  int zrec_form = 0;                   // the Z record of the last run (Ctx::zrec): 0 none stored (recording off, or no Z update in the mask),
                                       // 1 stand-alone or lean update (its "prepared" flag holds), 2 fused update (always prepared)
  int slot_base = 0;                   // chain slot of iteration i is i - slot_base (bfmmm_set_slot_base)
  double* tt_save = nullptr;            // state saved across a tempered-transition block
  // bfmmm_debug_get("tt_trace"): what the last bfmmm_tempered_transition computed on the host {N_t, ladder[0 .. N_t - 1], the beta of
  // sweep l = 1 .. 2 N_t, sig[0 .. 2 N_t], rss[0 .. 2 N_t], log u, logA, accepted} (empty: no block yet)
  std::vector<double> tt_trace;
  std::vector<double> B_host;           // bfmmm_create_from_basis: the caller's basis rows (bfmmm_get_basis)
  bool state_dirty = true;             // the state was changed from the host: proposals prepared on the device are stale
  int profile = 0;
  double fam_ms[FAM_COUNT] = {0};
  int64_t fam_launches[FAM_COUNT] = {0};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double post_ms[PT_COUNT] = {0};      // the timers of the chain-slot calls (kPostNames): device time and launches of a kernel
  int64_t post_launches[PT_COUNT] = {0};   // family in the last call that ran it
};

namespace bfmmm {
int fail(const std::string& msg);      // sets the calling thread's bfmmm_last_error text; returns 1
// synchronous copy on the sampler's own stream
hipError_t copy_sync(bfmmm_handle* h, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
// the context of the selected chain (host view)
Ctx selc(const bfmmm_handle* h);
}
