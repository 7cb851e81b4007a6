// C ABI of the sampler (include/bfmmm.h), what is read off the chain slots after a run: the chain arrays, their convergence
// diagnostics, the per-curve log-density with its diagnostics, the pooled per-curve fitted functions and bands, their simultaneous
// bands, the pooled co-membership matrix of the curves and the least-squares draw against it, the pooled per-curve covariance
// surfaces and the prediction of held-out curves with their fitted functions; and what is written into the slots from outside
// (bfmmm_set_chain) with the log-likelihood of such slots.  The cluster-level calls (alignment, rescale and what is pooled under
// either labelling) are capi_cluster.hip's, the PSIS-LOO family over the chain slots capi_loo.hip's.
// What an entry point is made of is capi_chain.hpp's, shared with those files.
#include "capi_chain.hpp"

namespace {

// ---- the pooled per-curve fitted functions (kernels_curve_fit.hip) -----------------------------------------
struct FitSetup {
  FitCall f;
  int64_t m = 0;                    // curves of the result
  long long CS = 0, NJ = 0;         // draws per row, projection directions
};

// The checks both calls share, then E, the curve list and the projection table on the device (owned by b) and the table
// filled.  shared_bytes: what these take of the budget.
int fit_check_args(const SlotCheck& ck, int which, const double* E, int G, const int32_t* curves, int n_curves, FitSetup& s) {
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"E", E}})) return 1;
  if (which != 0 && which != 1) return fail(fn + ": 'which' must be 0 (mean) or 1 (fit), got " + std::to_string(which));
  if (G < 1) return fail(fn + ": 'G' must be at least 1");
  const bfmmm_handle* h = ck.h;
  if (curves && n_curves < 1) return fail(fn + ": 'n_curves' must be at least 1 where 'curves' is given");
  if (ck.curve_list(curves, n_curves, &s.m) || ck.range() || ck.row_limit()) return 1;
  s.CS = ck.CS();
  s.f.which = which; s.f.G = G; s.f.first_slot = ck.first_slot; s.f.n_slots = ck.n_slots;
  const std::string err = fit_check(h->c, s.f);
  if (!err.empty()) return fail(fn + ": " + err);
  s.NJ = fit_directions(h->c.d, which);
  return 0;
}
size_t fit_shared_bytes(const bfmmm_handle* h, const FitSetup& s) {
  return sizeof(double) * ((size_t)s.CS * s.f.G * (size_t)s.NJ + (size_t)s.f.G * h->c.d.P + 16) + sizeof(int32_t) * (((size_t)s.m + 1) & ~(size_t)1);
}
int fit_prepare(const SlotCheck& ck, const double* E, const int32_t* curves, FitSetup& s, CallBufs& b) {
  bfmmm_handle* h = ck.h;
  double *d_E = nullptr, *d_tab = nullptr;
  int32_t* d_curves = nullptr;
  HIPCHK(b.put(h, &d_E, E, (size_t)s.f.G * h->c.d.P));
  HIPCHK(b.get(&d_tab, (size_t)s.CS * s.f.G * (size_t)s.NJ));
  if (curves) HIPCHK(b.put(h, &d_curves, curves, (size_t)s.m));
  s.f.E = d_E; s.f.curves = d_curves; s.f.tab = d_tab;
  reset_timers(h, PT_FIT_PROJECT, PT_FIT_REDUCE);
  return once(ck, b, PT_FIT_PROJECT, 0, [&] { return launch_fit_project(h->c, s.f, h->st); });
}

}  // namespace

extern "C" int bfmmm_get_chain(bfmmm_handle* h, const char* name, int n_slots, double* out, int64_t capacity) {
  if (!h || !name || !out) return fail("bfmmm_get_chain: null argument");
  if (n_slots < 0 || n_slots > h->T) return fail("bfmmm_get_chain: n_slots out of range");
  HIPCHK(hipSetDevice(h->device));
  const std::string s(name);
  const ChainArr a = chain_array(selc(h), h->T, s);        // of the selected chain of the batch
  HIPCHK(hipStreamSynchronize(h->st));
  if (!a.p) return fail("bfmmm_get_chain: unknown name '" + s + "'");
  if (capacity < a.len * n_slots) return fail("bfmmm_get_chain(" + s + "): buffer too small");
  if (a.ps == 1) HIPCHK(copy_sync(h, out, a.p, sizeof(double) * (size_t)(a.len * n_slots), hipMemcpyDeviceToHost));
  else      // slot fastest on the device (tau): returned n_slots x len column-major
    for (int64_t k = 0; k < a.len; ++k)
      HIPCHK(copy_sync(h, out + (size_t)n_slots * k, a.p + (size_t)a.ps * k, sizeof(double) * (size_t)n_slots, hipMemcpyDeviceToHost));
  return 0;
}

// Every chain of the batch, slots [first_slot, first_slot + n_slots) of `name`: elements are gathered in chunks of
// consecutive elements into the workspace of a RowCall.
extern "C" int bfmmm_chain_diagnostics(bfmmm_handle* h, const char* name, int first_slot, int n_slots, int64_t max_workspace_bytes,
                                       double* rhat, double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean,
                                       double* mean, double* sd, int64_t capacity) {
  SlotCheck ck{"bfmmm_chain_diagnostics", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"name", name}, {"rhat", rhat}, {"ess_bulk", ess_bulk}, {"ess_tail", ess_tail}, {"ess_mean", ess_mean},
               {"mcse_mean", mcse_mean}, {"mean", mean}, {"sd", sd}}) ||
      ck.range() || ck.budget_sign(max_workspace_bytes))
    return 1;
  const Ctx& c = h->c;          // chain 0 of the batch
  const ChainArr a = chain_array(c, h->T, name);
  if (!a.p) return fail(ck.fn + ": unknown name '" + name + "'");
  ck.tag = std::string("(") + name + ")";
  if (ck.capacity(capacity, a.len) || ck.row_limit()) return 1;
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  RowCall rows(ck, a.len, 0, true, -1);
  if (rows.plan(max_workspace_bytes, 0, kNoCap, nullptr, nullptr)) return 1;
  return rows.run(outs, nullptr, nullptr, [&](int64_t p0, int cnt, double* d_x) {
    return diag_gather(a.p, a.cov ? c.chain_bytes_cov : c.chain_bytes, a.ss, a.ps, first_slot, n_slots, h->nch, (int)p0, cnt, d_x, h->st);
  });
}

// ---- per-curve marginal log-density of the chain slots (kernels_curve_ll.hip) ------------------------------
// The n x C x n_slots matrix (draw fastest, then chain, then curve) on the host, computed in chunks of consecutive curves
// on the sampler's stream.
extern "C" int bfmmm_chain_curve_loglik(bfmmm_handle* h, int first_slot, int n_slots, double* out, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_loglik", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"out", out}}) || ck.range()) return 1;
  const int n = h->c.d.n;
  const int64_t per_row = ck.CS();
  if (ck.capacity(capacity, (int64_t)n * per_row)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_CURVE_LL, PT_CURVE_LL);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(((size_t)256 << 20) / (sizeof(double) * (size_t)per_row))));
  CallBufs b;
  double* d_x = nullptr;
  HIPCHK(b.get(&d_x, (size_t)chunk * (size_t)per_row));
  return for_chunks(ck, n, chunk, [&](int64_t i0, int rows) {
    std::string err = curve_ll_timed(ck, (int)i0, rows, d_x);
    if (err.empty()) err = Back{h, i0, rows}(out, d_x, (size_t)per_row).done();
    if (err.empty()) curve_ll_collect(h);
    return err;
  });
}

// The seven statistics of bfmmm_chain_diagnostics for the n rows of that matrix: chunks of consecutive curves are computed
// into the workspace of a RowCall; the matrix never leaves the device.
extern "C" int bfmmm_chain_curve_diagnostics(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes,
                                             double* rhat, double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean,
                                             double* mean, double* sd, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_diagnostics", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"rhat", rhat}, {"ess_bulk", ess_bulk}, {"ess_tail", ess_tail}, {"ess_mean", ess_mean}, {"mcse_mean", mcse_mean},
               {"mean", mean}, {"sd", sd}}) ||
      ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, h->c.d.n) || ck.row_limit())
    return 1;
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  RowCall rows(ck, h->c.d.n, 0, true, PT_CURVE_LL);
  if (rows.plan(max_workspace_bytes, 0, kNoCap, nullptr, nullptr)) return 1;
  return rows.run(outs, nullptr, nullptr, [&](int64_t i0, int cnt, double* d_x) {
    return launch_chain_curve_ll(h->c, first_slot, n_slots, (int)i0, cnt, d_x, h->st);
  });
}

// ---- pooled per-curve fitted functions of the chain slots and their bands (kernels_curve_fit.hip) ----------
namespace bfmmm { int g_curve_fit_route = 0; }
extern "C" void bfmmm_set_curve_fit_route(int route) { bfmmm::g_curve_fit_route = route == 1 ? 1 : 0; }

// The values themselves on the host, in chunks of consecutive result rows.
extern "C" int bfmmm_chain_curve_fit(bfmmm_handle* h, int which, const double* E, int G, const int32_t* curves, int n_curves,
                                     int first_slot, int n_slots, double* out, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_fit", h, first_slot, n_slots};
  FitSetup s;
  if (ck.ptrs({{"h", h}, {"out", out}}) || fit_check_args(ck, which, E, G, curves, n_curves, s)) return 1;
  const int64_t per_curve = (int64_t)G * s.CS;
  if (ck.capacity(capacity, (int64_t)s.m * per_curve)) return 1;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  if (fit_prepare(ck, E, curves, s, b)) return 1;
  Timer values;
  HIPCHK(b.timers({&values}));
  int64_t chunk = std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / (sizeof(double) * (size_t)per_curve)));
  chunk = std::min<int64_t>(std::min<int64_t>(chunk, s.m), std::max<int64_t>(1, (1LL << 30) / G));
  double* d_v = nullptr;
  HIPCHK(b.get(&d_v, (size_t)chunk * per_curve));
  return for_chunks(ck, s.m, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(values, h->st, [&] { return launch_fit_values(h->c, s.f, (int)r0, rows, d_v, h->st); });
    if (err.empty()) err = Back{h, r0, rows}(out, d_v, (size_t)per_curve).done();
    if (err.empty()) collect(h, values, PT_FIT_VALUES);
    return err;
  });
}

// Mean, sd and quantiles of every row; the values stay on the device (rows of up to 8192 draws: in LDS).
extern "C" int bfmmm_chain_curve_bands(bfmmm_handle* h, int which, const double* E, int G, const int32_t* curves, int n_curves,
                                       int first_slot, int n_slots, const double* probs, int nq, int64_t max_workspace_bytes,
                                       double* mean, double* sd, double* quantiles, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_bands", h, first_slot, n_slots};
  FitSetup s;
  if (ck.ptrs({{"h", h}, {"probs", probs}, {"mean", mean}, {"sd", sd}, {"quantiles", quantiles}}) ||
      fit_check_args(ck, which, E, G, curves, n_curves, s) || ck.probs_list(probs, nq, 1, quantiles) || ck.budget_sign(max_workspace_bytes) ||
      ck.capacity(capacity, (int64_t)s.m * G, "rows"))
    return 1;
  const bool lds_rows = s.CS <= fit_lds_rows() && !g_curve_fit_route;
  const SortWs ws(s.CS, true);                              // k_bands_quantiles_big sorts in a workspace
  const bool sort_ws = ws.on;
  const int NP = (int)ws.NP;
  const size_t per_curve = sizeof(double) * (size_t)G * ((size_t)(2 + nq) + (lds_rows ? 0 : (size_t)s.CS + (size_t)NP));
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), fit_shared_bytes(h, s), per_curve, s.m, cells_cap(G), "curve", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  Timer first, reduce;      // k_fit_rows, or k_fit_values and then the sort and the moments of its values
  HIPCHK(b.timers({&first, &reduce}));
  double *d_probs = nullptr, *d_out = nullptr, *d_v = nullptr, *d_w = nullptr;
  HIPCHK(probs_put(b, h, probs, nq, &d_probs));
  HIPCHK(b.get(&d_out, (size_t)chunk * G * (2 + nq)));
  if (!lds_rows) HIPCHK(b.get(&d_v, (size_t)chunk * G * (size_t)s.CS));
  if (sort_ws) HIPCHK(b.get(&d_w, (size_t)chunk * G * (size_t)NP));
  if (fit_prepare(ck, E, curves, s, b)) return 1;
  double* d_mean = d_out;
  double* d_sd = d_out + (size_t)chunk * G;
  double* d_q = d_out + 2 * (size_t)chunk * G;
  return for_chunks(ck, s.m, chunk, [&](int64_t r0, int rows) {
    const long long ncol = (long long)rows * G;
    std::string err = timed(first, h->st, [&] {
      return lds_rows ? launch_fit_rows(h->c, s.f, (int)r0, rows, d_probs, nq, d_mean, d_sd, d_q, h->st)
                      : launch_fit_values(h->c, s.f, (int)r0, rows, d_v, h->st);
    });
    if (err.empty() && !lds_rows)
      err = timed(reduce, h->st, [&] {
        std::string e = launch_bands_quantiles(d_v, (int)s.CS, ncol, d_w, d_probs, nq, d_q, h->st);
        // the sorted rows are in the workspace: the rule again, rounded as k_fit_rows rounds it
        if (e.empty() && sort_ws) e = launch_fit_quantiles(d_w, NP, (int)s.CS, ncol, d_probs, nq, d_q, h->st);
        if (e.empty()) e = launch_bands_moments(d_v, (int)s.CS, ncol, d_mean, d_sd, h->st);
        return e;
      });
    if (err.empty()) err = Back{h, r0, rows}(mean, d_mean, (size_t)G)(sd, d_sd, (size_t)G)(quantiles, d_q, (size_t)G * nq).done();
    if (!err.empty()) return err;
    collect(h, first, lds_rows ? PT_FIT_ROWS : PT_FIT_VALUES);
    if (!lds_rows) collect(h, reduce, PT_FIT_REDUCE);
    return err;
  });
}

// Simultaneous band of every result row: mean, sd, crit = the (1 - alpha) quantile over the draws of the largest
// standardised deviation over the grid, lower / upper = mean -/+ crit sd.  No value is stored: k_fit_sim forms them three times.
extern "C" int bfmmm_chain_curve_bands_sim(bfmmm_handle* h, int which, const double* E, int G, const int32_t* curves, int n_curves,
                                           int first_slot, int n_slots, double alpha, int64_t max_workspace_bytes,
                                           double* mean, double* sd, double* crit, double* lower, double* upper, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_bands_sim", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  FitSetup s;
  if (ck.ptrs({{"h", h}, {"crit", crit}, {"lower", lower}, {"upper", upper}}) || fit_check_args(ck, which, E, G, curves, n_curves, s)) return 1;
  if (ck.alpha_inside(alpha) || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, (int64_t)s.m * G, "rows")) return 1;
  if (G > fit_sim_gmax())
    return fail(fn + ": 'G' above " + std::to_string(fit_sim_gmax()) + ": mean and sd of a curve's grid points stay in LDS beside its sort row");
  const SortWs ws(s.CS, true);                              // C goes to a workspace row that k_bands_quantiles_big sorts
  const bool sort_ws = ws.on;
  const int NP = (int)ws.NP;
  const size_t per_curve = sizeof(double) * (4 * (size_t)G + 1 + (sort_ws ? (size_t)s.CS + (size_t)NP : 0));
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), fit_shared_bytes(h, s), per_curve, s.m, cells_cap(G), "curve", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  Timer sim, sort, band;      // k_fit_sim; for long rows the sort of their maxima, then k_fit_sim_band
  HIPCHK(b.timers({&sim, &sort, &band}));
  double *d_p = nullptr, *d_out = nullptr, *d_crit = nullptr, *d_c = nullptr, *d_w = nullptr;
  const double p = 1.0 - alpha;
  HIPCHK(b.get(&d_p, 16));
  HIPCHK(b.get(&d_out, 4 * (size_t)chunk * G));
  HIPCHK(b.get(&d_crit, (size_t)chunk));
  if (sort_ws) {
    HIPCHK(b.get(&d_c, (size_t)chunk * (size_t)s.CS));
    HIPCHK(b.get(&d_w, (size_t)chunk * (size_t)NP));
  }
  HIPCHK(copy_sync(h, d_p, &p, sizeof(double), hipMemcpyHostToDevice));
  reset_timers(h, PT_SIM, PT_SIM_REDUCE);
  if (fit_prepare(ck, E, curves, s, b)) return 1;
  double* d_mean = d_out;
  double* d_sd = d_out + (size_t)chunk * G;
  double* d_lo = d_out + 2 * (size_t)chunk * G;
  double* d_up = d_out + 3 * (size_t)chunk * G;
  return for_chunks(ck, s.m, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(sim, h->st, [&] { return launch_fit_sim(h->c, s.f, (int)r0, rows, p, d_mean, d_sd, d_crit, d_lo, d_up, d_c, h->st); });
    if (err.empty() && sort_ws)
      err = timed(sort, h->st, [&] {
        const std::string e = launch_bands_quantiles(d_c, (int)s.CS, rows, d_w, d_p, 1, d_crit, h->st);
        // the sorted rows are in the workspace: the rule again, rounded as k_fit_sim rounds it
        return e.empty() ? launch_fit_quantiles(d_w, NP, (int)s.CS, rows, d_p, 1, d_crit, h->st) : e;
      });
    if (err.empty() && sort_ws) err = timed(band, h->st, [&] { return launch_fit_sim_band(d_mean, d_sd, d_crit, G, rows, d_lo, d_up, h->st); });
    if (err.empty())
      err = Back{h, r0, rows}(mean, d_mean, (size_t)G)(sd, d_sd, (size_t)G)(lower, d_lo, (size_t)G)(upper, d_up, (size_t)G)(crit, d_crit, 1).done();
    if (!err.empty()) return err;
    collect(h, sim, PT_SIM);
    if (sort_ws) {
      collect(h, sort, PT_SIM_REDUCE);
      collect(h, band, PT_SIM);
    }
    return err;
  });
}

// ---- pooled co-membership of curves from the chain slots (kernels_similarity.hip) -----------------------------
extern "C" void bfmmm_set_similarity_block(int block) { bfmmm::g_similarity_block = block == 1 || block == 2 ? block : 0; }

// Mean, sd and per-chain means of d_ij = sum_k Z_ik Z_jk over the draws, in chunks of consecutive result rows; only they
// reach the host.
extern "C" int bfmmm_chain_similarity(bfmmm_handle* h, const int32_t* curves, int n_curves, int first_slot, int n_slots,
                                      int64_t max_workspace_bytes, double* mean, double* sd, double* chain_mean, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_similarity", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"h", h}, {"mean", mean}})) return 1;
  const int n = h->c.d.n, C = h->nch;
  int64_t m = 0;
  if (n_curves < 0) return fail(fn + ": 'n_curves' must not be negative");
  if (ck.curve_list(curves, n_curves, &m) || ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, m * n) || ck.row_limit()) return 1;
  // a result row: its n entries of mean, of sd and of every chain's mean, and its curve index
  const size_t per_row = sizeof(double) * (size_t)n * (1 + (sd ? 1 : 0) + (chain_mean ? (size_t)C : 0)) + (curves ? sizeof(int32_t) : 0);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, per_row, m, 1 << 30, nullptr, &chunk)) return 1;
  reset_timers(h, PT_SIMILARITY, PT_SIMILARITY);
  if (m == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  double *d_mean = nullptr, *d_sd = nullptr, *d_cm = nullptr;
  int* d_curves = nullptr;
  Timer kernel;
  HIPCHK(b.timers({&kernel}));
  HIPCHK(b.get(&d_mean, (size_t)chunk * n));
  if (sd) HIPCHK(b.get(&d_sd, (size_t)chunk * n));
  if (chain_mean) HIPCHK(b.get(&d_cm, (size_t)chunk * C * n));
  if (curves) HIPCHK(b.get(&d_curves, (size_t)chunk));
  return for_chunks(ck, m, chunk, [&](int64_t r0, int rows) {
    if (curves && copy_sync(h, d_curves, curves + r0, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess)
      return std::string("copy of the curve list failed");
    std::string err = timed(kernel, h->st, [&] { return launch_similarity(h->c, first_slot, n_slots, d_curves, (int)r0, rows, d_mean, d_sd, d_cm, h->st); });
    if (err.empty()) err = Back{h, r0, rows}(sd, d_sd, (size_t)n)(chain_mean, d_cm, (size_t)C * n)(mean, d_mean, (size_t)n).done();
    if (err.empty()) collect(h, kernel, PT_SIMILARITY);
    return err;
  });
}

// ---- the least-squares draw of the clustering (kernels_similarity.hip) -------------------------------------------
// loss(q, t) = sum_ij (d_ij(q, t) - mean_ij)^2 of every draw, in chunks of consecutive 64 x 64 blocks of the upper triangle: a
// chunk's per-block sums go through k_similarity_loss_reduce into the loss vector, which stays on the device for diag_launch.
extern "C" int bfmmm_chain_similarity_loss(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes, double* loss,
                                           int64_t capacity, int32_t* best_chain, int32_t* best_slot, double* stats) {
  const SlotCheck ck{"bfmmm_chain_similarity_loss", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"loss", loss}}) || ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, ck.CS()) || ck.row_limit())
    return 1;
  const int C = h->nch, S = n_slots;
  const size_t N = (size_t)ck.CS();
  const int64_t blocks = similarity_loss_blocks(h->c.d.n);
  // shared by all blocks: the loss vector and, where asked for, the seven statistics and the workspace of their row; a block: its N sums
  const size_t stat_doubles = stats ? 7 + diag_row_ws_doubles(C, S) : 0;
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), sizeof(double) * (N + stat_doubles), sizeof(double) * N, blocks, 1 << 30, "block", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_SIM_LOSS, PT_SIM_LOSS_REDUCE);
  CallBufs b;
  double *d_loss = nullptr, *d_part = nullptr, *d_stat = nullptr;
  Timer kernel, reduce;
  HIPCHK(b.timers({&kernel, &reduce}));
  HIPCHK(b.get(&d_loss, N));
  HIPCHK(b.get(&d_part, (size_t)chunk * N));
  if (stats) HIPCHK(b.get(&d_stat, stat_doubles));
  const int rc = for_chunks(ck, blocks, chunk, [&](int64_t b0, int nb) {
    std::string err = timed(kernel, h->st, [&] { return launch_similarity_loss(h->c, first_slot, n_slots, b0, nb, d_part, h->st); });
    if (err.empty()) err = timed(reduce, h->st, [&] { return launch_similarity_loss_reduce(h->c, first_slot, n_slots, b0, nb, d_part, d_loss, h->st); });
    if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = "kernel failed";
    if (!err.empty()) return err;
    collect(h, kernel, PT_SIM_LOSS);
    collect(h, reduce, PT_SIM_LOSS_REDUCE);
    return err;
  });
  if (rc) return rc;
  if (stats) {
    const std::string err = diag_launch(d_loss, 1, C, S, d_stat, 1, d_stat + 7, 1, h->st);
    if (!err.empty()) { (void)hipStreamSynchronize(h->st); return fail(ck.fn + ": " + err); }
    HIPCHK(copy_sync(h, stats, d_stat, sizeof(double) * 7, hipMemcpyDeviceToHost));
  }
  HIPCHK(copy_sync(h, loss, d_loss, sizeof(double) * N, hipMemcpyDeviceToHost));
  // the first minimum in (chain, slot) order
  size_t best = 0;
  for (size_t o = 1; o < N; ++o)
    if (loss[o] < loss[best]) best = o;
  if (best_chain) *best_chain = (int32_t)(best / (size_t)S);
  if (best_slot) *best_slot = first_slot + (int32_t)(best % (size_t)S);
  return 0;
}

// One slot of `name` of the selected chain.
extern "C" int bfmmm_get_slot(bfmmm_handle* h, const char* name, int slot, double* out, int64_t capacity) {
  const std::string fn = "bfmmm_get_slot";
  if (!h) return fail(fn + ": 'h' is null");
  if (!name) return fail(fn + ": 'name' is null");
  if (!out) return fail(fn + ": 'out' is null");
  if (slot < 0 || slot >= h->T) return fail(fn + ": 'slot' out of range");
  HIPCHK(hipSetDevice(h->device));
  const std::string s(name);
  const ChainArr a = chain_array(selc(h), h->T, s);
  if (!a.p) return fail(fn + ": unknown name '" + s + "'");
  if (capacity < a.len) return fail(fn + "(" + s + "): 'capacity' below " + std::to_string(a.len) + " entries");
  HIPCHK(hipStreamSynchronize(h->st));
  if (a.ps == 1) {
    HIPCHK(copy_sync(h, out, a.p + (size_t)a.ss * slot, sizeof(double) * (size_t)a.len, hipMemcpyDeviceToHost));
    return 0;
  }
  // slot fastest on the device (tau): the slot's len entries lie ps doubles apart, one strided copy
  HIPCHK(hipMemcpy2DAsync(out, sizeof(double), a.p + (size_t)a.ss * slot, sizeof(double) * (size_t)a.ps, sizeof(double), (size_t)a.len,
                          hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

// ---- chains from outside and their log-likelihood (kernels_slot_ll.hip) ----------------------------------------
// The mirror of bfmmm_get_chain: n_slots draws of `name`, in the layout that call returns for n_slots slots, into slots
// [first_slot, first_slot + n_slots) of the selected chain.  Nothing else is touched.
extern "C" int bfmmm_set_chain(bfmmm_handle* h, const char* name, int first_slot, int n_slots, const double* values, int64_t count) {
  const std::string fn = "bfmmm_set_chain";
  if (!h) return fail(fn + ": 'h' is null");
  if (!name) return fail(fn + ": 'name' is null");
  if (!values) return fail(fn + ": 'values' is null");
  const std::string s(name);
  const ChainArr a = chain_array(selc(h), h->T, s);
  if (!a.p) return fail(fn + ": unknown name '" + s + "'");
  if (first_slot < 0 || first_slot >= h->T) return fail(fn + "(" + s + "): 'first_slot' out of range");
  if (n_slots < 1 || n_slots > h->T - first_slot) return fail(fn + "(" + s + "): 'n_slots' out of range (first_slot + n_slots > T)");
  if (count != a.len * n_slots)
    return fail(fn + "(" + s + "): 'count' must be " + std::to_string(a.len * n_slots) + " (" + std::to_string(a.len) + " entries x " +
                std::to_string(n_slots) + " slots), got " + std::to_string(count));
  const bool by_slot = a.ps == 1;      // else slot fastest (tau): values[t + n_slots e]
  const bool positive = s == "sigma_sq";
  for (int64_t o = 0; o < count; ++o) {
    const bool finite = std::isfinite(values[o]);
    if (finite && !(positive && values[o] <= 0.0)) continue;
    const int64_t t = by_slot ? o / a.len : o % n_slots, e = by_slot ? o % a.len : o / n_slots;
    return fail(fn + "(" + s + "): value at slot " + std::to_string(first_slot + t) + ", entry " + std::to_string(e) +
                (finite ? " is not positive" : " is not finite"));
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));
  double* dst = const_cast<double*>(a.p);
  if (by_slot) HIPCHK(copy_sync(h, dst + (size_t)a.ss * first_slot, values, sizeof(double) * (size_t)count, hipMemcpyHostToDevice));
  else      // one run of n_slots slots per entry
    for (int64_t e = 0; e < a.len; ++e)
      HIPCHK(copy_sync(h, dst + (size_t)a.ps * e + (size_t)a.ss * first_slot, values + (size_t)n_slots * e, sizeof(double) * (size_t)n_slots,
                       hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

// loglik(q, t) of every chain and slot of the range from the records and the slots, in chunks of consecutive curves: k_slot_rss fills
// the chunk's rows, k_slot_ll_reduce adds them in curve order to the call's accumulator, and the last chunk's reduction applies
// k_loglik's closed form (and stores where asked).  curve: the rows as l_i, chunk by chunk.
extern "C" int bfmmm_chain_slot_loglik(bfmmm_handle* h, int first_slot, int n_slots, int store, int64_t max_workspace_bytes, double* loglik,
                                       double* curve, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_slot_loglik", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"loglik", loglik}}) || ck.range() || ck.budget_sign(max_workspace_bytes)) return 1;
  const int n = h->c.d.n;
  const size_t N = (size_t)ck.CS();
  if (ck.capacity(capacity, curve ? (int64_t)n * (int64_t)N : (int64_t)N)) return 1;
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), sizeof(double) * N, sizeof(double) * N, n, kNoCap, "curve", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_SLOT_LL, PT_SLOT_LL_REDUCE);
  CallBufs b;
  double *d_acc = nullptr, *d_part = nullptr;
  Timer kernel, reduce;
  HIPCHK(b.timers({&kernel, &reduce}));
  HIPCHK(b.get(&d_acc, N));
  HIPCHK(b.get(&d_part, (size_t)chunk * N));
  const int rc = for_chunks(ck, n, chunk, [&](int64_t i0, int rows) {
    std::string err = timed(kernel, h->st, [&] { return launch_slot_rss(h->c, first_slot, n_slots, (int)i0, rows, d_part, h->st); });
    if (err.empty())
      err = timed(reduce, h->st, [&] { return launch_slot_ll_reduce(h->c, first_slot, n_slots, (int)i0, rows, curve != nullptr, store != 0, d_part, d_acc, h->st); });
    if (err.empty()) err = Back{h, i0, rows}(curve, (const double*)d_part, N).done();
    if (err.empty() && hipGetLastError() != hipSuccess) err = "kernel failed";
    if (!err.empty()) return err;
    collect(h, kernel, PT_SLOT_LL);
    collect(h, reduce, PT_SLOT_LL_REDUCE);
    return err;
  });
  if (rc) return rc;
  HIPCHK(copy_sync(h, loglik, d_acc, sizeof(double) * N, hipMemcpyDeviceToHost));
  return 0;
}

// ---- pooled per-curve covariance surfaces from the chain slots (kernels_curve_cov.hip) ------------------------
// Mean, sd and per-chain means of C_i(g, h) = sum_m (E1_g . V_im)(E2_h . V_im) over the draws, in chunks of consecutive result
// rows; the projection tables are filled once per call and only the three results reach the host.
extern "C" int bfmmm_chain_curve_cov(bfmmm_handle* h, const double* E1, int G1, const double* E2, int G2, int diagonal,
                                     const int32_t* curves, int n_curves, int first_slot, int n_slots, int64_t max_workspace_bytes,
                                     double* mean, double* sd, double* chain_mean, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_cov", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"h", h}, {"E1", E1}, {"mean", mean}}) || ck.grid_pair(G1, E2, G2, diagonal)) return 1;
  const int C = h->nch, P = h->c.d.P;
  if (!E2) G2 = G1;
  int64_t m = 0, chunk = 0;
  if (n_curves < 0) return fail(fn + ": 'n_curves' must not be negative");
  if (ck.curve_list(curves, n_curves, &m)) return 1;
  const int64_t cells = diagonal ? (int64_t)G1 : (int64_t)G1 * G2;      // entries of a curve's result
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, m * cells) || ck.row_limit()) return 1;
  CovCall f;
  f.G1 = G1; f.G2 = G2; f.diagonal = diagonal ? 1 : 0; f.first_slot = first_slot; f.n_slots = n_slots;
  const std::string bad = cov_check(h->c, f);
  if (!bad.empty()) return fail(fn + ": " + bad);
  // shared by all curves: the tables, E1, E2 and the curve list; a curve: its entries of mean, of sd and of every chain's mean
  const size_t tab1 = cov_table_doubles(h->c, f, 0), tab2 = E2 ? cov_table_doubles(h->c, f, 1) : 0;
  const size_t shared = sizeof(double) * (tab1 + tab2 + (size_t)G1 * P + (E2 ? (size_t)G2 * P : 0)) +
                        (curves ? sizeof(int32_t) * (((size_t)m + 1) & ~(size_t)1) : 0);
  const size_t per_curve = sizeof(double) * (size_t)cells * (1 + (sd ? 1 : 0) + (chain_mean ? (size_t)C : 0));
  if (ck.units(budget_of(max_workspace_bytes), shared, per_curve, m, cells_cap(cells), "curve", &chunk)) return 1;
  reset_timers(h, PT_COV_PROJECT, PT_COV);
  if (m == 0) return 0;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  double *d_E1 = nullptr, *d_E2 = nullptr, *d_mean = nullptr, *d_sd = nullptr, *d_cm = nullptr;
  int32_t* d_curves = nullptr;
  Timer kernel;
  HIPCHK(b.timers({&kernel}));
  HIPCHK(b.put(h, &d_E1, E1, (size_t)G1 * P));
  HIPCHK(b.get(&f.tab1, tab1));
  if (E2) {
    HIPCHK(b.put(h, &d_E2, E2, (size_t)G2 * P));
    HIPCHK(b.get(&f.tab2, tab2));
  }
  if (curves) HIPCHK(b.put(h, &d_curves, curves, (size_t)m));
  HIPCHK(b.get(&d_mean, (size_t)chunk * cells));
  if (sd) HIPCHK(b.get(&d_sd, (size_t)chunk * cells));
  if (chain_mean) HIPCHK(b.get(&d_cm, (size_t)chunk * C * cells));
  f.E1 = d_E1; f.E2 = d_E2; f.curves = d_curves;
  if (once(ck, b, PT_COV_PROJECT, E2 ? 2 : 1, [&] { return launch_cov_project(h->c, f, h->st); })) return 1;
  return for_chunks(ck, m, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(kernel, h->st, [&] { return launch_curve_cov(h->c, f, (int)r0, rows, d_mean, d_sd, d_cm, h->st); });
    if (err.empty()) err = Back{h, r0, rows}(sd, d_sd, (size_t)cells)(chain_mean, d_cm, (size_t)C * cells)(mean, d_mean, (size_t)cells).done();
    if (err.empty()) collect(h, kernel, PT_COV);
    return err;
  });
}

// ---- prediction of held-out curves from the chain slots (kernels_predict.hip) -----------------------------------
// The records of all new curves once per call (launch_stats_* as they are; a from-basis handle forms them on the host as its
// creation does), then per chunk of consecutive new curves k_predict into the chunk's traces and k_predict_pool over them.
// bfmmm_chain_predict_fit (kernels_predict_fit.hip) is the same call with a FitAsk: every check under its own name,
// k_predict_fit in k_predict's place, and behind the pooling the moments of the fitted function and the quantiles of its paths.
namespace {
struct FitAsk {
  const double* E;
  int G, noise;
  const double* probs;
  int nq;
  double *fit_mean, *fit_sd, *fit_q, *mean_trace, *var_trace, *path_trace;
  int32_t* path_index;
  double *path_u, *path_xi;
};
// bfmmm_chain_predict_laplace (kernels_predict_laplace.hip): the same call with k_predict_lap in k_predict's place, one
// round and no sample table; what it returns besides (each may be null)
struct LapAsk {
  int32_t* n_modes;
  double *components, *eta_samples;
};

int predict_call(const char* name, const FitAsk* fit, const LapAsk* lap, bfmmm_handle* h, const double* y, const double* t, const double* B,
                 const int64_t* offsets, int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                 int n_stages, uint64_t seed, const double* zs, int64_t max_workspace_bytes, double* lpd, double* z_mean, double* z_sd,
                 double* ess_mean, double* ess_min, double* lpd_trace, double* z_trace, double* ess_trace, double* prop_trace,
                 double* samples, int64_t capacity) {
  const SlotCheck ck{name, h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"h", h}})) return 1;
  if (n_new < 0) return fail(fn + ": 'n_new' must not be negative");
  if (n_new == 0) return 0;
  if (ck.ptrs({{"lpd", lpd}, {"z_mean", z_mean}, {"z_sd", z_sd}, {"ess_mean", ess_mean}, {"ess_min", ess_min}})) return 1;
  const Ctx& c = h->c;
  const int G = fit ? fit->G : 0, nq = fit ? fit->nq : 0;
  if (fit) {
    if (ck.ptrs({{"E", fit->E}, {"fit_mean", fit->fit_mean}, {"fit_sd", fit->fit_sd}})) return 1;
    if (G < 1) return fail(fn + ": 'G' must be at least 1");
    for (int64_t e = 0; e < (int64_t)G * c.d.P; ++e)
      if (!std::isfinite(fit->E[e])) return fail(fn + ": 'E'[" + std::to_string(e / c.d.P) + ", " + std::to_string(e % c.d.P) + "] is not finite");
    if (nq > 0 && ck.ptrs({{"probs", fit->probs}, {"fit_q", fit->fit_q}})) return 1;
    if (ck.probs_list(fit->probs, nq, 0, fit->fit_q)) return 1;
  }
  const Dims& d = c.d;
  const int K = d.K, P = d.P, D = d.D, J = n_samples, R = n_stages;
  const bool mv = d.mv != 0, from_basis = !h->B_host.empty();
  if (ck.ptrs({{"y", y}})) return 1;
  if (mv) {
    if (t || B || offsets) return fail(fn + ": the multivariate model takes 'y' alone: 't', 'B' and 'offsets' must be null");
  } else if (from_basis) {
    if (ck.ptrs({{"B", B}, {"offsets", offsets}})) return 1;
    if (t) return fail(fn + ": a sampler created from a basis takes 'B', not 't'");
  } else {
    if (ck.ptrs({{"t", t}, {"offsets", offsets}})) return 1;
    if (B) return fail(fn + ": a spline sampler takes 't', not 'B'");
  }
  if (!mv) {
    if (offsets[0] < 0) return fail(fn + ": 'offsets'[0] must not be negative");
    for (int r = 0; r < n_new; ++r)
      if (offsets[r + 1] - offsets[r] < 1)
        return fail(fn + ": new curve " + std::to_string(r) + " is empty (offsets " + std::to_string(offsets[r]) + " .. " + std::to_string(offsets[r + 1]) +
                    "): at least 1 point a curve");
  }
  if (D > 0 && !X) return fail(fn + ": 'X' is null but the sampler has " + std::to_string(D) + " covariates");
  if (D == 0 && X) return fail(fn + ": 'X' is given but the sampler has no covariates");
  for (int64_t e = 0; X && e < (int64_t)n_new * D; ++e)
    if (!std::isfinite(X[e])) return fail(fn + ": 'X'[" + std::to_string(e % n_new) + ", " + std::to_string(e / n_new) + "] is not finite");
  if (J < 1) return fail(fn + ": 'n_samples' must be at least 1, got " + std::to_string(J));
  if (R < 1) return fail(fn + ": 'n_stages' must be at least 1, got " + std::to_string(R));
  if (zs && R != 1) return fail(fn + ": 'zs' takes the place of the stage-0 samples: 'n_stages' must be 1, got " + std::to_string(R));
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, n_new, "rows") || ck.row_limit()) return 1;
  // the RNG index ((r R + st) J + j) K + k is a 32-bit counter word
  if (!zs && !lap && (long double)n_new * (long double)R * (long double)J * (long double)K > 4294967296.0L)
    return fail(fn + ": n_new x n_stages x n_samples x K = " + std::to_string(n_new) + " x " + std::to_string(R) + " x " + std::to_string(J) + " x " +
                std::to_string(K) + " exceeds the 4294967296 (2^32) indices of the random number counter");
  // (the mixture proposal: index (r J + j)(K + 1) + i)
  if (lap && (long double)n_new * (long double)J * (long double)(K + 1) > 4294967296.0L)
    return fail(fn + ": n_new x n_samples x (K + 1) = " + std::to_string(n_new) + " x " + std::to_string(J) + " x " + std::to_string(K + 1) +
                " exceeds the 4294967296 (2^32) indices of the random number counter");
  if (perm && ck.perm_check(perm)) return 1;
  PredictCall f;
  f.n_new = n_new; f.J = J; f.R = R; f.first_slot = first_slot; f.n_slots = n_slots; f.seed = seed;
  PredictFitCall ff;
  if (fit) { ff.G = G; ff.noise = fit->noise; }
  ff.p = f;
  const std::string bad = fit ? predict_fit_check(c, ff, nullptr) : lap ? predict_lap_check(c, f, nullptr) : predict_check(c, f, nullptr);
  if (!bad.empty()) return fail(fn + ": " + bad);
  const size_t N = (size_t)ck.CS();
  const int Mn = d.M;
  // the fit of a curve: mu_t, v_t and the paths (3 G N), U and j* (N + N / 2), xi (N M), mean, sd and quantiles (G (2 + nq)) and,
  // for rows too long for the LDS sort, their workspace
  const SortWs sws((long long)N, fit && nq > 0);
  const size_t fit_curve = fit ? (size_t)G * (3 * N + 2 + (size_t)nq + sws.NP) + N + (N + 1) / 2 + N * (size_t)Mn : 0;
  const size_t fit_shared = fit ? sizeof(double) * ((size_t)G * P + 16) : 0;
  const int64_t n_obs = mv ? (int64_t)n_new * P : offsets[n_new];
  // shared by all curves: the data (y, and t and the offsets of a spline sampler), the records and counts, X, perm, zs; a curve: its
  // traces (lpd, ess, m, q, the proposals and the samples where asked for) and its five pooled results
  const size_t shared = sizeof(double) * ((from_basis ? 0 : (size_t)n_obs * (mv ? 1 : 2)) + (size_t)n_new * d.LREC + (X ? (size_t)n_new * D : 0) +
                                          (zs ? N * (size_t)J * K : 0) + 2) +
                        sizeof(int64_t) * (!mv && !from_basis ? (size_t)n_new + 1 : 0) + sizeof(int32_t) * (((size_t)n_new + 1) & ~(size_t)1) +
                        (perm ? sizeof(int32_t) * ((N * K + 1) & ~(size_t)1) : 0) + fit_shared;
  // the mixture proposal of a curve: n_modes (an int a draw, counted as a double), the components and the samples where asked for
  const size_t CD = (size_t)predict_lap_comp_doubles(K);
  const size_t lap_curve = lap ? N * (1 + (lap->components ? (size_t)(K + 2) * CD : 0) + (lap->eta_samples ? (size_t)J * (K - 1) : 0)) : 0;
  const size_t per_curve = sizeof(double) * (N * (2 + 2 * (size_t)K + (prop_trace ? (size_t)R * K : 0) + (samples ? (size_t)R * J * K : 0)) + 3 + 2 * (size_t)K +
                                             fit_curve + lap_curve);
  const size_t budget = budget_of(max_workspace_bytes);
  if (samples && budget < shared + per_curve)
    return fail(fn + ": 'samples' of one curve (n_chains x n_slots x n_stages x n_samples x K doubles) with the rest need " +
                std::to_string(shared + per_curve) + " bytes, above 'max_workspace_bytes' = " + std::to_string(budget) + " " +
                SlotCheck::plan_text(shared, per_curve, "curve"));
  int64_t chunk = 0;
  const int64_t cells = (int64_t)std::max<size_t>(1, per_curve / sizeof(double) / std::max<size_t>(N, 1));
  if (ck.units(budget, shared, per_curve, n_new, cells_cap(cells), "curve", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  const int pt = fit ? PT_PREDICT_FIT : lap ? PT_PREDICT_LAPLACE : PT_PREDICT;
  reset_timers(h, PT_PREDICT_STATS, PT_PREDICT_STATS);
  reset_timers(h, pt, pt);
  CallBufs b;
  double *d_y = nullptr, *d_t = nullptr, *d_rec = nullptr, *d_X = nullptr, *d_zs = nullptr, *d_tr = nullptr, *d_prop = nullptr, *d_smp = nullptr,
         *d_out = nullptr;
  int64_t* d_off = nullptr;
  int *d_ni = nullptr, *d_err = nullptr;
  int32_t* d_perm = nullptr;
  Timer stats, kernel, pool, fpool, quant;
  HIPCHK(b.timers({&stats, &kernel, &pool, &fpool, &quant}));
  HIPCHK(b.get(&d_rec, (size_t)n_new * d.LREC));
  HIPCHK(b.get(&d_ni, (size_t)n_new));
  if (from_basis) {
    // band-packed G = B'B ([dd P + lo] = G(lo, lo + dd), dd <= BW), s = B'y, yy, as bfmmm_create_from_basis forms them
    std::vector<double> hrec((size_t)n_new * d.LREC, 0.0);
    std::vector<int> hni((size_t)n_new);
    for (int r = 0; r < n_new; ++r) {
      double* rc = hrec.data() + (size_t)r * d.LREC;
      hni[r] = (int)(offsets[r + 1] - offsets[r]);
      for (int64_t l = offsets[r]; l < offsets[r + 1]; ++l) {
        const double* br = B + (size_t)l * P;
        for (int lo = 0; lo < P; ++lo) {
          if (br[lo] == 0.0) continue;
          for (int dd = 0; dd <= d.BW && lo + dd < P; ++dd) rc[dd * P + lo] += br[lo] * br[lo + dd];
          rc[d.LG + lo] += br[lo] * y[l];
        }
        rc[d.LG + P] += y[l] * y[l];
      }
    }
    HIPCHK(copy_sync(h, d_rec, hrec.data(), sizeof(double) * hrec.size(), hipMemcpyHostToDevice));
    HIPCHK(copy_sync(h, d_ni, hni.data(), sizeof(int) * hni.size(), hipMemcpyHostToDevice));
  } else {
    HIPCHK(b.put(h, &d_y, y, (size_t)n_obs));
    if (!mv) {
      HIPCHK(b.put(h, &d_t, t, (size_t)n_obs));
      HIPCHK(b.put(h, &d_off, offsets, (size_t)n_new + 1));
      HIPCHK(b.get(&d_err, 2));
      HIPCHK(hipMemsetAsync(d_err, 0, sizeof(int) * 2, h->st));
    }
    HIPCHK(hipMemsetAsync(d_rec, 0, sizeof(double) * (size_t)n_new * d.LREC, h->st));
    int herr = 0;
    const std::string serr = timed(stats, h->st, [&] {
      if (mv) { launch_stats_multivariate(n_new, P, d.LREC, d_y, d_rec, d_ni, h->st); return std::string(); }
      return launch_stats_functional(h->cfg.basis_degree, n_new, P, d.LREC, d_off, d_t, d_y, h->d_knots, h->n_knots, d_rec, d_ni, nullptr, d_err, h->st)
                 ? std::string("unsupported basis_degree") : std::string();
    });
    if (!serr.empty()) { (void)hipStreamSynchronize(h->st); return fail(fn + ": " + serr); }
    if (!mv) HIPCHK(copy_sync(h, &herr, d_err, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(hipGetLastError());
    collect(h, stats, PT_PREDICT_STATS);
    if (herr) return fail(fn + ": at least one time point of the new curves lies outside 'boundary_knots'");
  }
  if (X) HIPCHK(b.put(h, &d_X, X, (size_t)n_new * D));
  if (perm) HIPCHK(b.put(h, &d_perm, perm, N * K));
  if (zs) HIPCHK(b.put(h, &d_zs, zs, N * (size_t)J * K));
  const size_t NK = N * (size_t)K;
  HIPCHK(b.get(&d_tr, (size_t)chunk * (2 * N + 2 * NK)));
  HIPCHK(b.get(&d_out, (size_t)chunk * (3 + 2 * (size_t)K)));
  if (prop_trace) HIPCHK(b.get(&d_prop, (size_t)chunk * NK * R));
  if (samples) HIPCHK(b.get(&d_smp, (size_t)chunk * NK * R * J));
  f.rec = d_rec; f.ni = d_ni; f.X = d_X; f.perm = d_perm; f.zs = d_zs;
  int32_t* d_nm = nullptr;
  double *d_comp = nullptr, *d_eta = nullptr;
  if (lap) {
    HIPCHK(b.get(&d_nm, (size_t)chunk * N));
    if (lap->components) HIPCHK(b.get(&d_comp, (size_t)chunk * N * (K + 2) * CD));
    if (lap->eta_samples) HIPCHK(b.get(&d_eta, (size_t)chunk * N * J * (K - 1)));
  }
  double* d_lpd_t = d_tr;
  double* d_ess_t = d_lpd_t + (size_t)chunk * N;
  double* d_m_t = d_ess_t + (size_t)chunk * N;
  double* d_q_t = d_m_t + (size_t)chunk * NK;
  double* d_lpd = d_out;
  double* d_emean = d_lpd + chunk;
  double* d_emin = d_emean + chunk;
  double* d_zm = d_emin + chunk;
  double* d_zsd = d_zm + (size_t)chunk * K;
  // the fit's buffers of a chunk: mu_t, v_t, paths; U, xi; mean, sd, quantiles, sort workspace; j*
  double *d_E = nullptr, *d_probs = nullptr, *d_fit = nullptr, *d_fres = nullptr;
  int32_t* d_pidx = nullptr;
  const size_t GN = (size_t)G * N;
  if (fit) {
    HIPCHK(b.put(h, &d_E, fit->E, (size_t)G * P));
    HIPCHK(probs_put(b, h, fit->probs, nq, &d_probs));
    HIPCHK(b.get(&d_fit, (size_t)chunk * (3 * GN + N + N * (size_t)Mn)));
    HIPCHK(b.get(&d_fres, (size_t)chunk * G * (2 + (size_t)nq + sws.NP)));
    HIPCHK(b.get(&d_pidx, (size_t)chunk * N));
    ff.p = f; ff.E = d_E;
  }
  double *d_mu_t = nullptr, *d_var_t = nullptr, *d_path_t = nullptr, *d_pu = nullptr, *d_pxi = nullptr, *d_fmean = nullptr, *d_fsd = nullptr,
         *d_fq = nullptr, *d_fw = nullptr;
  if (fit) {
    d_mu_t = d_fit;
    d_var_t = d_mu_t + (size_t)chunk * GN;
    d_path_t = d_var_t + (size_t)chunk * GN;
    d_pu = d_path_t + (size_t)chunk * GN;
    d_pxi = d_pu + (size_t)chunk * N;
    d_fmean = d_fres;
    d_fsd = d_fmean + (size_t)chunk * G;
    d_fq = d_fsd + (size_t)chunk * G;
    d_fw = d_fq + (size_t)chunk * G * nq;
  }
  return for_chunks(ck, n_new, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(kernel, h->st, [&] {
      return fit ? launch_predict_fit(c, ff, (int)r0, rows, d_lpd_t, d_ess_t, d_m_t, d_q_t, d_prop, d_smp, d_mu_t, d_var_t, d_path_t, d_pidx, d_pu,
                                      d_pxi, h->st)
             : lap ? launch_predict_lap(c, f, (int)r0, rows, d_lpd_t, d_ess_t, d_m_t, d_q_t, d_nm, d_comp, d_eta, h->st)
                   : launch_predict(c, f, (int)r0, rows, d_lpd_t, d_ess_t, d_m_t, d_q_t, d_prop, d_smp, h->st);
    });
    if (err.empty() && fit) {
      // (the pooled rows of the chunk are consecutive from 0 in every buffer: launch_predict_fit wrote rows of G N)
      err = timed(fpool, h->st, [&] { return launch_predict_fit_pool((long long)N, (long long)rows * G, d_mu_t, d_var_t, d_fmean, d_fsd, h->st); });
      if (err.empty() && nq)
        err = timed(quant, h->st, [&] { return launch_bands_quantiles(d_path_t, (int)N, (long long)rows * G, d_fw, d_probs, nq, d_fq, h->st); });
      if (err.empty())
        err = Back{h, r0, rows, true}(fit->mean_trace, d_mu_t, GN)(fit->var_trace, d_var_t, GN)(fit->path_trace, d_path_t, GN)(
                  fit->path_u, d_pu, N)(fit->path_xi, d_pxi, N * (size_t)Mn)(fit->fit_mean, d_fmean, (size_t)G)(fit->fit_sd, d_fsd, (size_t)G)(
                  nq ? fit->fit_q : nullptr, d_fq, (size_t)G * nq).queued();
      if (err.empty() && fit->path_index &&
          hipMemcpyAsync(fit->path_index + (size_t)r0 * N, d_pidx, sizeof(int32_t) * (size_t)rows * N, hipMemcpyDeviceToHost, h->st) != hipSuccess)
        err = kBackFailed;
    }
    if (err.empty())
      err = timed(pool, h->st, [&] { return launch_predict_pool(K, (long long)N, rows, d_lpd_t, d_ess_t, d_m_t, d_q_t, d_lpd, d_zm, d_zsd, d_emean, d_emin, h->st); });
    if (err.empty() && lap)
      err = Back{h, r0, rows}(lap->n_modes, (const int32_t*)d_nm, N)(lap->components, (const double*)d_comp, N * (K + 2) * CD)(
                lap->eta_samples, (const double*)d_eta, N * (size_t)J * (K - 1)).queued();
    if (err.empty())
      err = Back{h, r0, rows}(lpd_trace, d_lpd_t, N)(ess_trace, d_ess_t, N)(z_trace, d_m_t, NK)(prop_trace, d_prop, NK * R)(samples, d_smp, NK * R * J)(
                lpd, d_lpd, 1)(ess_mean, d_emean, 1)(ess_min, d_emin, 1)(z_mean, d_zm, K)(z_sd, d_zsd, K).done();
    if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
    if (!err.empty()) return err;
    collect(h, kernel, pt);
    collect(h, pool, pt);
    if (fit) collect(h, fpool, pt);
    if (fit && nq) collect(h, quant, pt);
    return err;
  });
}
}  // namespace

extern "C" int bfmmm_chain_predict(bfmmm_handle* h, const double* y, const double* t, const double* B, const int64_t* offsets,
                                   int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                                   int n_stages, uint64_t seed, const double* zs, int64_t max_workspace_bytes,
                                   double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min,
                                   double* lpd_trace, double* z_trace, double* ess_trace, double* prop_trace, double* samples,
                                   int64_t capacity) {
  return predict_call("bfmmm_chain_predict", nullptr, nullptr, h, y, t, B, offsets, n_new, X, perm, first_slot, n_slots, n_samples, n_stages, seed, zs,
                      max_workspace_bytes, lpd, z_mean, z_sd, ess_mean, ess_min, lpd_trace, z_trace, ess_trace, prop_trace, samples, capacity);
}

extern "C" int bfmmm_chain_predict_fit(bfmmm_handle* h, const double* y, const double* t, const double* B, const int64_t* offsets,
                                       int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                                       int n_stages, uint64_t seed, const double* zs, const double* E, int G, int noise,
                                       const double* probs, int nq, int64_t max_workspace_bytes,
                                       double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min,
                                       double* fit_mean, double* fit_sd, double* fit_q,
                                       double* lpd_trace, double* z_trace, double* ess_trace, double* prop_trace, double* samples,
                                       double* mean_trace, double* var_trace, double* path_trace, int32_t* path_index, double* path_u,
                                       double* path_xi, int64_t capacity) {
  const FitAsk fit{E, G, noise ? 1 : 0, probs, nq, fit_mean, fit_sd, fit_q, mean_trace, var_trace, path_trace, path_index, path_u, path_xi};
  return predict_call("bfmmm_chain_predict_fit", &fit, nullptr, h, y, t, B, offsets, n_new, X, perm, first_slot, n_slots, n_samples, n_stages, seed, zs,
                      max_workspace_bytes, lpd, z_mean, z_sd, ess_mean, ess_min, lpd_trace, z_trace, ess_trace, prop_trace, samples, capacity);
}

extern "C" int bfmmm_chain_predict_laplace(bfmmm_handle* h, const double* y, const double* t, const double* B, const int64_t* offsets,
                                           int n_new, const double* X, const int32_t* perm, int first_slot, int n_slots, int n_samples,
                                           uint64_t seed, int64_t max_workspace_bytes,
                                           double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min,
                                           double* lpd_trace, double* z_trace, double* ess_trace,
                                           int32_t* n_modes, double* components, double* eta_samples, int64_t capacity) {
  const LapAsk lap{n_modes, components, eta_samples};
  return predict_call("bfmmm_chain_predict_laplace", nullptr, &lap, h, y, t, B, offsets, n_new, X, perm, first_slot, n_slots, n_samples, 1, seed,
                      nullptr, max_workspace_bytes, lpd, z_mean, z_sd, ess_mean, ess_min, lpd_trace, z_trace, ess_trace, nullptr, nullptr, capacity);
}

