// C ABI of the sampler (include/bfmmm.h), what is read off the chain slots after a run: the chain arrays, their convergence
// diagnostics, the per-curve log-density with its diagnostics, the pooled per-curve fitted functions and bands,
// their simultaneous bands, the pooled co-membership matrix of the curves and the least-squares draw against it, the pooled
// per-curve covariance surfaces, the label alignment against a pivot, the pooled cluster summaries under it, the cluster
// covariance surfaces with their bands and their eigenvalues and eigenfunctions, the reference's rescale step per draw with the
// summaries, mean functions and covariance surfaces under it, the contrasts of cluster mean functions and covariate effects
// under either labelling and the prediction of held-out curves with
// their fitted functions; and what is written into the slots from outside (bfmmm_set_chain) with the log-likelihood of such slots.
// The PSIS-LOO family over the chain slots is capi_loo.hip's.
// What an entry point is made of is capi_chain.hpp's (SlotCheck, CallBufs, for_chunks, `once`, Back), shared with that file.  What
// several of the entry points here do is written once as well: SortWs for the rule that long rows sort in a workspace, and
// RowReducer for a chunk of rows of C S pooled values: its layout in one allocation, its reduction (moments or the seven
// statistics, then the quantiles) and its copies back.
#include "capi_chain.hpp"

namespace {

// ---- the chain arrays ---------------------------------------------------------------------------------------------------
// Element e of slot t of array `name` is p[t ss + e ps] in the chain of context c, and q * c.chain_bytes (cov: chain_bytes_cov)
// bytes further in the q-th chain after it.  p null: no array of that name (covariate arrays exist once covariates were set).
struct ChainArr { const char* nm; const double* p; int64_t len; bool cov; int64_t ss, ps; };
ChainArr chain_array(const Ctx& c, int T, const std::string& name) {
  const Dims& d = c.d;
  const int64_t n = d.n, K = d.K, P = d.P, M = d.M, D = d.D;
  const ChainArr arrs[] = {{"nu", c.c_nu, K * P}, {"chi", c.c_chi, n * M}, {"Z", c.c_Z, n * K}, {"pi", c.c_pi, K},
                           {"alpha_3", c.c_alpha3, 1}, {"delta", c.c_delta, K * M}, {"A", c.c_A, K * 2},
                           {"sigma_sq", c.c_sigma, 1}, {"gamma", c.c_gamma, K * P * M}, {"Phi", c.c_Phi, K * P * M},
                           {"loglik", c.c_loglik, 1},
                           {"eta", c.c_eta, P * D * K, true}, {"xi", c.c_xi, K * P * D * M, true}, {"tau_eta", c.c_tau_eta, K * D, true},
                           {"gamma_xi", c.c_gamma_xi, K * P * D * M, true}, {"delta_xi", c.c_delta_xi, K * M * D, true},
                           {"A_xi", c.c_A_xi, K * 2 * D, true},
                           {"tau", c.c_tau, K, false, 1, T}};      // tau: T_alloc x K column-major (slot fastest)
  for (ChainArr a : arrs)
    if (name == a.nm && a.p) {
      if (!a.ps) { a.ss = a.len; a.ps = 1; }      // the others: slot by slot
      return a;
    }
  return {};
}

// 16 doubles on the device (owned by b) with the call's nq probabilities in front, and `extra` more behind them
hipError_t probs_put(CallBufs& b, bfmmm_handle* h, const double* probs, int nq, double** d_probs, int extra = 0) {
  const hipError_t e = b.get(d_probs, 16 + (size_t)extra);
  return e != hipSuccess || !nq ? e : copy_sync(h, *d_probs, probs, sizeof(double) * (size_t)nq, hipMemcpyHostToDevice);
}

// ---- rows of N = C S pooled values (kernels_bands.hip, kernels_diag.hip) ---------------------------------------------------------
// Where quantiles are wanted, rows of up to fit_lds_rows() draws sort in LDS and longer ones in a workspace of NP doubles a row
// (k_bands_quantiles_big); `also`: the caller sorts such rows by a threshold of its own.
struct SortWs {
  bool on;
  size_t NP;
  SortWs(long long N, bool wanted, bool also = false)
      : on((wanted && N > fit_lds_rows()) || also), NP(on ? (size_t)bands_sort_pad((int)N) : 0) {}
};

// A chunk of rows of N values in one allocation, their reduction and the copies back.  Two flavours: mean and sd
// (launch_bands_moments; a row takes N + 2 + nq + NP doubles) or the seven statistics (diag_launch; N + tier + 7 + nq + NP), then
// the nq quantiles (launch_bands_quantiles) where nq > 0.  The sub-buffers hold `chunk` rows each, in the order of the members.
struct RowReducer {
  bfmmm_handle* h;
  int C, S, nq;
  bool seven;
  size_t N, tier;
  SortWs ws;
  const double* probs = nullptr;      // the nq probabilities on the device
  double *x = nullptr, *mean = nullptr, *sd = nullptr, *out7 = nullptr, *tws = nullptr, *q = nullptr, *w = nullptr;
  std::vector<double> hb;             // the seven statistics of a chunk, statistic by statistic

  RowReducer(const SlotCheck& ck, int nq, bool seven, bool also_sort = false)
      : h(ck.h), C(ck.h->nch), S(ck.n_slots), nq(nq), seven(seven), N((size_t)ck.CS()), tier(seven ? diag_row_ws_doubles(C, S) : 0),
        ws(ck.CS(), nq > 0, also_sort) {}
  size_t res_doubles() const { return (seven ? tier + 7 : 2) + (size_t)nq + ws.NP; }      // of a row, without its values
  size_t row_bytes() const { return sizeof(double) * (N + res_doubles()); }
  // the sub-buffers of `chunk` rows: the values at vals, the rest from res on
  void place(double* vals, double* res, int64_t chunk) {
    const size_t n = (size_t)chunk;
    x = vals;
    if (seven) { out7 = res; tws = out7 + 7 * n; q = tws + tier * n; }
    else { mean = res; sd = mean + n; q = sd + n; }
    w = q + (size_t)nq * n;
  }
  hipError_t alloc(CallBufs& b, int64_t chunk) {
    double* p = nullptr;
    const hipError_t e = b.get(&p, row_bytes() / sizeof(double) * (size_t)chunk);
    if (e == hipSuccess) place(p, p + (size_t)chunk * N, chunk);
    return e;
  }
  std::string reduce(long long rows) const {
    std::string err = seven ? diag_launch(x, rows, C, S, out7, rows, tws, rows, h->st) : launch_bands_moments(x, (int)N, rows, mean, sd, h->st);
    if (err.empty() && nq) err = launch_bands_quantiles(x, (int)N, rows, w, probs, nq, q, h->st);
    return err;
  }
  // rows [r0, r0 + rows) of the results to the host: quant and trace where asked for, then outs: mean and sd, or the seven statistics
  std::string to_host(int64_t r0, int rows, double* const* outs, double* quant, double* trace) {
    Back back{h, r0, rows};
    back(nq ? quant : nullptr, q, (size_t)nq)(trace, x, N);
    if (!seven) return back(outs[0], mean, 1)(outs[1], sd, 1).done();
    hb.resize(7 * (size_t)rows);
    const std::string err = Back{h, 0, 1, back.ok}(hb.data(), out7, 7 * (size_t)rows).done();
    for (int s = 0; err.empty() && s < 7; ++s) std::copy(hb.begin() + (size_t)s * rows, hb.begin() + (size_t)(s + 1) * rows, outs[s] + r0);
    return err;
  }
};

// ---- split R-hat, ESS, MCSE, mean and sd of rows of C S draws (kernels_diag.hip) --------------------------------
// fill(p0, rows, d_x) puts rows [p0, p0 + rows) of the len rows into the workspace (row-major: draw fastest, then chain),
// where diag_launch reduces them; nothing goes to the host but the seven statistics.  ll_timed: fill is curve_ll_timed.
template <typename Fill>
int seven_stats(const SlotCheck& ck, int64_t len, int64_t max_workspace_bytes, double* const (&outs)[7], bool ll_timed, Fill fill) {
  bfmmm_handle* h = ck.h;
  RowReducer r(ck, 0, true);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, r.row_bytes(), len, kNoCap, nullptr, &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  if (ll_timed) reset_timers(h, PT_CURVE_LL, PT_CURVE_LL);
  CallBufs b;
  HIPCHK(r.alloc(b, chunk));
  return for_chunks(ck, len, chunk, [&](int64_t p0, int rows) {
    std::string err = fill((int)p0, rows, r.x);
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = r.to_host(p0, rows, outs, nullptr, nullptr);
    if (err.empty() && ll_timed) curve_ll_collect(h);
    return err;
  });
}

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
// consecutive elements into the workspace of seven_stats.
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
  return seven_stats(ck, a.len, max_workspace_bytes, outs, false, [&](int p0, int rows, double* d_x) {
    return diag_gather(a.p, a.cov ? c.chain_bytes_cov : c.chain_bytes, a.ss, a.ps, first_slot, n_slots, h->nch, p0, rows, d_x, h->st);
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
// into the workspace of seven_stats; the matrix never leaves the device.
extern "C" int bfmmm_chain_curve_diagnostics(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes,
                                             double* rhat, double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean,
                                             double* mean, double* sd, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_curve_diagnostics", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"rhat", rhat}, {"ess_bulk", ess_bulk}, {"ess_tail", ess_tail}, {"ess_mean", ess_mean}, {"mcse_mean", mcse_mean},
               {"mean", mean}, {"sd", sd}}) ||
      ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, h->c.d.n) || ck.row_limit())
    return 1;
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  return seven_stats(ck, h->c.d.n, max_workspace_bytes, outs, true, [&](int p0, int rows, double* d_x) { return curve_ll_timed(ck, p0, rows, d_x); });
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

// ---- label alignment against a pivot and the pooled cluster summaries (kernels_align.hip) ----------------------
namespace {

// (inner, outer) of the component axis of a chain array: element e = a + inner (k + K b), a < inner, b < outer; inner 0: no
// component axis.  False: no array of that name.
bool align_axis(const Dims& d, const std::string& name, int64_t* inner) {
  const int64_t n = d.n, P = d.P, M = d.M, D = d.D;
  const struct { const char* nm; int64_t inner; } axes[] = {
      {"nu", 1}, {"Phi", 1}, {"gamma", 1}, {"Z", n}, {"pi", 1}, {"tau", 1}, {"delta", 1}, {"A", 1}, {"eta", P * D}, {"xi", P * D * M},
      {"gamma_xi", P * D * M}, {"tau_eta", 1}, {"delta_xi", 1}, {"A_xi", 1}, {"chi", 0}, {"sigma_sq", 0}, {"alpha_3", 0}, {"loglik", 0}};
  for (const auto& a : axes)
    if (name == a.nm) { *inner = a.inner; return true; }
  return false;
}

// every row perm[(q S + s) K + .] a permutation of 0 .. K - 1, or fail() naming the first draw that is not
int perm_check(const SlotCheck& ck, const int32_t* perm) {
  const int K = ck.h->c.d.K, S = ck.n_slots;
  for (long long o = 0; o < ck.CS(); ++o) {
    unsigned seen = 0;
    for (int l = 0; l < K; ++l) {
      const int32_t v = perm[o * K + l];
      if (v < 0 || v >= K || (seen >> v & 1u))
        return fail(ck.fn + ": 'perm' of chain " + std::to_string(o / S) + ", slot " + std::to_string(ck.first_slot + o % S) +
                    " is not a permutation of 0 .. " + std::to_string(K - 1));
      seen |= 1u << v;
    }
  }
  return 0;
}


}  // namespace

// perm and score of every draw against the pivot Zref: one launch of k_align_gram, one workgroup per draw.
extern "C" int bfmmm_chain_align(bfmmm_handle* h, const double* Zref, int first_slot, int n_slots, int32_t* perm, double* score,
                                 int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_align", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"Zref", Zref}, {"perm", perm}}) || ck.range() || ck.row_limit()) return 1;
  const Dims& d = h->c.d;
  const int64_t N = ck.CS();
  if (ck.capacity(capacity, N * d.K)) return 1;
  for (int64_t e = 0; e < (int64_t)d.n * d.K; ++e)
    if (!std::isfinite(Zref[e]))
      return fail(ck.fn + ": 'Zref'[" + std::to_string(e % d.n) + ", " + std::to_string(e / d.n) + "] is not finite");
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_ALIGN_GRAM, PT_ALIGN_GRAM);
  CallBufs b;
  double *d_ref = nullptr, *d_score = nullptr;
  int32_t* d_perm = nullptr;
  Timer gram;
  HIPCHK(b.timers({&gram}));
  HIPCHK(b.put(h, &d_ref, Zref, (size_t)d.n * d.K));
  HIPCHK(b.get(&d_perm, (size_t)N * d.K));
  HIPCHK(b.get(&d_score, (size_t)N));
  return for_chunks(ck, 1, 1, [&](int64_t, int) {
    std::string err = timed(gram, h->st, [&] { return launch_align_gram(h->c, d_ref, first_slot, n_slots, d_perm, d_score, h->st); });
    if (err.empty()) err = Back{h, 0, 1}(score, d_score, (size_t)N)(perm, d_perm, (size_t)N * d.K).done();
    if (err.empty()) collect(h, gram, PT_ALIGN_GRAM);
    return err;
  });
}

// bfmmm_chain_diagnostics of `name` with every draw's components relabelled by its row of perm, and the quantiles of the same
// gathered rows: k_align_gather, then diag_launch and launch_bands_quantiles as they are, in chunks of consecutive elements.
extern "C" int bfmmm_chain_aligned_summary(bfmmm_handle* h, const char* name, const int32_t* perm, int first_slot, int n_slots,
                                           const double* probs, int nq, int64_t max_workspace_bytes, double* rhat, double* ess_bulk,
                                           double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd, double* quant,
                                           int64_t capacity) {
  SlotCheck ck{"bfmmm_chain_aligned_summary", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"name", name}, {"perm", perm}, {"rhat", rhat}, {"ess_bulk", ess_bulk}, {"ess_tail", ess_tail},
               {"ess_mean", ess_mean}, {"mcse_mean", mcse_mean}, {"mean", mean}, {"sd", sd}}) ||
      ck.range() || ck.budget_sign(max_workspace_bytes))
    return 1;
  const Ctx& c = h->c;          // chain 0 of the batch
  const ChainArr a = chain_array(c, h->T, name);
  int64_t inner = 0;
  if (!a.p || !align_axis(c.d, name, &inner)) return fail(ck.fn + ": unknown name '" + name + "'");
  ck.tag = std::string("(") + name + ")";
  if (ck.capacity(capacity, a.len) || ck.row_limit() || ck.probs_list(probs, nq, 0, quant) || perm_check(ck, perm)) return 1;
  const int C = h->nch, S = n_slots, K = c.d.K;
  RowReducer r(ck, nq, true);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, r.row_bytes(), a.len, kNoCap, nullptr, &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_ALIGN_GATHER, PT_ALIGN_GATHER);
  CallBufs b;
  double* d_probs = nullptr;
  int32_t* d_perm = nullptr;
  Timer gather;
  HIPCHK(b.timers({&gather}));
  HIPCHK(r.alloc(b, chunk));
  HIPCHK(b.put(h, &d_perm, perm, r.N * K));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs));
  r.probs = d_probs;
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  return for_chunks(ck, a.len, chunk, [&](int64_t p0, int rows) {
    std::string err = timed(gather, h->st, [&] {
      return launch_align_gather(a.p, a.cov ? c.chain_bytes_cov : c.chain_bytes, a.ss, a.ps, first_slot, S, C, (int)p0, rows, d_perm, K, inner,
                                 r.x, h->st);
    });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = r.to_host(p0, rows, outs, quant, nullptr);
    if (err.empty()) collect(h, gather, PT_ALIGN_GATHER);
    return err;
  });
}

// Mean, sd and quantiles over the pooled draws of the K G cluster mean functions E nu_k with the labels aligned: k_align_project
// into rows of C S values, then launch_bands_moments and launch_bands_quantiles as they are, in chunks of consecutive rows.
extern "C" int bfmmm_chain_cluster_mean_bands(bfmmm_handle* h, const int32_t* perm, const double* E, int G, int first_slot, int n_slots,
                                              const double* probs, int nq, int64_t max_workspace_bytes, double* mean, double* sd,
                                              double* quant, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_cluster_mean_bands", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"perm", perm}, {"E", E}, {"mean", mean}, {"sd", sd}})) return 1;
  if (G < 1) return fail(ck.fn + ": 'G' must be at least 1");
  if (ck.range() || ck.budget_sign(max_workspace_bytes)) return 1;
  const Ctx& c = h->c;
  const int K = c.d.K, P = c.d.P;
  const int64_t len = (int64_t)K * G;
  if (ck.capacity(capacity, len, "rows") || ck.row_limit() || ck.probs_list(probs, nq, 0, quant) || perm_check(ck, perm)) return 1;
  RowReducer r(ck, nq, false);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, r.row_bytes(), len, 65535, nullptr, &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_ALIGN_PROJECT, PT_ALIGN_PROJECT);
  CallBufs b;
  double *d_E = nullptr, *d_probs = nullptr;
  int32_t* d_perm = nullptr;
  Timer project;
  HIPCHK(b.timers({&project}));
  HIPCHK(r.alloc(b, chunk));
  HIPCHK(b.put(h, &d_E, E, (size_t)G * P));
  HIPCHK(b.put(h, &d_perm, perm, r.N * K));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs));
  r.probs = d_probs;
  double* const outs[2] = {mean, sd};
  return for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(project, h->st, [&] { return launch_align_project(c, d_E, G, d_perm, first_slot, n_slots, (int)r0, rows, r.x, h->st); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = r.to_host(r0, rows, outs, quant, nullptr);
    if (err.empty()) collect(h, project, PT_ALIGN_PROJECT);
    return err;
  });
}

// ---- cluster covariance surfaces with bands under aligned labels (kernels_cluster_cov.hip) ----------------------
// Mean, sd and quantiles over the pooled draws of c_r(g, h) = sum_m W1_k[g][m] W2_l[h][m] of the aligned pairs r = (k, l), and the
// simultaneous band per pair: k_ccov_project once per call, then per chunk of consecutive result rows k_ccov_values into rows of
// C S values and launch_bands_moments and launch_bands_quantiles on them as they are.  The band's deviations need every chunk's
// mean and sd: with one chunk its values are reused, with several a second sweep forms them again for k_ccov_maxdev.
// The body of bfmmm_chain_cluster_cov_bands and bfmmm_chain_cluster_cov_bands_rescaled: the labels of a draw are its row of perm, or
// (mix set) its K x K transform mix[(cs K + k) K + c], under which the tables are filled raw and mixed in a second pass.
static int ccov_call(const char* name, bfmmm_handle* h, const int32_t* perm, const double* mix, const double* E1, int G1, const double* E2,
                     int G2, int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot, int n_slots,
                     const double* probs, int nq, double alpha, int64_t max_workspace_bytes, double* mean, double* sd, double* quant,
                     double* crit, double* lower, double* upper, double* trace, int64_t capacity, bool rescaled) {
  const SlotCheck ck{name, h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"h", h}, {rescaled ? "mix" : "perm", rescaled ? (const void*)mix : (const void*)perm}, {"E1", E1}, {"mean", mean}, {"sd", sd}}) ||
      ck.grid_pair(G1, E2, G2, diagonal))
    return 1;
  if (n_pairs < 0) return fail(fn + ": 'n_pairs' must not be negative");
  const Ctx& c = h->c;
  const int K = c.d.K, P = c.d.P, D = c.d.D;
  for (int r = 0; pairs && r < n_pairs; ++r)
    if (pairs[2 * r] < 0 || pairs[2 * r] >= K || pairs[2 * r + 1] < 0 || pairs[2 * r + 1] >= K)
      return fail(fn + ": 'pairs'[" + std::to_string(r) + "] = (" + std::to_string(pairs[2 * r]) + ", " + std::to_string(pairs[2 * r + 1]) +
                  ") outside 0 .. " + std::to_string(K - 1));
  if (ck.covariate_setting(x)) return 1;
  if (c.d.M < 1) return fail(fn + ": n_eigen is 0: the model has no covariance surface");
  if (!E2) G2 = G1;
  // the pairs of the result: the caller's, or all k <= l
  std::vector<int32_t> pr;
  if (pairs) pr.assign(pairs, pairs + 2 * (size_t)n_pairs);
  else
    for (int k = 0; k < K; ++k)
      for (int l = k; l < K; ++l) { pr.push_back(k); pr.push_back(l); }
  const int64_t m = (int64_t)pr.size() / 2;
  const int64_t cells = diagonal ? (int64_t)G1 : (int64_t)G1 * G2;      // entries of a pair's result
  const int64_t len = m * cells;
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, len) || ck.row_limit() || ck.probs_list(probs, nq, 0, quant))
    return 1;
  const bool band = crit || lower || upper;
  if (band && !(crit && lower && upper)) return fail(fn + ": 'crit', 'lower' and 'upper' must be all null or all set");
  if ((band && ck.alpha_inside(alpha)) || (!rescaled && perm_check(ck, perm))) return 1;
  CcovCall f;
  f.G1 = G1; f.G2 = G2; f.diagonal = diagonal ? 1 : 0; f.first_slot = first_slot; f.n_slots = n_slots; f.n_pairs = m;
  const std::string bad = ccov_check(c, f);
  if (!bad.empty()) return fail(fn + ": " + bad);
  reset_timers(h, PT_CCOV_PROJECT, PT_CCOV_MAXDEV);
  if (m == 0) return 0;
  const size_t N = (size_t)ck.CS();
  const bool long_dev = band && (long long)N > ccov_sort_rows();               // dev's rows are sorted in the workspace too
  RowReducer r(ck, nq, false, long_dev);
  // shared by all rows: the tables, E1, E2, x, probs, perm, the pairs and, for the band, dev and crit; a row: its values, its sort
  // workspace, its mean, sd and quantiles
  const size_t tab1 = ccov_table_doubles(c, f, 0), tab2 = E2 ? ccov_table_doubles(c, f, 1) : 0;
  const size_t shared = sizeof(double) * (tab1 + tab2 + (size_t)G1 * P + (E2 ? (size_t)G2 * P : 0) + (x ? (size_t)D : 0) + 17 +
                                          (band ? (size_t)m * N + (size_t)m : 0)) +
                        (rescaled ? sizeof(double) * N * K * K : sizeof(int32_t) * ((N * K + 1) & ~(size_t)1)) + sizeof(int32_t) * 2 * (size_t)m;
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), shared, r.row_bytes(), len, 1 << 30, "row", &chunk)) return 1;
  const int64_t nchunks = (len + chunk - 1) / chunk;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  double *d_E1 = nullptr, *d_E2 = nullptr, *d_x = nullptr, *d_probs = nullptr, *d_dev = nullptr, *d_crit = nullptr, *d_mix = nullptr;
  int32_t *d_perm = nullptr, *d_pairs = nullptr;
  Timer values, maxdev;
  HIPCHK(b.timers({&values, &maxdev}));
  HIPCHK(r.alloc(b, chunk));
  HIPCHK(b.put(h, &d_E1, E1, (size_t)G1 * P));
  HIPCHK(b.get(&f.tab1, tab1));
  if (E2) {
    HIPCHK(b.put(h, &d_E2, E2, (size_t)G2 * P));
    HIPCHK(b.get(&f.tab2, tab2));
  }
  if (x) HIPCHK(b.put(h, &d_x, x, (size_t)D));
  if (rescaled) HIPCHK(b.put(h, &d_mix, mix, N * K * K));
  else HIPCHK(b.put(h, &d_perm, perm, N * K));
  HIPCHK(b.put(h, &d_pairs, (const int32_t*)pr.data(), pr.size()));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs, 1));      // [16]: 1 - alpha
  r.probs = d_probs;
  const double p_crit = 1.0 - alpha;
  if (band) {
    HIPCHK(copy_sync(h, d_probs + 16, &p_crit, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(b.get(&d_dev, (size_t)m * N));
    HIPCHK(b.get(&d_crit, (size_t)m));
    HIPCHK(hipMemsetAsync(d_dev, 0, sizeof(double) * (size_t)m * N, h->st));      // the maximum starts from 0.0
  }
  f.E1 = d_E1; f.E2 = d_E2; f.x = d_x; f.perm = d_perm; f.mix = d_mix; f.pairs = d_pairs;
  if (once(ck, b, PT_CCOV_PROJECT, E2 ? 2 : 1, [&] { return launch_ccov_project(c, f, h->st); })) return 1;
  double* const outs[2] = {mean, sd};
  auto dev_launch = [&](int64_t r0, int rows) {
    return timed(maxdev, h->st, [&] { return launch_ccov_maxdev(f, (long long)N, r0, rows, r.x, r.mean, r.sd, d_dev, h->st); });
  };
  int rc = for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    const bool dev_now = band && nchunks == 1;
    std::string err = timed(values, h->st, [&] { return launch_ccov_values(c, f, r0, rows, r.x, h->st); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty() && dev_now) err = dev_launch(r0, rows);
    if (err.empty()) err = r.to_host(r0, rows, outs, quant, trace);
    if (!err.empty()) return err;
    collect(h, values, PT_CCOV);
    if (dev_now) collect(h, maxdev, PT_CCOV_MAXDEV);
    return err;
  });
  if (rc || !band) return rc;
  if (nchunks > 1) {
    // the second sweep: the same kernel on the same tables gives the same values, now against every chunk's mean and sd
    rc = for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
      std::string err = timed(values, h->st, [&] { return launch_ccov_values(c, f, r0, rows, r.x, h->st); });
      if (err.empty() && (copy_sync(h, r.mean, mean + r0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess ||
                          copy_sync(h, r.sd, sd + r0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess))
        err = "copy of the chunk's mean and sd failed";
      if (err.empty()) err = dev_launch(r0, rows);
      if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = "kernel failed";
      if (!err.empty()) return err;
      collect(h, values, PT_CCOV);
      collect(h, maxdev, PT_CCOV_MAXDEV);
      return err;
    });
    if (rc) return rc;
  }
  // crit[r]: the (1 - alpha) quantile of dev's row r, interpolated without an fma as k_fit_sim's is; long rows are sorted by
  // k_bands_quantiles_big, in pieces of as many rows as the chunk's sort workspace holds, and the rule read off them again
  rc = for_chunks(ck, m, long_dev ? std::min<int64_t>(m, chunk) : m, [&](int64_t p0, int cnt) {
    std::string err;
    if (!long_dev) err = launch_ccov_crit(d_dev + (size_t)p0 * N, (long long)N, cnt, p_crit, d_crit + p0, h->st);
    else {
      err = launch_bands_quantiles(d_dev + (size_t)p0 * N, (int)N, cnt, r.w, d_probs + 16, 1, d_crit + p0, h->st);
      if (err.empty()) err = launch_fit_quantiles(r.w, (int)r.ws.NP, (int)N, cnt, d_probs + 16, 1, d_crit + p0, h->st);
    }
    return err.empty() ? Back{h, p0, cnt}(crit, d_crit + p0, 1).done() : err;
  });
  if (rc) return rc;
  {
#pragma clang fp contract(off)
    for (int64_t e = 0; e < len; ++e) {
      const double w = crit[e / cells] * sd[e];
      lower[e] = mean[e] - w;
      upper[e] = mean[e] + w;
    }
  }
  return 0;
}

extern "C" int bfmmm_chain_cluster_cov_bands(bfmmm_handle* h, const int32_t* perm, const double* E1, int G1, const double* E2, int G2,
                                             int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot, int n_slots,
                                             const double* probs, int nq, double alpha, int64_t max_workspace_bytes, double* mean, double* sd,
                                             double* quant, double* crit, double* lower, double* upper, double* trace, int64_t capacity) {
  return ccov_call("bfmmm_chain_cluster_cov_bands", h, perm, nullptr, E1, G1, E2, G2, diagonal, pairs, n_pairs, x, first_slot, n_slots, probs, nq,
                   alpha, max_workspace_bytes, mean, sd, quant, crit, lower, upper, trace, capacity, false);
}

// bfmmm_chain_cluster_cov_bands with the transform of every draw in place of its permutation: W~_k = sum_c A[k][c] W_c (k_ccov_mix)
extern "C" int bfmmm_chain_cluster_cov_bands_rescaled(bfmmm_handle* h, const double* mix, const double* E1, int G1, const double* E2, int G2,
                                                      int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot,
                                                      int n_slots, const double* probs, int nq, double alpha, int64_t max_workspace_bytes,
                                                      double* mean, double* sd, double* quant, double* crit, double* lower, double* upper,
                                                      double* trace, int64_t capacity) {
  return ccov_call("bfmmm_chain_cluster_cov_bands_rescaled", h, nullptr, mix, E1, G1, E2, G2, diagonal, pairs, n_pairs, x, first_slot, n_slots,
                   probs, nq, alpha, max_workspace_bytes, mean, sd, quant, crit, lower, upper, trace, capacity, true);
}

// ---- the reference's rescale step per draw (kernels_rescale.hip) ----------------------------------------------------
// A, A^-1, the pure curves, rcond and z_min of every draw: one launch of k_rescale_transform, one workgroup per draw.  transform
// null: the rule under perm (null: the identity); else A is the caller's and perm is not read.
extern "C" int bfmmm_chain_rescale(bfmmm_handle* h, const int32_t* perm, const double* transform, int first_slot, int n_slots, double* mix,
                                   double* mix_inv, int32_t* curve, double* rcond, double* z_min, int64_t* n_singular, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_rescale", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"mix", mix}, {"mix_inv", mix_inv}, {"curve", curve}, {"rcond", rcond}, {"z_min", z_min}}) || ck.range() ||
      ck.row_limit())
    return 1;
  const int K = h->c.d.K;
  const size_t N = (size_t)ck.CS(), KK = (size_t)K * K;
  if (ck.capacity(capacity, (int64_t)(N * KK)) || (!transform && perm && perm_check(ck, perm))) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_RESCALE_TRANSFORM, PT_RESCALE_TRANSFORM);
  CallBufs b;
  double *d_given = nullptr, *d_mix = nullptr, *d_inv = nullptr, *d_rc = nullptr, *d_zm = nullptr;
  int32_t *d_perm = nullptr, *d_curve = nullptr, *d_flag = nullptr;
  std::vector<int32_t> flag(N);
  Timer tr;
  HIPCHK(b.timers({&tr}));
  if (transform) HIPCHK(b.put(h, &d_given, transform, N * KK));
  else if (perm) HIPCHK(b.put(h, &d_perm, perm, N * K));
  HIPCHK(b.get(&d_mix, N * KK));
  HIPCHK(b.get(&d_inv, N * KK));
  HIPCHK(b.get(&d_curve, N * K));
  HIPCHK(b.get(&d_rc, N));
  HIPCHK(b.get(&d_zm, N));
  HIPCHK(b.get(&d_flag, N));
  const int rc = for_chunks(ck, 1, 1, [&](int64_t, int) {
    std::string err = timed(tr, h->st, [&] {
      return launch_rescale_transform(h->c, d_perm, d_given, first_slot, n_slots, d_mix, d_inv, d_curve, d_rc, d_zm, d_flag, h->st);
    });
    if (err.empty()) err = Back{h, 0, 1}(mix, d_mix, N * KK)(mix_inv, d_inv, N * KK)(curve, d_curve, N * K)(rcond, d_rc, N)(z_min, d_zm, N)(flag.data(), d_flag, N).done();
    if (err.empty()) collect(h, tr, PT_RESCALE_TRANSFORM);
    return err;
  });
  if (rc) return rc;
  int64_t cnt = 0;
  for (size_t o = 0; o < N; ++o) cnt += flag[o] ? 1 : 0;      // the kernel's own flag: rcond of a finite inverse can underflow to 0
  if (n_singular) *n_singular = cnt;
  return 0;
}

// bfmmm_chain_aligned_summary under the transform of every draw: k_rescale_gather, then the unchanged RowReducer.  The reference
// rescales nu, Phi, eta and xi by A and Z by A^-1, and nothing else.
extern "C" int bfmmm_chain_rescaled_summary(bfmmm_handle* h, const char* name, const double* mix, const double* mix_inv, int first_slot,
                                            int n_slots, const double* probs, int nq, int64_t max_workspace_bytes, double* rhat,
                                            double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd,
                                            double* quant, int64_t capacity) {
  SlotCheck ck{"bfmmm_chain_rescaled_summary", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"name", name}, {"mix", mix}, {"mix_inv", mix_inv}, {"rhat", rhat}, {"ess_bulk", ess_bulk}, {"ess_tail", ess_tail},
               {"ess_mean", ess_mean}, {"mcse_mean", mcse_mean}, {"mean", mean}, {"sd", sd}}) ||
      ck.range() || ck.budget_sign(max_workspace_bytes))
    return 1;
  const Ctx& c = h->c;
  const std::string nm = name;
  const bool by_inverse = nm == "Z";
  if (!by_inverse && nm != "nu" && nm != "Phi" && nm != "eta" && nm != "xi")
    return fail(ck.fn + ": the reference defines no rescale for '" + nm + "' (only for nu, Phi, eta, xi and Z)");
  const ChainArr a = chain_array(c, h->T, nm);
  int64_t inner = 0;
  if (!a.p || !align_axis(c.d, nm, &inner) || inner < 1) return fail(ck.fn + ": no array '" + nm + "' (covariate arrays exist once covariates were set)");
  ck.tag = "(" + nm + ")";
  if (ck.capacity(capacity, a.len) || ck.row_limit() || ck.probs_list(probs, nq, 0, quant)) return 1;
  const int C = h->nch, S = n_slots, K = c.d.K;
  RowReducer r(ck, nq, true);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, r.row_bytes(), a.len, kNoCap, nullptr, &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_RESCALE_GATHER, PT_RESCALE_GATHER);
  CallBufs b;
  double *d_probs = nullptr, *d_w = nullptr;
  Timer gather;
  HIPCHK(b.timers({&gather}));
  HIPCHK(r.alloc(b, chunk));
  HIPCHK(b.put(h, &d_w, by_inverse ? mix_inv : mix, r.N * K * K));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs));
  r.probs = d_probs;
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  return for_chunks(ck, a.len, chunk, [&](int64_t p0, int rows) {
    std::string err = timed(gather, h->st, [&] {
      return launch_rescale_gather(a.p, a.cov ? c.chain_bytes_cov : c.chain_bytes, a.ss, a.ps, first_slot, S, C, (int)p0, rows, d_w,
                                   by_inverse ? 1 : K, by_inverse ? K : 1, K, inner, r.x, h->st);
    });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = r.to_host(p0, rows, outs, quant, nullptr);
    if (err.empty()) collect(h, gather, PT_RESCALE_GATHER);
    return err;
  });
}

// bfmmm_chain_cluster_mean_bands under the transform of every draw, at the covariate setting x (D entries; null: nu alone):
// k_rescale_project into rows of C S values, then the unchanged RowReducer.
extern "C" int bfmmm_chain_cluster_mean_bands_rescaled(bfmmm_handle* h, const double* mix, const double* E, int G, const double* x,
                                                       int first_slot, int n_slots, const double* probs, int nq, int64_t max_workspace_bytes,
                                                       double* mean, double* sd, double* quant, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_cluster_mean_bands_rescaled", h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"mix", mix}, {"E", E}, {"mean", mean}, {"sd", sd}})) return 1;
  if (G < 1) return fail(ck.fn + ": 'G' must be at least 1");
  if (ck.range() || ck.budget_sign(max_workspace_bytes)) return 1;
  const Ctx& c = h->c;
  const int K = c.d.K, P = c.d.P, D = c.d.D;
  if (x && !(D > 0 && c.c_eta)) return fail(ck.fn + ": 'x' is given but the sampler has no covariates");
  if (x && D > 8) return fail(ck.fn + ": more than 8 covariates");
  for (int d = 0; x && d < D; ++d)
    if (!std::isfinite(x[d])) return fail(ck.fn + ": 'x'[" + std::to_string(d) + "] is not finite");
  const int64_t len = (int64_t)K * G;
  if (ck.capacity(capacity, len, "rows") || ck.row_limit() || ck.probs_list(probs, nq, 0, quant)) return 1;
  RowReducer r(ck, nq, false);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, r.row_bytes(), len, 65535, nullptr, &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_RESCALE_PROJECT, PT_RESCALE_PROJECT);
  CallBufs b;
  double *d_E = nullptr, *d_probs = nullptr, *d_mix = nullptr, *d_x = nullptr;
  Timer project;
  HIPCHK(b.timers({&project}));
  HIPCHK(r.alloc(b, chunk));
  HIPCHK(b.put(h, &d_E, E, (size_t)G * P));
  HIPCHK(b.put(h, &d_mix, mix, r.N * K * K));
  if (x) HIPCHK(b.put(h, &d_x, x, (size_t)D));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs));
  r.probs = d_probs;
  double* const outs[2] = {mean, sd};
  return for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(project, h->st, [&] { return launch_rescale_project(c, d_E, G, d_mix, d_x, first_slot, n_slots, (int)r0, rows, r.x, h->st); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = r.to_host(r0, rows, outs, quant, nullptr);
    if (err.empty()) collect(h, project, PT_RESCALE_PROJECT);
    return err;
  });
}

// ---- contrasts of cluster mean functions and covariate effects (kernels_cluster_contrast.hip) ---------------------
// k_contrast_coef once per call, then per chunk of consecutive result rows e = r G + g: k_contrast_values into rows of C S values,
// the unchanged RowReducer, k_rows_count for prob_positive and k_contrast_norm into the R norm rows, which the second RowReducer (the
// seven statistics and the quantiles) reduces once the last chunk is done.  The band is bfmmm_chain_cluster_cov_bands' with `diagonal`:
// launch_ccov_maxdev, the second sweep where a call takes several chunks, launch_ccov_crit or the long-row sort; then k_rows_count on
// dev against t_r for p_sim.
extern "C" int bfmmm_chain_cluster_contrast_bands(bfmmm_handle* h, const double* mix, const double* E, int G, const double* w_nu,
                                                  const double* w_eta, int R, const double* weights, int first_slot, int n_slots,
                                                  const double* probs, int nq, double alpha, int64_t max_workspace_bytes, double* mean,
                                                  double* sd, double* quant, int32_t* n_positive, double* crit, double* lower, double* upper,
                                                  int32_t* n_exceed, double* norm_stats, double* norm_quant, double* trace, double* norm_trace,
                                                  int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_cluster_contrast_bands", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"h", h}, {"mix", mix}, {"E", E}, {"w_nu", w_nu}, {"mean", mean}, {"sd", sd}, {"n_positive", n_positive}, {"norm_stats", norm_stats}}))
    return 1;
  if (G < 1) return fail(fn + ": 'G' must be at least 1");
  if (R < 1 || R > 64) return fail(fn + ": 'R' = " + std::to_string(R) + " outside 1 .. 64");
  const Ctx& c = h->c;
  const int K = c.d.K, P = c.d.P, D = c.d.D;
  if (w_eta && !(D > 0 && c.c_eta)) return fail(fn + ": 'w_eta' is given but the sampler has no covariates");
  if (w_eta && D > 8) return fail(fn + ": more than 8 covariates");
  const int KD = w_eta ? K * D : 0;
  for (int r = 0; r < R; ++r) {
    bool any = false;
    for (int k = 0; k < K; ++k) {
      if (!std::isfinite(w_nu[r * K + k])) return fail(fn + ": 'w_nu'[" + std::to_string(r) + ", " + std::to_string(k) + "] is not finite");
      any = any || w_nu[r * K + k] != 0.0;
    }
    for (int e = 0; e < KD; ++e) {
      if (!std::isfinite(w_eta[(size_t)r * KD + e]))
        return fail(fn + ": 'w_eta'[" + std::to_string(r) + ", " + std::to_string(e / D) + ", " + std::to_string(e % D) + "] is not finite");
      any = any || w_eta[(size_t)r * KD + e] != 0.0;
    }
    if (!any) return fail(fn + ": contrast " + std::to_string(r) + " has no weight other than zero");
  }
  for (int g = 0; weights && g < G; ++g)
    if (!(weights[g] >= 0.0) || !std::isfinite(weights[g])) return fail(fn + ": 'weights'[" + std::to_string(g) + "] is negative or not finite");
  const bool band = crit || lower || upper || n_exceed;
  if (band && !(crit && lower && upper && n_exceed)) return fail(fn + ": 'crit', 'lower', 'upper' and 'n_exceed' must be all null or all set");
  const int64_t len = (int64_t)R * G;
  if ((band && ck.alpha_inside(alpha)) || ck.capacity(capacity, len, "rows") || ck.range() || ck.budget_sign(max_workspace_bytes) || ck.row_limit() ||
      ck.probs_list(probs, nq, 0, quant) || (nq > 0 && ck.ptrs({{"norm_quant", norm_quant}})))
    return 1;
  ContrastCall f;
  f.G = G; f.R = R; f.first_slot = first_slot; f.n_slots = n_slots;
  const size_t N = (size_t)ck.CS();
  const bool long_dev = band && (long long)N > ccov_sort_rows();               // dev's rows are sorted in the workspace too
  RowReducer r(ck, nq, false, long_dev), nr(ck, nq, true);
  // shared by all rows: the coefficient table, E, the label maps, the weights, probs, the R norm rows with their statistics, the
  // counts of p_sim and, for the band, dev, crit and t; a row: its values, its sort workspace, its mean, sd, quantiles and count
  const size_t shared = sizeof(double) * ((size_t)R * P * N + (size_t)G * P + N * K * K + (size_t)R * (K + KD) + (size_t)G + 17 +
                                          (band ? (size_t)R * N + 2 * (size_t)R : 0)) +
                        nr.row_bytes() * (size_t)R + sizeof(int32_t) * (((size_t)R + 1) & ~(size_t)1);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), shared, r.row_bytes() + sizeof(double), len, 65535, "row", &chunk)) return 1;
  const int64_t nchunks = (len + chunk - 1) / chunk;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_CONTRAST_COEF, PT_CONTRAST_NORM);
  CallBufs b;
  double *d_E = nullptr, *d_mix = nullptr, *d_wn = nullptr, *d_we = nullptr, *d_w = nullptr, *d_probs = nullptr, *d_dev = nullptr,
         *d_crit = nullptr, *d_thr = nullptr;
  int32_t *d_cnt = nullptr, *d_cntR = nullptr;
  Timer values, norm;
  HIPCHK(b.timers({&values, &norm}));
  HIPCHK(r.alloc(b, chunk));
  HIPCHK(nr.alloc(b, R));
  HIPCHK(b.get(&d_cnt, (size_t)chunk * 2));
  HIPCHK(b.get(&d_cntR, ((size_t)R + 1) & ~(size_t)1));
  HIPCHK(b.put(h, &d_E, E, (size_t)G * P));
  HIPCHK(b.put(h, &d_mix, mix, N * K * K));
  HIPCHK(b.put(h, &d_wn, w_nu, (size_t)R * K));
  if (w_eta) HIPCHK(b.put(h, &d_we, w_eta, (size_t)R * KD));
  const std::vector<double> even(weights ? 0 : (size_t)G, 1.0 / G);      // the default quadrature: the mean square over the grid
  HIPCHK(b.put(h, &d_w, weights ? weights : even.data(), (size_t)G));
  HIPCHK(b.get(&f.tab, (size_t)R * P * N));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs, 1));      // [16]: 1 - alpha
  r.probs = nr.probs = d_probs;
  HIPCHK(hipMemsetAsync(nr.x, 0, sizeof(double) * (size_t)R * N, h->st));         // the sums start from 0.0
  const double p_crit = 1.0 - alpha;
  if (band) {
    HIPCHK(copy_sync(h, d_probs + 16, &p_crit, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(b.get(&d_dev, (size_t)R * N));
    HIPCHK(b.get(&d_crit, (size_t)R));
    HIPCHK(b.get(&d_thr, (size_t)R));
    HIPCHK(hipMemsetAsync(d_dev, 0, sizeof(double) * (size_t)R * N, h->st));      // the maximum starts from 0.0
  }
  f.E = d_E; f.mix = d_mix; f.w_nu = d_wn; f.w_eta = d_we; f.w = d_w;
  if (once(ck, b, PT_CONTRAST_COEF, 0, [&] { return launch_contrast_coef(c, f, h->st); })) return 1;
  CcovCall mf;                                          // what launch_ccov_maxdev reads: R "pairs" of G diagonal entries
  mf.G1 = G; mf.G2 = G; mf.diagonal = 1; mf.n_pairs = R;
  double* const outs[2] = {mean, sd};
  auto dev_launch = [&](int64_t r0, int rows) { return launch_ccov_maxdev(mf, (long long)N, r0, rows, r.x, r.mean, r.sd, d_dev, h->st); };
  int rc = for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(values, h->st, [&] { return launch_contrast_values(c, f, r0, rows, r.x, h->st); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = launch_rows_count(r.x, (long long)N, rows, nullptr, 0, d_cnt, h->st);
    if (err.empty()) err = timed(norm, h->st, [&] { return launch_contrast_norm(c, f, r0, rows, r.x, nr.x, h->st); });
    if (err.empty() && band && nchunks == 1) err = dev_launch(r0, rows);
    if (err.empty()) err = Back{h, r0, rows}(n_positive, (const int32_t*)d_cnt, 1).queued();
    if (err.empty()) err = r.to_host(r0, rows, outs, quant, trace);
    if (!err.empty()) return err;
    collect(h, values, PT_CONTRAST_VALUES);
    collect(h, norm, PT_CONTRAST_NORM);
    return err;
  });
  if (rc) return rc;
  // the size of every contrast per draw: the seven statistics and the pooled quantiles of the R rows
  rc = for_chunks(ck, 1, 1, [&](int64_t, int) {
    std::string err = nr.reduce(R);
    double* outs7[7];
    for (int s = 0; s < 7; ++s) outs7[s] = norm_stats + (size_t)s * R;
    if (err.empty()) err = nr.to_host(0, R, outs7, norm_quant, norm_trace);
    return err;
  });
  if (rc || !band) return rc;
  if (nchunks > 1) {
    // the second sweep: the same kernel on the same table gives the same values, now against every chunk's mean and sd
    rc = for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
      std::string err = timed(values, h->st, [&] { return launch_contrast_values(c, f, r0, rows, r.x, h->st); });
      if (err.empty() && (copy_sync(h, r.mean, mean + r0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess ||
                          copy_sync(h, r.sd, sd + r0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess))
        err = "copy of the chunk's mean and sd failed";
      if (err.empty()) err = dev_launch(r0, rows);
      if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = "kernel failed";
      if (err.empty()) collect(h, values, PT_CONTRAST_VALUES);
      return err;
    });
    if (rc) return rc;
  }
  // crit[r] as bfmmm_chain_cluster_cov_bands reads it off dev
  rc = for_chunks(ck, R, long_dev ? std::min<int64_t>(R, chunk) : R, [&](int64_t p0, int cnt) {
    std::string err;
    if (!long_dev) err = launch_ccov_crit(d_dev + (size_t)p0 * N, (long long)N, cnt, p_crit, d_crit + p0, h->st);
    else {
      err = launch_bands_quantiles(d_dev + (size_t)p0 * N, (int)N, cnt, r.w, d_probs + 16, 1, d_crit + p0, h->st);
      if (err.empty()) err = launch_fit_quantiles(r.w, (int)r.ws.NP, (int)N, cnt, d_probs + 16, 1, d_crit + p0, h->st);
    }
    return err.empty() ? Back{h, p0, cnt}(crit, (const double*)(d_crit + p0), 1).done() : err;
  });
  if (rc) return rc;
  std::vector<double> thr((size_t)R, 0.0);
  {
#pragma clang fp contract(off)
    for (int64_t e = 0; e < len; ++e) {
      const double w = crit[e / G] * sd[e];
      lower[e] = mean[e] - w;
      upper[e] = mean[e] + w;
      // t_r: the largest |mean| / sd over the grid points with sd > 0; the band at level p excludes zero somewhere where crit_p < t_r
      if (sd[e] > 0.0) thr[(size_t)(e / G)] = std::max(thr[(size_t)(e / G)], std::fabs(mean[e]) / sd[e]);
    }
  }
  HIPCHK(copy_sync(h, d_thr, thr.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice));
  return for_chunks(ck, 1, 1, [&](int64_t, int) {
    const std::string err = launch_rows_count(d_dev, (long long)N, R, d_thr, 1, d_cntR, h->st);
    return err.empty() ? Back{h, 0, R}(n_exceed, (const int32_t*)d_cntR, 1).done() : err;
  });
}

// ---- cluster eigenvalues and eigenfunctions under aligned labels (kernels_cluster_eig.hip) --------------------
// k_ceig_gram and k_ceig_solve once per call: every draw's lambda, pve and total as rows of C S values, its signed b and its status
// word.  The K M + K M + K small rows are reduced at once by launch_bands_moments and launch_bands_quantiles, the lambda rows also
// by diag_launch, all as they are; then per chunk of consecutive eigenfunction rows k_ceig_values and the same two launchers.
extern "C" void bfmmm_set_cluster_eig_form(int form) { bfmmm::g_cluster_eig_form = form == 1 || form == 2 ? form : 0; }

extern "C" int bfmmm_chain_cluster_eigen(bfmmm_handle* h, const int32_t* perm, const double* E, int G, const double* w, const double* x,
                                         int n_functions, const double* ref, int first_slot, int n_slots, const double* probs, int nq,
                                         int64_t max_workspace_bytes, double* val_diag, double* val_quant, double* pve_mean, double* pve_sd,
                                         double* pve_quant, double* tot_mean, double* tot_sd, double* tot_quant, double* fn_mean,
                                         double* fn_sd, double* fn_quant, double* val_trace, double* fn_trace, int32_t* max_sweeps,
                                         int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_cluster_eigen", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  if (ck.ptrs({{"h", h}, {"perm", perm}, {"E", E}, {"val_diag", val_diag}, {"pve_mean", pve_mean}, {"pve_sd", pve_sd},
               {"tot_mean", tot_mean}, {"tot_sd", tot_sd}, {"max_sweeps", max_sweeps}}))
    return 1;
  if (G < 1) return fail(fn + ": 'G' must be at least 1");
  const Ctx& c = h->c;
  const int K = c.d.K, P = c.d.P, M = c.d.M, D = c.d.D, J = n_functions;
  if (M < 1) return fail(fn + ": n_eigen is 0: the model has no covariance surface");
  if (J < 0 || J > M) return fail(fn + ": 'n_functions' = " + std::to_string(J) + " outside 0 .. " + std::to_string(M) + " (n_eigen)");
  for (int g = 0; w && g < G; ++g)
    if (!(w[g] >= 0.0) || !std::isfinite(w[g])) return fail(fn + ": 'w'[" + std::to_string(g) + "] is negative or not finite");
  if (ck.covariate_setting(x)) return 1;
  const int64_t len = (int64_t)K * J * G;      // eigenfunction rows
  if (J > 0 && ck.ptrs({{"fn_mean", fn_mean}, {"fn_sd", fn_sd}})) return 1;
  for (int64_t e = 0; ref && e < len; ++e)
    if (!std::isfinite(ref[e])) return fail(fn + ": 'ref'[" + std::to_string(e) + "] is not finite");
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, len, "rows") || ck.row_limit() ||
      ck.probs_list(probs, nq, 0, val_quant))
    return 1;
  if (nq > 0 && (ck.ptrs({{"pve_quant", pve_quant}, {"tot_quant", tot_quant}}) || (J > 0 && ck.ptrs({{"fn_quant", fn_quant}})))) return 1;
  if (perm_check(ck, perm)) return 1;
  CeigCall f;
  f.G = G; f.J = J; f.first_slot = first_slot; f.n_slots = n_slots;
  const std::string bad = ceig_check(c, f);
  if (!bad.empty()) return fail(fn + ": " + bad);
  reset_timers(h, PT_CEIG_GRAM, PT_CEIG_VALUES);
  const int S = n_slots;
  const size_t N = (size_t)ck.CS();
  const size_t KM = (size_t)K * M, rs = 2 * KM + (size_t)K;                    // the small rows: lambda, pve, total
  const bool with_ref = ref && J > 0;
  // the eigenfunction rows in chunks; all rs small rows at once: their mean, sd and quantiles (sm) and the seven statistics of
  // the KM lambda rows in front (sv), on the values the solve leaves in d_small
  RowReducer r(ck, nq, false), sm(ck, nq, false), sv(ck, 0, true);
  // shared by all rows: Q, R, E, w, x, ref, probs, the small rows with their results and workspaces, the b of every draw, the
  // status words and perm; an eigenfunction row: its values, its sort workspace, its mean, sd and quantiles
  const size_t small_ws = rs * sm.res_doubles() + KM * sv.res_doubles();
  const size_t shared = sizeof(double) * ((size_t)P * P + (with_ref ? (size_t)K * J * P + (size_t)len : 0) + (size_t)G * P + (w ? (size_t)G : 0) +
                                          (x ? (size_t)D : 0) + 16 + N * rs + small_ws + N * K * J * P) +
                        sizeof(int32_t) * 2 * N * K;
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), shared, len > 0 ? r.row_bytes() : 0, len, 1 << 30, "row", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  double *d_E = nullptr, *d_w = nullptr, *d_x = nullptr, *d_ref = nullptr, *d_probs = nullptr, *d_small = nullptr, *d_sres = nullptr;
  int32_t *d_perm = nullptr, *d_status = nullptr;
  Timer gram, solve, values;
  HIPCHK(b.timers({&gram, &solve, &values}));
  HIPCHK(b.put(h, &d_E, E, (size_t)G * P));
  if (w) HIPCHK(b.put(h, &d_w, w, (size_t)G));
  if (x) HIPCHK(b.put(h, &d_x, x, (size_t)D));
  if (with_ref) {
    HIPCHK(b.put(h, &d_ref, ref, (size_t)len));
    HIPCHK(b.get(&f.R, (size_t)K * J * P));
  }
  HIPCHK(b.put(h, &d_perm, perm, N * K));
  HIPCHK(b.get(&d_status, N * K));
  HIPCHK(probs_put(b, h, probs, nq, &d_probs));
  r.probs = sm.probs = d_probs;
  HIPCHK(b.get(&f.Q, (size_t)P * P));
  HIPCHK(b.get(&d_small, N * rs));
  HIPCHK(b.get(&d_sres, small_ws));
  HIPCHK(b.get(&f.b, N * K * J * P));
  if (len > 0) HIPCHK(r.alloc(b, chunk));
  f.E = d_E; f.w = d_w; f.x = d_x; f.ref = d_ref; f.perm = d_perm; f.status = d_status;
  f.lam = d_small; f.pve = d_small + N * KM; f.tot = d_small + 2 * N * KM;
  sm.place(d_small, d_sres, (int64_t)rs);
  sv.place(d_small, d_sres + rs * sm.res_doubles(), (int64_t)KM);
  std::vector<int32_t> st_host(N * K);
  std::vector<double> smh(2 * rs);      // mean and sd of the small rows
  // the solve and the small rows
  int rc = for_chunks(ck, 1, 1, [&](int64_t, int) {
    std::string err = timed(gram, h->st, [&] { return launch_ceig_gram(c, f, h->st); });
    if (err.empty()) err = timed(solve, h->st, [&] { return launch_ceig_solve(c, f, h->st); });
    if (err.empty()) err = Back{h, 0, 1}(st_host.data(), d_status, N * K).done();
    if (!err.empty()) return err;
    collect(h, gram, PT_CEIG_GRAM);
    collect(h, solve, PT_CEIG);
    int32_t mx = 0;
    for (size_t o = 0; o < N * K; ++o) {
      if (st_host[o] & 0x100)
        return "no convergence in " + std::to_string(ceig_sweep_cap()) + " sweeps: chain " + std::to_string(o / K / S) + ", slot " +
               std::to_string(first_slot + (int)(o / K % S)) + ", component " + std::to_string(o % K);
      mx = std::max(mx, st_host[o] & 0xff);
    }
    *max_sweeps = mx;
    err = sm.reduce((long long)rs);
    if (err.empty()) err = sv.reduce((long long)KM);
    // the results lie statistic by statistic over all rs rows: lambda's KM rows, pve's KM, total's K.  Mean and sd of lambda are
    // among the seven statistics.
    const size_t q1 = KM * (size_t)nq;
    double* const nul = nullptr;
    if (err.empty())
      err = Back{h, 0, 1}(nq ? val_quant : nul, sm.q, q1)(nq ? pve_quant : nul, sm.q + q1, q1)(nq ? tot_quant : nul, sm.q + 2 * q1, (size_t)K * nq)(
                val_trace, d_small, N * KM)(val_diag, sv.out7, 7 * KM)(smh.data(), sm.mean, 2 * rs).done();
    if (!err.empty()) return err;
    std::copy(smh.begin() + KM, smh.begin() + 2 * KM, pve_mean);
    std::copy(smh.begin() + 2 * KM, smh.begin() + rs, tot_mean);
    std::copy(smh.begin() + rs + KM, smh.begin() + rs + 2 * KM, pve_sd);
    std::copy(smh.begin() + rs + 2 * KM, smh.begin() + 2 * rs, tot_sd);
    return err;
  });
  if (rc || len == 0) return rc;
  double* const outs[2] = {fn_mean, fn_sd};
  return for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(values, h->st, [&] { return launch_ceig_values(c, f, r0, rows, r.x, h->st); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = r.to_host(r0, rows, outs, fn_quant, fn_trace);
    if (err.empty()) collect(h, values, PT_CEIG_VALUES);
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
  if (perm && perm_check(ck, perm)) return 1;
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

