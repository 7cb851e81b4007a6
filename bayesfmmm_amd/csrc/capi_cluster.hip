// C ABI of the sampler (include/bfmmm.h), the cluster-level calls over the chain slots: the label alignment against a pivot and
// the reference's rescale step per draw; under either labelling the pooled summaries of a chain array, the cluster mean functions
// with their bands, the cluster covariance surfaces with their bands and the contrasts of cluster mean functions and covariate
// effects; and the cluster eigenvalues and eigenfunctions under aligned labels.
// What an entry point is made of is capi_chain.hpp's, shared with capi_chain.hip and capi_loo.hip; a call that is rows and their
// reduction is its RowCall.  Written once here: one body per pair of calls that differ in the labelling alone (summary_call,
// mean_bands_call, ccov_call: `rescaled` says which), and SimBand, the simultaneous band of the covariance surfaces and the contrasts.
#include "capi_chain.hpp"

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

// ---- the pooled summaries of a chain array under either labelling (kernels_align.hip, kernels_rescale.hip) ---
// bfmmm_chain_diagnostics of `name` with every draw's components relabelled, and the quantiles of the same gathered rows, in chunks
// of consecutive elements: by the draw's row of perm (k_align_gather), or (rescaled) by its transform (k_rescale_gather): the
// reference rescales nu, Phi, eta and xi by A and Z by A^-1, and nothing else.
int summary_call(const char* fname, bfmmm_handle* h, const char* name, const int32_t* perm, const double* mix, const double* mix_inv,
                 int first_slot, int n_slots, const double* probs, int nq, int64_t max_workspace_bytes, double* rhat, double* ess_bulk,
                 double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd, double* quant, int64_t capacity,
                 bool rescaled) {
  SlotCheck ck{fname, h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {"name", name}}) || (rescaled ? ck.ptrs({{"mix", mix}, {"mix_inv", mix_inv}}) : ck.ptrs({{"perm", perm}})) ||
      ck.ptrs({{"rhat", rhat}, {"ess_bulk", ess_bulk}, {"ess_tail", ess_tail}, {"ess_mean", ess_mean}, {"mcse_mean", mcse_mean}, {"mean", mean},
               {"sd", sd}}) ||
      ck.range() || ck.budget_sign(max_workspace_bytes))
    return 1;
  const Ctx& c = h->c;          // chain 0 of the batch
  const std::string nm = name;
  const bool by_inverse = rescaled && nm == "Z";
  if (rescaled && !by_inverse && nm != "nu" && nm != "Phi" && nm != "eta" && nm != "xi")
    return fail(ck.fn + ": the reference defines no rescale for '" + nm + "' (only for nu, Phi, eta, xi and Z)");
  const ChainArr a = chain_array(c, h->T, nm);
  int64_t inner = 0;
  if (!a.p || !align_axis(c.d, nm, &inner) || (rescaled && inner < 1))
    return fail(ck.fn + (rescaled ? ": no array '" + nm + "' (covariate arrays exist once covariates were set)" : ": unknown name '" + nm + "'"));
  ck.tag = "(" + nm + ")";
  if (ck.capacity(capacity, a.len) || ck.row_limit() || ck.probs_list(probs, nq, 0, quant) || (!rescaled && ck.perm_check(perm))) return 1;
  const int C = h->nch, K = c.d.K;
  RowCall rows(ck, a.len, nq, true, rescaled ? PT_RESCALE_GATHER : PT_ALIGN_GATHER);
  if (rows.plan(max_workspace_bytes, 0, kNoCap, nullptr, probs)) return 1;
  int32_t* d_perm = nullptr;
  double* d_w = nullptr;
  if (rescaled) HIPCHK(rows.b.put(h, &d_w, by_inverse ? mix_inv : mix, rows.r.N * K * K));
  else HIPCHK(rows.b.put(h, &d_perm, perm, rows.r.N * K));
  const auto chain_bytes = a.cov ? c.chain_bytes_cov : c.chain_bytes;
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  return rows.run(outs, quant, nullptr, [&](int64_t p0, int cnt, double* d_x) {
    return rescaled ? launch_rescale_gather(a.p, chain_bytes, a.ss, a.ps, first_slot, n_slots, C, (int)p0, cnt, d_w, by_inverse ? 1 : K,
                                            by_inverse ? K : 1, K, inner, d_x, h->st)
                    : launch_align_gather(a.p, chain_bytes, a.ss, a.ps, first_slot, n_slots, C, (int)p0, cnt, d_perm, K, inner, d_x, h->st);
  });
}

// ---- the cluster mean functions with their bands under either labelling ------------------------------------
// Mean, sd and quantiles over the pooled draws of the K G cluster mean functions E nu_k, in chunks of consecutive rows: with the
// labels aligned by perm (k_align_project), or (rescaled) under the transform of every draw at the covariate setting x (D entries;
// null: nu alone; k_rescale_project).
int mean_bands_call(const char* fname, bfmmm_handle* h, const int32_t* perm, const double* mix, const double* E, int G, const double* x,
                    int first_slot, int n_slots, const double* probs, int nq, int64_t max_workspace_bytes, double* mean, double* sd,
                    double* quant, int64_t capacity, bool rescaled) {
  const SlotCheck ck{fname, h, first_slot, n_slots};
  if (ck.ptrs({{"h", h}, {rescaled ? "mix" : "perm", rescaled ? (const void*)mix : (const void*)perm}, {"E", E}, {"mean", mean}, {"sd", sd}}))
    return 1;
  if (G < 1) return fail(ck.fn + ": 'G' must be at least 1");
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.covariates("x", x) || ck.x_finite(x)) return 1;
  const Ctx& c = h->c;
  const int K = c.d.K, P = c.d.P;
  const int64_t len = (int64_t)K * G;
  if (ck.capacity(capacity, len, "rows") || ck.row_limit() || ck.probs_list(probs, nq, 0, quant) || (!rescaled && ck.perm_check(perm))) return 1;
  RowCall rows(ck, len, nq, false, rescaled ? PT_RESCALE_PROJECT : PT_ALIGN_PROJECT);
  if (rows.plan(max_workspace_bytes, 0, 65535, nullptr, probs)) return 1;
  double *d_E = nullptr, *d_mix = nullptr, *d_x = nullptr;
  int32_t* d_perm = nullptr;
  HIPCHK(rows.b.put(h, &d_E, E, (size_t)G * P));
  if (rescaled) HIPCHK(rows.b.put(h, &d_mix, mix, rows.r.N * K * K));
  else HIPCHK(rows.b.put(h, &d_perm, perm, rows.r.N * K));
  if (x) HIPCHK(rows.b.put(h, &d_x, x, (size_t)c.d.D));
  double* const outs[2] = {mean, sd};
  return rows.run(outs, quant, nullptr, [&](int64_t r0, int cnt, double* d_v) {
    return rescaled ? launch_rescale_project(c, d_E, G, d_mix, d_x, first_slot, n_slots, (int)r0, cnt, d_v, h->st)
                    : launch_align_project(c, d_E, G, d_perm, first_slot, n_slots, (int)r0, cnt, d_v, h->st);
  });
}

// ---- the simultaneous band of result rows e = r cells + g of m groups r ------------------------------------------
// dev[r N + cs]: the largest standardised deviation of draw cs over the entries of group r (the pairs of the covariance surfaces,
// the contrasts), which needs every chunk's mean and sd: with one chunk the caller's first sweep calls maxdev() on its values,
// with several sweep() forms them again.  finish(): crit[r], the (1 - alpha) quantile of dev's row r, and lower / upper = mean -/+
// crit sd.  Off (no band asked for): nothing on the device and no bytes.
struct SimBand {
  const SlotCheck& ck;
  bool on, long_dev;      // long_dev: dev's rows are sorted in the chunk's workspace too (RowReducer's also_sort)
  double p_crit;
  int64_t m, cells;
  size_t N;
  int pt_maxdev;          // the timer that counts maxdev's launches (-1: none)
  CcovCall shape;         // what launch_ccov_maxdev reads: m "pairs" of `cells` entries
  Timer t_maxdev;
  double *d_dev = nullptr, *d_crit = nullptr, *d_p = nullptr;

  SimBand(const SlotCheck& ck, bool on, double alpha, int64_t m, int G1, int G2, int diagonal, int pt_maxdev)
      : ck(ck), on(on), long_dev(on && ck.CS() > ccov_sort_rows()), p_crit(1.0 - alpha), m(m), cells(diagonal ? (int64_t)G1 : (int64_t)G1 * G2),
        N((size_t)ck.CS()), pt_maxdev(pt_maxdev) {
    shape.G1 = G1; shape.G2 = G2; shape.diagonal = diagonal ? 1 : 0; shape.n_pairs = m;
  }
  size_t doubles() const { return on ? (size_t)m * N + (size_t)m : 0; }      // dev and crit, of the bytes shared by the call
  // dev (the maximum starts from 0.0) and crit on the device, and 1 - alpha behind the 16 probabilities of d_probs
  int alloc(CallBufs& b, double* d_probs) {
    if (!on) return 0;
    bfmmm_handle* h = ck.h;
    d_p = d_probs + 16;
    if (pt_maxdev >= 0) HIPCHK(b.timers({&t_maxdev}));
    HIPCHK(copy_sync(h, d_p, &p_crit, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(b.get(&d_dev, (size_t)m * N));
    HIPCHK(b.get(&d_crit, (size_t)m));
    HIPCHK(hipMemsetAsync(d_dev, 0, sizeof(double) * (size_t)m * N, h->st));
    return 0;
  }
  // rows [r0, r0 + rows) of the chunk in r, with its mean and sd, into dev; collected() once the stream has been synchronised
  std::string maxdev(const RowReducer& r, int64_t r0, int rows) const {
    auto launch = [&] { return launch_ccov_maxdev(shape, (long long)N, r0, rows, r.x, r.mean, r.sd, d_dev, ck.h->st); };
    return pt_maxdev >= 0 ? timed(t_maxdev, ck.h->st, launch) : launch();
  }
  void collected() const { if (pt_maxdev >= 0) collect(ck.h, t_maxdev, pt_maxdev); }
  // the second sweep: values(r0, rows), the same kernel on the same tables, gives the same values, now against every chunk's mean and
  // sd from the host; its launches count in timer pt_values as the first sweep's do
  template <typename Values>
  int sweep(const RowReducer& r, int64_t len, int64_t chunk, const double* mean, const double* sd, const Timer& t_values, int pt_values, Values values) {
    bfmmm_handle* h = ck.h;
    return for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
      std::string err = timed(t_values, h->st, [&] { return values(r0, rows); });
      if (err.empty() && (copy_sync(h, r.mean, mean + r0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess ||
                          copy_sync(h, r.sd, sd + r0, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess))
        err = "copy of the chunk's mean and sd failed";
      if (err.empty()) err = maxdev(r, r0, rows);
      if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = "kernel failed";
      if (!err.empty()) return err;
      collect(h, t_values, pt_values);
      collected();
      return err;
    });
  }
  // crit[r], interpolated without an fma as k_fit_sim's is; long rows are sorted by k_bands_quantiles_big, in pieces of as many rows
  // as the chunk's sort workspace holds, and the rule read off them again.  Then the band of all len entries on the host.
  int finish(const RowReducer& r, int64_t chunk, int64_t len, const double* mean, const double* sd, double* crit, double* lower, double* upper) {
    bfmmm_handle* h = ck.h;
    const int rc = for_chunks(ck, m, long_dev ? std::min<int64_t>(m, chunk) : m, [&](int64_t p0, int cnt) {
      std::string err;
      if (!long_dev) err = launch_ccov_crit(d_dev + (size_t)p0 * N, (long long)N, cnt, p_crit, d_crit + p0, h->st);
      else {
        err = launch_bands_quantiles(d_dev + (size_t)p0 * N, (int)N, cnt, r.w, d_p, 1, d_crit + p0, h->st);
        if (err.empty()) err = launch_fit_quantiles(r.w, (int)r.ws.NP, (int)N, cnt, d_p, 1, d_crit + p0, h->st);
      }
      return err.empty() ? Back{h, p0, cnt}(crit, (const double*)(d_crit + p0), 1).done() : err;
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
};

// ---- cluster covariance surfaces with bands under either labelling (kernels_cluster_cov.hip) ------------------
// Mean, sd and quantiles over the pooled draws of c_r(g, h) = sum_m W1_k[g][m] W2_l[h][m] of the pairs r = (k, l), and the
// simultaneous band per pair: k_ccov_project once per call, then per chunk of consecutive result rows k_ccov_values into rows of
// C S values and launch_bands_moments and launch_bands_quantiles on them as they are, then SimBand.
// The labels of a draw are its row of perm, or (rescaled) its K x K transform mix[(cs K + k) K + c], under which the tables are
// filled raw and mixed in a second pass: W~_k = sum_c A[k][c] W_c (k_ccov_mix).
int ccov_call(const char* name, bfmmm_handle* h, const int32_t* perm, const double* mix, const double* E1, int G1, const double* E2,
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
  if ((band && ck.alpha_inside(alpha)) || (!rescaled && ck.perm_check(perm))) return 1;
  CcovCall f;
  f.G1 = G1; f.G2 = G2; f.diagonal = diagonal ? 1 : 0; f.first_slot = first_slot; f.n_slots = n_slots; f.n_pairs = m;
  const std::string bad = ccov_check(c, f);
  if (!bad.empty()) return fail(fn + ": " + bad);
  reset_timers(h, PT_CCOV_PROJECT, PT_CCOV_MAXDEV);
  if (m == 0) return 0;
  const size_t N = (size_t)ck.CS();
  SimBand sb(ck, band, alpha, m, G1, G2, diagonal, PT_CCOV_MAXDEV);
  RowReducer r(ck, nq, false, sb.long_dev);
  // shared by all rows: the tables, E1, E2, x, probs, perm, the pairs and, for the band, dev and crit; a row: its values, its sort
  // workspace, its mean, sd and quantiles
  const size_t tab1 = ccov_table_doubles(c, f, 0), tab2 = E2 ? ccov_table_doubles(c, f, 1) : 0;
  const size_t shared = sizeof(double) * (tab1 + tab2 + (size_t)G1 * P + (E2 ? (size_t)G2 * P : 0) + (x ? (size_t)D : 0) + 17 + sb.doubles()) +
                        (rescaled ? sizeof(double) * N * K * K : sizeof(int32_t) * ((N * K + 1) & ~(size_t)1)) + sizeof(int32_t) * 2 * (size_t)m;
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), shared, r.row_bytes(), len, 1 << 30, "row", &chunk)) return 1;
  const bool dev_now = band && chunk >= len;      // one chunk: its values are reused for the band's deviations
  HIPCHK(hipSetDevice(h->device));
  CallBufs b;
  double *d_E1 = nullptr, *d_E2 = nullptr, *d_x = nullptr, *d_probs = nullptr, *d_mix = nullptr;
  int32_t *d_perm = nullptr, *d_pairs = nullptr;
  Timer values;
  HIPCHK(b.timers({&values}));
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
  if (sb.alloc(b, d_probs)) return 1;
  f.E1 = d_E1; f.E2 = d_E2; f.x = d_x; f.perm = d_perm; f.mix = d_mix; f.pairs = d_pairs;
  if (once(ck, b, PT_CCOV_PROJECT, E2 ? 2 : 1, [&] { return launch_ccov_project(c, f, h->st); })) return 1;
  double* const outs[2] = {mean, sd};
  auto fill = [&](int64_t r0, int rows) { return launch_ccov_values(c, f, r0, rows, r.x, h->st); };
  const int rc = for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(values, h->st, [&] { return fill(r0, rows); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty() && dev_now) err = sb.maxdev(r, r0, rows);
    if (err.empty()) err = r.to_host(r0, rows, outs, quant, trace);
    if (!err.empty()) return err;
    collect(h, values, PT_CCOV);
    if (dev_now) sb.collected();
    return err;
  });
  if (rc || !band) return rc;
  if (!dev_now && sb.sweep(r, len, chunk, mean, sd, values, PT_CCOV, fill)) return 1;
  return sb.finish(r, chunk, len, mean, sd, crit, lower, upper);
}

}  // namespace

// ---- label alignment against a pivot (kernels_align.hip) -----------------------------------------------------------
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
  if (ck.capacity(capacity, (int64_t)(N * KK)) || (!transform && perm && ck.perm_check(perm))) return 1;
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

// ---- the thin exports of the bodies above ------------------------------------------------------------------------------------------
extern "C" int bfmmm_chain_aligned_summary(bfmmm_handle* h, const char* name, const int32_t* perm, int first_slot, int n_slots,
                                           const double* probs, int nq, int64_t max_workspace_bytes, double* rhat, double* ess_bulk,
                                           double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd, double* quant,
                                           int64_t capacity) {
  return summary_call("bfmmm_chain_aligned_summary", h, name, perm, nullptr, nullptr, first_slot, n_slots, probs, nq, max_workspace_bytes, rhat,
                      ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd, quant, capacity, false);
}

extern "C" int bfmmm_chain_rescaled_summary(bfmmm_handle* h, const char* name, const double* mix, const double* mix_inv, int first_slot,
                                            int n_slots, const double* probs, int nq, int64_t max_workspace_bytes, double* rhat,
                                            double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd,
                                            double* quant, int64_t capacity) {
  return summary_call("bfmmm_chain_rescaled_summary", h, name, nullptr, mix, mix_inv, first_slot, n_slots, probs, nq, max_workspace_bytes, rhat,
                      ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd, quant, capacity, true);
}

extern "C" int bfmmm_chain_cluster_mean_bands(bfmmm_handle* h, const int32_t* perm, const double* E, int G, int first_slot, int n_slots,
                                              const double* probs, int nq, int64_t max_workspace_bytes, double* mean, double* sd,
                                              double* quant, int64_t capacity) {
  return mean_bands_call("bfmmm_chain_cluster_mean_bands", h, perm, nullptr, E, G, nullptr, first_slot, n_slots, probs, nq, max_workspace_bytes,
                         mean, sd, quant, capacity, false);
}

extern "C" int bfmmm_chain_cluster_mean_bands_rescaled(bfmmm_handle* h, const double* mix, const double* E, int G, const double* x,
                                                       int first_slot, int n_slots, const double* probs, int nq, int64_t max_workspace_bytes,
                                                       double* mean, double* sd, double* quant, int64_t capacity) {
  return mean_bands_call("bfmmm_chain_cluster_mean_bands_rescaled", h, nullptr, mix, E, G, x, first_slot, n_slots, probs, nq,
                         max_workspace_bytes, mean, sd, quant, capacity, true);
}

extern "C" int bfmmm_chain_cluster_cov_bands(bfmmm_handle* h, const int32_t* perm, const double* E1, int G1, const double* E2, int G2,
                                             int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot, int n_slots,
                                             const double* probs, int nq, double alpha, int64_t max_workspace_bytes, double* mean, double* sd,
                                             double* quant, double* crit, double* lower, double* upper, double* trace, int64_t capacity) {
  return ccov_call("bfmmm_chain_cluster_cov_bands", h, perm, nullptr, E1, G1, E2, G2, diagonal, pairs, n_pairs, x, first_slot, n_slots, probs, nq,
                   alpha, max_workspace_bytes, mean, sd, quant, crit, lower, upper, trace, capacity, false);
}

extern "C" int bfmmm_chain_cluster_cov_bands_rescaled(bfmmm_handle* h, const double* mix, const double* E1, int G1, const double* E2, int G2,
                                                      int diagonal, const int32_t* pairs, int n_pairs, const double* x, int first_slot,
                                                      int n_slots, const double* probs, int nq, double alpha, int64_t max_workspace_bytes,
                                                      double* mean, double* sd, double* quant, double* crit, double* lower, double* upper,
                                                      double* trace, int64_t capacity) {
  return ccov_call("bfmmm_chain_cluster_cov_bands_rescaled", h, nullptr, mix, E1, G1, E2, G2, diagonal, pairs, n_pairs, x, first_slot, n_slots,
                   probs, nq, alpha, max_workspace_bytes, mean, sd, quant, crit, lower, upper, trace, capacity, true);
}

// ---- contrasts of cluster mean functions and covariate effects (kernels_cluster_contrast.hip) ---------------------
// k_contrast_coef once per call, then per chunk of consecutive result rows e = r G + g: k_contrast_values into rows of C S values,
// the unchanged RowReducer, k_rows_count for prob_positive and k_contrast_norm into the R norm rows, which the second RowReducer (the
// seven statistics and the quantiles) reduces once the last chunk is done.  The band is SimBand's over R groups of G entries, without
// a timer for its deviations; then k_rows_count on dev against t_r for p_sim.
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
  if (ck.covariates("w_eta", w_eta)) return 1;
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
  SimBand sb(ck, band, alpha, R, G, G, 1, -1);
  RowReducer r(ck, nq, false, sb.long_dev), nr(ck, nq, true);
  // shared by all rows: the coefficient table, E, the label maps, the weights, probs, the R norm rows with their statistics, the
  // counts of p_sim and, for the band, dev, crit and t; a row: its values, its sort workspace, its mean, sd, quantiles and count
  const size_t shared = sizeof(double) * ((size_t)R * P * N + (size_t)G * P + N * K * K + (size_t)R * (K + KD) + (size_t)G + 17 + sb.doubles() +
                                          (band ? (size_t)R : 0)) +
                        nr.row_bytes() * (size_t)R + sizeof(int32_t) * (((size_t)R + 1) & ~(size_t)1);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), shared, r.row_bytes() + sizeof(double), len, 65535, "row", &chunk)) return 1;
  const bool dev_now = band && chunk >= len;      // one chunk: its values are reused for the band's deviations
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_CONTRAST_COEF, PT_CONTRAST_NORM);
  CallBufs b;
  double *d_E = nullptr, *d_mix = nullptr, *d_wn = nullptr, *d_we = nullptr, *d_w = nullptr, *d_probs = nullptr, *d_thr = nullptr;
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
  if (sb.alloc(b, d_probs)) return 1;
  if (band) HIPCHK(b.get(&d_thr, (size_t)R));
  f.E = d_E; f.mix = d_mix; f.w_nu = d_wn; f.w_eta = d_we; f.w = d_w;
  if (once(ck, b, PT_CONTRAST_COEF, 0, [&] { return launch_contrast_coef(c, f, h->st); })) return 1;
  double* const outs[2] = {mean, sd};
  auto fill = [&](int64_t r0, int rows) { return launch_contrast_values(c, f, r0, rows, r.x, h->st); };
  int rc = for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(values, h->st, [&] { return fill(r0, rows); });
    if (err.empty()) err = r.reduce(rows);
    if (err.empty()) err = launch_rows_count(r.x, (long long)N, rows, nullptr, 0, d_cnt, h->st);
    if (err.empty()) err = timed(norm, h->st, [&] { return launch_contrast_norm(c, f, r0, rows, r.x, nr.x, h->st); });
    if (err.empty() && dev_now) err = sb.maxdev(r, r0, rows);
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
  if (!dev_now && sb.sweep(r, len, chunk, mean, sd, values, PT_CONTRAST_VALUES, fill)) return 1;
  if (sb.finish(r, chunk, len, mean, sd, crit, lower, upper)) return 1;
  // t_r: the largest |mean| / sd over the grid points with sd > 0; the band at level p excludes zero somewhere where crit_p < t_r
  std::vector<double> thr((size_t)R, 0.0);
  for (int64_t e = 0; e < len; ++e)
    if (sd[e] > 0.0) thr[(size_t)(e / G)] = std::max(thr[(size_t)(e / G)], std::fabs(mean[e]) / sd[e]);
  HIPCHK(copy_sync(h, d_thr, thr.data(), sizeof(double) * (size_t)R, hipMemcpyHostToDevice));
  return for_chunks(ck, 1, 1, [&](int64_t, int) {
    const std::string err = launch_rows_count(sb.d_dev, (long long)N, R, d_thr, 1, d_cntR, h->st);
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
  if (ck.perm_check(perm)) return 1;
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
  RowCall rows(ck, len, nq, false, PT_CEIG_VALUES);
  RowReducer sm(ck, nq, false), sv(ck, 0, true);
  // shared by all rows: Q, R, E, w, x, ref, probs, the small rows with their results and workspaces, the b of every draw, the
  // status words and perm; an eigenfunction row: its values, its sort workspace, its mean, sd and quantiles
  const size_t small_ws = rs * sm.res_doubles() + KM * sv.res_doubles();
  const size_t shared = sizeof(double) * ((size_t)P * P + (with_ref ? (size_t)K * J * P + (size_t)len : 0) + (size_t)G * P + (w ? (size_t)G : 0) +
                                          (x ? (size_t)D : 0) + 16 + N * rs + small_ws + N * K * J * P) +
                        sizeof(int32_t) * 2 * N * K;
  if (rows.plan(max_workspace_bytes, shared, 1 << 30, "row", probs)) return 1;
  CallBufs& b = rows.b;
  double *d_E = nullptr, *d_w = nullptr, *d_x = nullptr, *d_ref = nullptr, *d_small = nullptr, *d_sres = nullptr;
  int32_t *d_perm = nullptr, *d_status = nullptr;
  Timer gram, solve;
  HIPCHK(b.timers({&gram, &solve}));
  HIPCHK(b.put(h, &d_E, E, (size_t)G * P));
  if (w) HIPCHK(b.put(h, &d_w, w, (size_t)G));
  if (x) HIPCHK(b.put(h, &d_x, x, (size_t)D));
  if (with_ref) {
    HIPCHK(b.put(h, &d_ref, ref, (size_t)len));
    HIPCHK(b.get(&f.R, (size_t)K * J * P));
  }
  HIPCHK(b.put(h, &d_perm, perm, N * K));
  HIPCHK(b.get(&d_status, N * K));
  sm.probs = rows.r.probs;
  HIPCHK(b.get(&f.Q, (size_t)P * P));
  HIPCHK(b.get(&d_small, N * rs));
  HIPCHK(b.get(&d_sres, small_ws));
  HIPCHK(b.get(&f.b, N * K * J * P));
  f.E = d_E; f.w = d_w; f.x = d_x; f.ref = d_ref; f.perm = d_perm; f.status = d_status;
  f.lam = d_small; f.pve = d_small + N * KM; f.tot = d_small + 2 * N * KM;
  sm.place(d_small, d_sres, (int64_t)rs);
  sv.place(d_small, d_sres + rs * sm.res_doubles(), (int64_t)KM);
  std::vector<int32_t> st_host(N * K);
  std::vector<double> smh(2 * rs);      // mean and sd of the small rows
  // the solve and the small rows
  const int rc = for_chunks(ck, 1, 1, [&](int64_t, int) {
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
  return rows.run(outs, fn_quant, fn_trace, [&](int64_t r0, int cnt, double* d_v) { return launch_ceig_values(c, f, r0, cnt, d_v, h->st); });
}
