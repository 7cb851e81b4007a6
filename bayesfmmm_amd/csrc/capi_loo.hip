// C ABI of the sampler (include/bfmmm.h), the PSIS-LOO family over the chain slots: over curves (bfmmm_chain_loo),
// over curves with the memberships integrated out (bfmmm_chain_loo_marginal, 7o) and the same under the Laplace mixture proposal
// (bfmmm_chain_loo_marginal_laplace, 7p), over observations with the LOO-PIT (bfmmm_chain_loo_pointwise, 7q), over blocks of
// observations within curves (bfmmm_chain_loo_blocks, 7s) and chain by chain over curves or observations
// (bfmmm_chain_loo_by_chain, 7v).  The entry points are built as capi_chain.hip's, from capi_chain.hpp.
// What several of them do is written once here: psis_step for the PSIS pass of a chunk with its handshake between the two streams,
// kPsisNames for the six arrays it fills, DenseBasis for the dense basis rows of the two row calls, row_chunk_end for what they
// finish on the host, pointwise_tiles and pointwise_chunk for the tile plan and the launch of the observation-level calls.  The two
// marginal calls share psis_step alone: their checks interleave and their chunk bodies are short.
#include "capi_chain.hpp"

namespace {

// ---- the PSIS pass of a chunk ------------------------------------------------------------------------------------------------
// The six results of post_psis_device, in its order, by name: the null checks of the six arrays `res` of a call.
constexpr const char* kPsisNames[6] = {"lppd", "elpd_loo", "p_loo", "pareto_k", "elpd_waic", "p_waic"};
int psis_ptrs(const SlotCheck& ck, double* const (&res)[6]) {
  for (int v = 0; v < 6; ++v)
    if (ck.ptrs({{kPsisNames[v], res[v]}})) return 1;
  return 0;
}

// PSIS and WAIC of the `rows` rows of N draws at d_x into the six arrays of res from entry `at` on; with d_aux also the expectations
// of its n_aux matrices, `stride` apart, into expect (host, n_aux x rows).  post_psis_device runs on the device's default stream: the
// caller has drained the sampler's.  With a timer the device time between its events there goes to pt.  Answers "" or what failed.
std::string psis_step(bfmmm_handle* h, const double* d_x, size_t N, int rows, double* const (&res)[6], int64_t at, const Timer* t = nullptr,
                      int pt = 0, const double* d_aux = nullptr, int n_aux = 0, size_t stride = 0, double* expect = nullptr) {
  double* const outs[6] = {res[0] + at, res[1] + at, res[2] + at, res[3] + at, res[4] + at, res[5] + at};
  if (t) (void)hipEventRecord(t->from, nullptr);
  const int prc = d_aux ? post_psis_expect_device(d_x, (long long)N, rows, (int)N, d_aux, n_aux, (long long)stride, outs, expect)
                        : post_psis_device(d_x, (long long)N, rows, (int)N, outs);
  if (t) (void)hipEventRecord(t->to, nullptr);
  if (prc) return bfmmm_entry_last_error();
  if (t && hipEventSynchronize(t->to) != hipSuccess) return kBackFailed;
  if (t) collect(h, *t, pt);
  return "";
}

// ---- the two row calls -----------------------------------------------------------------------------------------------------------
// The dense basis rows of a row kernel's tiles: one launch_stats_functional for the whole call where the handle has the spline
// inputs, the chunk's rows from the handle's host copy where it was created from a basis, none for the multivariate model.
struct DenseBasis {
  bfmmm_handle* h;
  bool from_basis, spline;
  int n, P;
  std::vector<int> ni;            // the curves' observation counts
  std::vector<int64_t> off;       // and their prefix sums: the first row of a curve in y and in the basis
  double* d_B = nullptr;          // what the kernel indexes: every observation's row (spline) or the chunk's (from a basis)
  std::vector<double> hB;

  explicit DenseBasis(bfmmm_handle* h) : h(h), from_basis(!h->B_host.empty()), spline(!h->c.d.mv && !from_basis), n(h->c.d.n), P(h->c.d.P) {}
  int counts() {
    ni.resize((size_t)n);
    HIPCHK(hipStreamSynchronize(h->st));
    HIPCHK(copy_sync(h, ni.data(), h->c.ni, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    off.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + ni[i];
    return 0;
  }
  // of the budget: the rows of every observation with the scratch record of their launch; a tile's rows from a host basis
  size_t shared_bytes() const { return spline ? sizeof(double) * ((size_t)h->n_obs * P + (size_t)n * h->c.d.LREC) + sizeof(int) * ((size_t)n + 1) : 0; }
  size_t tile_bytes() const { return from_basis ? sizeof(double) * (size_t)LP_ROWS * P : 0; }
  // the buffers for chunks of `chunk` tiles, and the launch under timer pt
  int prepare(const SlotCheck& ck, CallBufs& b, int64_t chunk, int pt) {
    if (spline) {
      const Dims& d = h->c.d;
      double* rec_tmp = nullptr;
      int *ni_tmp = nullptr, *d_err = nullptr;
      HIPCHK(b.get(&d_B, (size_t)h->n_obs * P));
      HIPCHK(b.get(&rec_tmp, (size_t)n * d.LREC));
      HIPCHK(b.get(&ni_tmp, (size_t)n));
      HIPCHK(b.get(&d_err, 1));
      HIPCHK(hipMemsetAsync(d_err, 0, sizeof(int), h->st));
      return once(ck, b, pt, 0, [&] {
        const int bad = launch_stats_functional(h->cfg.basis_degree, n, P, d.LREC, h->d_off, h->d_t, h->d_y, h->d_knots, h->n_knots, rec_tmp, ni_tmp, d_B, d_err, h->st);
        return std::string(bad ? "unsupported basis_degree" : "");
      });
    }
    if (from_basis) {
      HIPCHK(b.get(&d_B, (size_t)chunk * LP_ROWS * P));
      hB.resize((size_t)chunk * LP_ROWS * P);
    }
    return 0;
  }
  // From a host basis: `count` rows of it from row src on become rows dst .. of the chunk's, then the chunk's `rows` rows go up.
  // Nothing to do otherwise.  False: the copy failed.
  void stage(int64_t src, int count, int64_t dst) {
    if (from_basis) std::copy(h->B_host.begin() + (size_t)src * P, h->B_host.begin() + (size_t)(src + count) * P, hB.begin() + (size_t)dst * P);
  }
  bool upload(int rows) {
    return !from_basis || copy_sync(h, d_B, hB.data(), sizeof(double) * (size_t)rows * P, hipMemcpyHostToDevice) == hipSuccess;
  }
};

// The end of a chunk of `rows` rows at `base` of the result: pit, mean and sd from the expectations of the three auxiliaries in hexp
// (Phi(z), m, m^2 + v; a matrix after the other) and, where var_trace is asked for, the variance in place of the fourth matrix of
// d_x, its copy to the host and its time into pt.
std::string row_chunk_end(bfmmm_handle* h, const std::vector<double>& hexp, int64_t base, int rows, double* pit, double* mean, double* sd,
                          double* d_x, size_t stride, size_t N, double* var_trace, const Timer& vark, int pt) {
  for (int r = 0; r < rows; ++r) {
    const double e1 = hexp[(size_t)rows + r];
    pit[base + r] = hexp[(size_t)r];
    mean[base + r] = e1;
    sd[base + r] = std::sqrt(std::max(0.0, hexp[2 * (size_t)rows + r] - e1 * e1));
  }
  if (!var_trace) return "";
  std::string err = timed(vark, h->st, [&] { return launch_loo_pointwise_var(d_x + 2 * stride, d_x + 3 * stride, (size_t)rows * N, h->st); });
  if (err.empty()) err = Back{h, base, rows}(var_trace, (const double*)(d_x + 3 * stride), N).done();
  if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
  if (err.empty()) collect(h, vark, pt);
  return err;
}

// The row tiles of bfmmm_chain_loo_pointwise for the m selected curves (curves null: curve j is j), in the order of the result:
// up to LP_ROWS consecutive observations of a curve each.  Answers the rows of the result.
int64_t pointwise_tiles(const DenseBasis& basis, const int32_t* curves, int64_t m, std::vector<LpTile>& tiles) {
  int64_t total = 0;
  for (int64_t j = 0; j < m; ++j) {
    const int i = curves ? curves[j] : (int)j;
    for (int r0 = 0; r0 < basis.ni[i]; r0 += LP_ROWS) {
      const int rows = std::min(LP_ROWS, basis.ni[i] - r0);
      tiles.push_back({i, rows, basis.off[i] + r0, basis.off[i] + r0, total});
      total += rows;
    }
  }
  return total;
}

// Tiles [p0, p0 + cnt) of that list as a chunk: their rows counted from the chunk's first, *base of the result, into ht and to the
// device with their basis rows, then k_loo_pointwise on the chunk's *rows rows between the events of kern.  "" or what failed.
std::string pointwise_chunk(const SlotCheck& ck, DenseBasis& basis, const std::vector<LpTile>& tiles, int64_t p0, int cnt, std::vector<LpTile>& ht,
                            LpTile* d_tiles, const Timer& kern, double* d_x, size_t stride, int64_t* base, int* rows) {
  bfmmm_handle* h = ck.h;
  *base = tiles[(size_t)p0].out_row;
  int64_t rows64 = 0;
  for (int q = 0; q < cnt; ++q) {
    LpTile t = tiles[(size_t)p0 + q];
    t.out_row -= *base;
    basis.stage(t.b0, t.rows, t.out_row);
    if (basis.from_basis) t.b0 = t.out_row;
    ht[(size_t)q] = t;
    rows64 = t.out_row + t.rows;
  }
  *rows = (int)rows64;
  if (copy_sync(h, d_tiles, ht.data(), sizeof(LpTile) * (size_t)cnt, hipMemcpyHostToDevice) != hipSuccess || !basis.upload(*rows))
    return std::string(kBackFailed);
  return timed(kern, h->st, [&] {
    return launch_loo_pointwise(h->c, d_tiles, cnt, basis.d_B, h->d_y, ck.first_slot, ck.n_slots, d_x, stride, h->st);
  });
}

}  // namespace

// PSIS-LOO and WAIC over curves with the chains pooled: a row is the C n_slots draws of a curve, chain-major, relative
// efficiency 1.  Chunks of consecutive curves go through the same post_psis_device on the device.
extern "C" int bfmmm_chain_loo(bfmmm_handle* h, int first_slot, int n_slots, int64_t max_workspace_bytes, double* lppd,
                               double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_loo", h, first_slot, n_slots};
  double* const res[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  if (ck.ptrs({{"h", h}}) || psis_ptrs(ck, res) || ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, h->c.d.n) ||
      ck.row_limit())
    return 1;
  const int64_t len = h->c.d.n;
  const long long CS = ck.CS();
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), 0, sizeof(double) * (size_t)CS, len, kNoCap, nullptr, &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_CURVE_LL, PT_CURVE_LL);
  CallBufs b;
  double* d_x = nullptr;
  HIPCHK(b.get(&d_x, (size_t)CS * (size_t)chunk));
  return for_chunks(ck, len, chunk, [&](int64_t p0, int rows) {
    std::string err = curve_ll_timed(ck, (int)p0, rows, d_x);
    // post_psis_device runs on the device's default stream: the matrix must be complete before it starts
    if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = "kernel failed";
    if (!err.empty()) return err;
    curve_ll_collect(h);
    return psis_step(h, d_x, (size_t)CS, rows, res, p0);
  });
}

// ---- marginal PSIS-LOO over curves, the memberships integrated out (kernels_loo_marginal.hip) ------------------------
// Per chunk of consecutive curves: k_predict on the resident records (the call of 7m with f.rec = c.rec, r = the curve's index, no
// stats launch and no copy) into lpd_t, ess_t and a_last; with `refine` the count of the selected pairs, their list at the
// prefix of the counts formed here, and k_lz_refine over the list; then k_lz_count once more for what is reported and
// post_psis_device on the chunk's lpd_t, as bfmmm_chain_loo calls it.
extern "C" int bfmmm_chain_loo_marginal(bfmmm_handle* h, int first_slot, int n_slots, int n_samples, int n_stages, uint64_t seed, int refine,
                                        double ess_floor, int refine_samples, int refine_stages, int64_t max_workspace_bytes,
                                        double* lppd, double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic,
                                        double* ess_mean, double* ess_min, int32_t* n_refined, int32_t* n_below,
                                        double* lpd_trace, double* ess_trace, double* ess_trace_first,
                                        int32_t* refined_index, double* refine_prop, double* refine_samples_out, int64_t* n_ref,
                                        int64_t capacity, int64_t ref_capacity) {
  const SlotCheck ck{"bfmmm_chain_loo_marginal", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  double* const res[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  if (ck.ptrs({{"h", h}}) || psis_ptrs(ck, res) || ck.ptrs({{"ess_mean", ess_mean}, {"ess_min", ess_min}, {"n_refined", n_refined}, {"n_below", n_below}}))
    return 1;
  const bool ref_out = refined_index || refine_prop || refine_samples_out;
  if (ref_out && ck.ptrs({{"n_ref", n_ref}})) return 1;
  const int J = n_samples, R = n_stages, J2 = refine_samples, R2 = refine_stages;
  if (J < 1) return fail(fn + ": 'n_samples' must be at least 1, got " + std::to_string(J));
  if (R < 1) return fail(fn + ": 'n_stages' must be at least 1, got " + std::to_string(R));
  if (J2 < 1) return fail(fn + ": 'refine_samples' must be at least 1, got " + std::to_string(J2));
  if (R2 < 1) return fail(fn + ": 'refine_stages' must be at least 1, got " + std::to_string(R2));
  if (!(std::isfinite(ess_floor) && ess_floor >= 0.0)) return fail(fn + ": 'ess_floor' must be finite and not negative, got " + std::to_string(ess_floor));
  const Ctx& c = h->c;
  const Dims& d = c.d;
  const int n = d.n, K = d.K;
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, n, "rows") || ck.row_limit()) return 1;
  if (ref_out && ref_capacity < 0) return fail(fn + ": 'ref_capacity' must not be negative");
  // the RNG indices ((i R + st) J + j) K + k and ((i R2 + st) J2 + j) K + k are 32-bit counter words
  if ((long double)n * (long double)R * (long double)J * (long double)K > 4294967296.0L)
    return fail(fn + ": n x n_stages x n_samples x K = " + std::to_string(n) + " x " + std::to_string(R) + " x " + std::to_string(J) + " x " +
                std::to_string(K) + " exceeds the 4294967296 (2^32) indices of the random number counter");
  if (refine && (long double)n * (long double)R2 * (long double)J2 * (long double)K > 4294967296.0L)
    return fail(fn + ": n x refine_stages x refine_samples x K = " + std::to_string(n) + " x " + std::to_string(R2) + " x " + std::to_string(J2) +
                " x " + std::to_string(K) + " exceeds the 4294967296 (2^32) indices of the random number counter");
  PredictCall f;
  f.n_new = n; f.J = J; f.R = R; f.first_slot = first_slot; f.n_slots = n_slots; f.seed = seed;
  f.rec = c.rec; f.ni = c.ni; f.X = c.X;
  PredictCall f2 = f;
  f2.J = J2; f2.R = R2;
  std::string bad = predict_check(c, f, nullptr);
  if (bad.empty() && refine) bad = lz_check(c, J2, R2, nullptr);
  if (!bad.empty()) return fail(fn + ": " + bad);
  const size_t N = (size_t)ck.CS(), NK = N * (size_t)K;
  double* const want_prop = refine ? refine_prop : nullptr;
  double* const want_smp = refine ? refine_samples_out : nullptr;
  // a curve: lpd_t, ess_t and a_last (N (2 + K)), ess_mean and ess_min, the two counts and the offset; with `refine` the list (three
  // ints a pair) and, where asked for, the proposals and the samples of the refinement, as if every pair were refined
  const size_t per_curve = sizeof(double) * (N * (2 + (size_t)K) + 2 + (want_prop ? NK * R2 : 0) + (want_smp ? NK * R2 * (size_t)J2 : 0)) +
                           sizeof(int32_t) * (2 + (refine ? 3 * N + 1 : 0)) + sizeof(int64_t);
  const size_t budget = budget_of(max_workspace_bytes);
  if (want_smp && budget < per_curve)
    return fail(fn + ": 'refine_samples_out' of one curve (n_chains x n_slots x refine_stages x refine_samples x K doubles) with the rest need " +
                std::to_string(per_curve) + " bytes, above 'max_workspace_bytes' = " + std::to_string(budget) + " " +
                SlotCheck::plan_text(0, per_curve, "curve"));
  int64_t chunk = 0;
  const int64_t cells = (int64_t)std::max<size_t>(1, per_curve / sizeof(double) / std::max<size_t>(N, 1));
  if (ck.units(budget, 0, per_curve, n, cells_cap(cells), "curve", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_LOO_MARGINAL, PT_LOO_MARGINAL_PSIS);
  CallBufs b;
  double *d_tr = nullptr, *d_out = nullptr, *d_prop = nullptr, *d_smp = nullptr;
  int32_t *d_cnt = nullptr, *d_list = nullptr;
  int64_t* d_off = nullptr;
  Timer first, count, list, refk, pool, psis;
  HIPCHK(b.timers({&first, &count, &list, &refk, &pool, &psis}));
  HIPCHK(b.get(&d_tr, (size_t)chunk * (2 * N + NK)));
  HIPCHK(b.get(&d_out, 2 * (size_t)chunk));
  HIPCHK(b.get(&d_cnt, 2 * (size_t)chunk));
  if (refine) {
    HIPCHK(b.get(&d_off, (size_t)chunk));
    HIPCHK(b.get(&d_list, 3 * (size_t)chunk * N));
  }
  if (want_prop) HIPCHK(b.get(&d_prop, (size_t)chunk * NK * R2));
  if (want_smp) HIPCHK(b.get(&d_smp, (size_t)chunk * NK * R2 * J2));
  double* d_lpd_t = d_tr;
  double* d_ess_t = d_lpd_t + (size_t)chunk * N;
  double* d_alast = d_ess_t + (size_t)chunk * N;
  double* d_emean = d_out;
  double* d_emin = d_emean + chunk;
  int32_t* d_below = d_cnt + chunk;
  std::vector<int32_t> hcnt((size_t)chunk);
  std::vector<int64_t> hoff((size_t)chunk);
  int64_t total_ref = 0;
  const int rc = for_chunks(ck, n, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(first, h->st, [&] {
      return launch_predict(c, f, (int)r0, rows, d_lpd_t, d_ess_t, nullptr, nullptr, nullptr, nullptr, h->st, refine ? d_alast : nullptr);
    });
    if (err.empty()) err = Back{h, r0, rows}(ess_trace_first, d_ess_t, N).queued();
    int64_t n_list = 0;
    std::fill(n_refined + r0, n_refined + r0 + rows, 0);
    if (err.empty() && refine) {
      err = timed(count, h->st, [&] { return launch_lz_count((long long)N, rows, d_lpd_t, d_ess_t, ess_floor, d_cnt, nullptr, nullptr, h->st); });
      if (err.empty() && copy_sync(h, hcnt.data(), d_cnt, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost) != hipSuccess) err = kBackFailed;
      if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
      if (!err.empty()) return err;
      for (int r = 0; r < rows; ++r) {
        if (hcnt[r] < 0 || (size_t)hcnt[r] > N) return std::string("k_lz_count: a count outside 0 .. n_chains x n_slots");
        hoff[r] = n_list;
        n_list += hcnt[r];
        n_refined[r0 + r] = hcnt[r];
      }
      if (n_list > 0) {
        if (ref_out && total_ref + n_list > ref_capacity)
          return "'ref_capacity' below the " + std::to_string(total_ref + n_list) + " pairs refined up to curve " + std::to_string(r0 + rows - 1);
        if (copy_sync(h, d_off, hoff.data(), sizeof(int64_t) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess) return std::string(kBackFailed);
        err = timed(list, h->st, [&] {
          return launch_lz_list((long long)N, n_slots, (int)r0, rows, d_lpd_t, d_ess_t, ess_floor, d_off, (long long)n_list, d_list, h->st);
        });
        if (err.empty())
          err = timed(refk, h->st, [&] {
            return launch_lz_refine(c, f2, (int)r0, rows, d_list, (long long)n_list, d_lpd_t, d_ess_t, d_alast, d_prop, d_smp, h->st);
          });
        if (err.empty())
          err = Back{h, total_ref, (int)n_list}(refined_index, d_list, 3)(want_prop, d_prop, (size_t)K * R2)(want_smp, d_smp, (size_t)K * R2 * J2).queued();
      }
    }
    if (err.empty())
      err = timed(pool, h->st, [&] { return launch_lz_count((long long)N, rows, d_lpd_t, d_ess_t, ess_floor, d_below, d_emean, d_emin, h->st); });
    if (err.empty())
      err = Back{h, r0, rows}(lpd_trace, d_lpd_t, N)(ess_trace, d_ess_t, N)(ess_mean, d_emean, 1)(ess_min, d_emin, 1)(n_below, d_below, 1).done();
    if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
    if (!err.empty()) return err;
    collect(h, first, PT_LOO_MARGINAL);
    if (refine) collect(h, count, PT_LOO_MARGINAL);
    if (n_list > 0) { collect(h, list, PT_LOO_MARGINAL); collect(h, refk, PT_LOO_MARGINAL); }
    collect(h, pool, PT_LOO_MARGINAL);
    total_ref += n_list;
    return psis_step(h, d_lpd_t, N, rows, res, r0, &psis, PT_LOO_MARGINAL_PSIS);
  });
  if (n_ref) *n_ref = total_ref;
  return rc;
}

// ---- the marginal PSIS-LOO under the Laplace mixture proposal (kernels_predict_laplace.hip) --------------------------
// Per chunk of consecutive curves: k_predict_lap on the resident records as the first and only pass (as bfmmm_chain_loo_marginal
// runs k_predict on them), k_lz_count for what is reported and post_psis_device on the chunk's lpd_t.  There is no refinement.
extern "C" int bfmmm_chain_loo_marginal_laplace(bfmmm_handle* h, int first_slot, int n_slots, int n_samples, uint64_t seed, double ess_floor,
                                                int64_t max_workspace_bytes,
                                                double* lppd, double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic,
                                                double* p_waic, double* ess_mean, double* ess_min, int32_t* n_below,
                                                double* lpd_trace, double* ess_trace, int32_t* n_modes, double* components,
                                                double* eta_samples, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_loo_marginal_laplace", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  double* const res[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  if (ck.ptrs({{"h", h}}) || psis_ptrs(ck, res) || ck.ptrs({{"ess_mean", ess_mean}, {"ess_min", ess_min}, {"n_below", n_below}})) return 1;
  const int J = n_samples;
  if (J < 1) return fail(fn + ": 'n_samples' must be at least 1, got " + std::to_string(J));
  if (!(std::isfinite(ess_floor) && ess_floor >= 0.0)) return fail(fn + ": 'ess_floor' must be finite and not negative, got " + std::to_string(ess_floor));
  const Ctx& c = h->c;
  const Dims& d = c.d;
  const int n = d.n, K = d.K;
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.capacity(capacity, n, "rows") || ck.row_limit()) return 1;
  // the RNG index (i J + j)(K + 1) + . is a 32-bit counter word
  if ((long double)n * (long double)J * (long double)(K + 1) > 4294967296.0L)
    return fail(fn + ": n x n_samples x (K + 1) = " + std::to_string(n) + " x " + std::to_string(J) + " x " + std::to_string(K + 1) +
                " exceeds the 4294967296 (2^32) indices of the random number counter");
  PredictCall f;
  f.n_new = n; f.J = J; f.R = 1; f.first_slot = first_slot; f.n_slots = n_slots; f.seed = seed;
  f.rec = c.rec; f.ni = c.ni; f.X = c.X;
  const std::string bad = predict_lap_check(c, f, nullptr);
  if (!bad.empty()) return fail(fn + ": " + bad);
  const size_t N = (size_t)ck.CS(), CD = (size_t)predict_lap_comp_doubles(K);
  // a curve: lpd_t and ess_t (2 N), n_modes (an int a draw, counted as a double), ess_mean and ess_min, the count; the components
  // and the samples where asked for
  const size_t per_curve = sizeof(double) * (N * (3 + (components ? (size_t)(K + 2) * CD : 0) + (eta_samples ? (size_t)J * (K - 1) : 0)) + 2) +
                           sizeof(int32_t) * 2;
  const size_t budget = budget_of(max_workspace_bytes);
  int64_t chunk = 0;
  const int64_t cells = (int64_t)std::max<size_t>(1, per_curve / sizeof(double) / std::max<size_t>(N, 1));
  if (ck.units(budget, 0, per_curve, n, cells_cap(cells), "curve", &chunk)) return 1;
  HIPCHK(hipSetDevice(h->device));
  reset_timers(h, PT_LOO_MARGINAL_PSIS, PT_LOO_MARGINAL_PSIS);
  reset_timers(h, PT_LOO_MARGINAL_LAPLACE, PT_LOO_MARGINAL_LAPLACE);
  CallBufs b;
  double *d_tr = nullptr, *d_out = nullptr, *d_comp = nullptr, *d_eta = nullptr;
  int32_t *d_below = nullptr, *d_nm = nullptr;
  Timer first, pool, psis;
  HIPCHK(b.timers({&first, &pool, &psis}));
  HIPCHK(b.get(&d_tr, (size_t)chunk * 2 * N));
  HIPCHK(b.get(&d_out, 2 * (size_t)chunk));
  HIPCHK(b.get(&d_below, (size_t)chunk));
  HIPCHK(b.get(&d_nm, (size_t)chunk * N));
  if (components) HIPCHK(b.get(&d_comp, (size_t)chunk * N * (K + 2) * CD));
  if (eta_samples) HIPCHK(b.get(&d_eta, (size_t)chunk * N * J * (K - 1)));
  double* d_lpd_t = d_tr;
  double* d_ess_t = d_lpd_t + (size_t)chunk * N;
  double* d_emean = d_out;
  double* d_emin = d_emean + chunk;
  return for_chunks(ck, n, chunk, [&](int64_t r0, int rows) {
    std::string err = timed(first, h->st, [&] {
      return launch_predict_lap(c, f, (int)r0, rows, d_lpd_t, d_ess_t, nullptr, nullptr, d_nm, d_comp, d_eta, h->st);
    });
    if (err.empty())
      err = timed(pool, h->st, [&] { return launch_lz_count((long long)N, rows, d_lpd_t, d_ess_t, ess_floor, d_below, d_emean, d_emin, h->st); });
    if (err.empty())
      err = Back{h, r0, rows}(n_modes, (const int32_t*)d_nm, N)(components, (const double*)d_comp, N * (K + 2) * CD)(
                eta_samples, (const double*)d_eta, N * (size_t)J * (K - 1)).queued();
    if (err.empty())
      err = Back{h, r0, rows}(lpd_trace, (const double*)d_lpd_t, N)(ess_trace, (const double*)d_ess_t, N)(ess_mean, (const double*)d_emean, 1)(
                ess_min, (const double*)d_emin, 1)(n_below, (const int32_t*)d_below, 1).done();
    if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
    if (!err.empty()) return err;
    collect(h, first, PT_LOO_MARGINAL_LAPLACE);
    collect(h, pool, PT_LOO_MARGINAL_LAPLACE);
    return psis_step(h, d_lpd_t, N, rows, res, r0, &psis, PT_LOO_MARGINAL_PSIS);
  });
}

// ---- observation-level PSIS-LOO and LOO-PIT of the chain slots (kernels_loo_pointwise.hip) ---------------------------
// The unit of a chunk is a row tile: up to LP_ROWS consecutive observations of one curve, listed on the host in the order of the
// result (the curves as selected, then the observations).  Per chunk k_loo_pointwise fills the four matrices of the chunk's rows
// (log-likelihood, PIT, conditional mean, second moment; draw fastest, then chain), post_psis_expect_device takes PSIS on the first
// with the other three as auxiliaries, and the traces go to the host where asked for.  The dense basis rows: DenseBasis.
extern "C" int bfmmm_chain_loo_pointwise(bfmmm_handle* h, const int32_t* curves, int n_curves, int first_slot, int n_slots,
                                         int64_t max_workspace_bytes, double* lppd, double* elpd_loo, double* p_loo, double* pareto_k,
                                         double* elpd_waic, double* p_waic, double* pit, double* mean, double* sd, double* loglik_trace,
                                         double* pit_trace, double* mean_trace, double* var_trace, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_loo_pointwise", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  double* const res[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  if (ck.ptrs({{"h", h}}) || psis_ptrs(ck, res) || ck.ptrs({{"pit", pit}, {"mean", mean}, {"sd", sd}})) return 1;
  if (curves && n_curves < 1) return fail(fn + ": 'n_curves' must be at least 1 where 'curves' is given");
  int64_t m = 0;
  if (ck.curve_list(curves, n_curves, &m) || ck.range() || ck.budget_sign(max_workspace_bytes) || ck.row_limit()) return 1;
  const Ctx& c = h->c;
  const std::string bad = loo_pointwise_check(c);
  if (!bad.empty()) return fail(fn + ": " + bad);
  HIPCHK(hipSetDevice(h->device));
  // the tile list, from the curves' observation counts
  DenseBasis basis(h);
  if (basis.counts()) return 1;
  std::vector<LpTile> tiles;
  const int64_t total = pointwise_tiles(basis, curves, m, tiles);
  if (ck.capacity(capacity, total, "rows")) return 1;
  if (tiles.empty()) return 0;
  const size_t N = (size_t)ck.CS();
  // a tile: its rows of the four matrices, the nine results a row, its entry of the list and what DenseBasis takes
  const size_t per_tile = sizeof(double) * (size_t)LP_ROWS * (4 * N + 9) + basis.tile_bytes() + sizeof(LpTile);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), basis.shared_bytes(), per_tile, (int64_t)tiles.size(), (int64_t)1 << 24, "tile", &chunk)) return 1;
  reset_timers(h, PT_LOO_POINTWISE, PT_LOO_POINTWISE_PSIS);
  CallBufs b;
  double* d_x = nullptr;
  LpTile* d_tiles = nullptr;
  Timer kern, vark, psis;
  HIPCHK(b.timers({&kern, &vark, &psis}));
  const size_t stride = (size_t)chunk * LP_ROWS * N;
  HIPCHK(b.get(&d_x, 4 * stride));
  HIPCHK(b.get(&d_tiles, (size_t)chunk));
  if (basis.prepare(ck, b, chunk, PT_LOO_POINTWISE)) return 1;
  std::vector<LpTile> ht((size_t)chunk);
  std::vector<double> hexp;
  return for_chunks(ck, (int64_t)tiles.size(), chunk, [&](int64_t p0, int cnt) {
    int64_t base = 0;
    int rows = 0;
    std::string err = pointwise_chunk(ck, basis, tiles, p0, cnt, ht, d_tiles, kern, d_x, stride, &base, &rows);
    if (err.empty())
      err = Back{h, base, rows}(loglik_trace, (const double*)d_x, N)(pit_trace, (const double*)(d_x + stride), N)(
                mean_trace, (const double*)(d_x + 2 * stride), N).done();
    if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
    if (!err.empty()) return err;
    collect(h, kern, PT_LOO_POINTWISE);
    hexp.resize(3 * (size_t)rows);
    err = psis_step(h, d_x, N, rows, res, base, &psis, PT_LOO_POINTWISE_PSIS, d_x + stride, 3, stride, hexp.data());
    if (!err.empty()) return err;
    return row_chunk_end(h, hexp, base, rows, pit, mean, sd, d_x, stride, N, var_trace, vark, PT_LOO_POINTWISE);
  });
}

// ---- PSIS-LOO chain by chain ----------------------------------------------------------------------------------------
// A row of bfmmm_chain_loo's and of bfmmm_chain_loo_pointwise's chunk matrix holds its C S draws chain-major: the matrix is also
// rows x C rows of S = n_slots draws, and the same psis_step takes it as that.  unit 0 is bfmmm_chain_loo's chunk loop, unit 1
// bfmmm_chain_loo_pointwise's (its tile plan, pointwise_chunk and so k_loo_pointwise as they are; of the four matrices it fills only
// the log-density goes through PSIS, without auxiliaries).  Entry r C + c of the six arrays: chain c of row r.
extern "C" int bfmmm_chain_loo_by_chain(bfmmm_handle* h, int unit, const int32_t* curves, int n_curves, int first_slot, int n_slots,
                                        int64_t max_workspace_bytes, double* lppd, double* elpd_loo, double* p_loo, double* pareto_k,
                                        double* elpd_waic, double* p_waic, int64_t capacity) {
  const SlotCheck ck{"bfmmm_chain_loo_by_chain", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  double* const res[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  if (ck.ptrs({{"h", h}}) || psis_ptrs(ck, res)) return 1;
  if (unit != 0 && unit != 1) return fail(fn + ": 'unit' must be 0 (curve) or 1 (observation), got " + std::to_string(unit));
  if (unit == 0 && curves) return fail(fn + ": 'curves' must be null with 'unit' 0: the curves are not selected there");
  if (curves && n_curves < 1) return fail(fn + ": 'n_curves' must be at least 1 where 'curves' is given");
  int64_t m = 0;
  if (ck.curve_list(curves, n_curves, &m) || ck.range() || ck.budget_sign(max_workspace_bytes) || ck.row_limit(n_slots, "n_slots")) return 1;
  const int64_t C = h->nch;
  const size_t N = (size_t)ck.CS(), S = (size_t)n_slots;
  const int64_t row_cap = (int64_t)2147483647 / C;      // rows x C is the PSIS pass's count of rows, an int
  if (unit == 0) {
    const int64_t len = h->c.d.n;
    if (ck.capacity(capacity, len * C)) return 1;
    int64_t chunk = 0;
    if (ck.units(budget_of(max_workspace_bytes), 0, sizeof(double) * N, len, row_cap, nullptr, &chunk)) return 1;
    HIPCHK(hipSetDevice(h->device));
    reset_timers(h, PT_CURVE_LL, PT_CURVE_LL);
    CallBufs b;
    double* d_x = nullptr;
    HIPCHK(b.get(&d_x, N * (size_t)chunk));
    return for_chunks(ck, len, chunk, [&](int64_t p0, int rows) {
      std::string err = curve_ll_timed(ck, (int)p0, rows, d_x);
      if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = "kernel failed";
      if (!err.empty()) return err;
      curve_ll_collect(h);
      return psis_step(h, d_x, S, rows * (int)C, res, p0 * C);
    });
  }
  const std::string bad = loo_pointwise_check(h->c);
  if (!bad.empty()) return fail(fn + ": " + bad);
  HIPCHK(hipSetDevice(h->device));
  DenseBasis basis(h);
  if (basis.counts()) return 1;
  std::vector<LpTile> tiles;
  const int64_t total = pointwise_tiles(basis, curves, m, tiles);
  if (ck.capacity(capacity, total * C)) return 1;
  if (tiles.empty()) return 0;
  // a tile: its rows of the four matrices, the six results a (row, chain), its entry of the list and what DenseBasis takes
  const size_t per_tile = sizeof(double) * (size_t)LP_ROWS * (4 * N + 6 * (size_t)C) + basis.tile_bytes() + sizeof(LpTile);
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), basis.shared_bytes(), per_tile, (int64_t)tiles.size(),
               std::min<int64_t>((int64_t)1 << 24, std::max<int64_t>(1, row_cap / LP_ROWS)), "tile", &chunk))
    return 1;
  reset_timers(h, PT_LOO_POINTWISE, PT_LOO_POINTWISE_PSIS);
  CallBufs b;
  double* d_x = nullptr;
  LpTile* d_tiles = nullptr;
  Timer kern, psis;
  HIPCHK(b.timers({&kern, &psis}));
  const size_t stride = (size_t)chunk * LP_ROWS * N;
  HIPCHK(b.get(&d_x, 4 * stride));
  HIPCHK(b.get(&d_tiles, (size_t)chunk));
  if (basis.prepare(ck, b, chunk, PT_LOO_POINTWISE)) return 1;
  std::vector<LpTile> ht((size_t)chunk);
  return for_chunks(ck, (int64_t)tiles.size(), chunk, [&](int64_t p0, int cnt) {
    int64_t base = 0;
    int rows = 0;
    std::string err = pointwise_chunk(ck, basis, tiles, p0, cnt, ht, d_tiles, kern, d_x, stride, &base, &rows);
    // post_psis_device runs on the device's default stream: the matrix must be complete before it starts
    if (err.empty() && (hipStreamSynchronize(h->st) != hipSuccess || hipGetLastError() != hipSuccess)) err = kBackFailed;
    if (!err.empty()) return err;
    collect(h, kern, PT_LOO_POINTWISE);
    return psis_step(h, d_x, S, rows * (int)C, res, base * C, &psis, PT_LOO_POINTWISE_PSIS);
  });
}

// ---- leave-block-out PSIS cross-validation within curves (kernels_loo_blocks.hip) ------------------------------------
// The unit of a chunk is a row tile of gathered rows: consecutive blocks of the list that belong to the same curve share a tile while
// they fit LP_ROWS rows, one row per listed observation, in the order of the lists.  Per chunk the tile and row tables go up,
// k_loo_blocks fills the four matrices of the chunk's rows (every row of a block with the block's log-density), the traces go to the
// host where asked for (loglik_trace from each block's first row), post_psis_expect_device takes PSIS on the first matrix with the
// other three as auxiliaries, and the host keeps the six PSIS results of each block's first row and finishes pit, mean and sd of
// every row.  The dense basis rows: DenseBasis.
extern "C" int bfmmm_chain_loo_blocks(bfmmm_handle* h, const int32_t* block_curve, const int64_t* block_offsets, const int32_t* block_obs,
                                      int64_t n_blocks, int first_slot, int n_slots, int64_t max_workspace_bytes, double* lppd,
                                      double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic, double* pit,
                                      double* mean, double* sd, double* loglik_trace, double* pit_trace, double* mean_trace,
                                      double* var_trace, int64_t block_capacity, int64_t row_capacity) {
  const SlotCheck ck{"bfmmm_chain_loo_blocks", h, first_slot, n_slots};
  const std::string& fn = ck.fn;
  double* const res[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  if (ck.ptrs({{"h", h}, {"block_curve", block_curve}, {"block_offsets", block_offsets}, {"block_obs", block_obs}}) || psis_ptrs(ck, res) ||
      ck.ptrs({{"pit", pit}, {"mean", mean}, {"sd", sd}}))
    return 1;
  if (n_blocks < 1) return fail(fn + ": 'n_blocks' must be at least 1");
  if (block_offsets[0] != 0) return fail(fn + ": 'block_offsets'[0] must be 0");
  const Ctx& c = h->c;
  const int n = c.d.n;
  for (int64_t k = 0; k < n_blocks; ++k) {
    const int64_t len = block_offsets[k + 1] - block_offsets[k];
    if (len < 1) return fail(fn + ": 'block_offsets' must increase: block " + std::to_string(k) + " is empty");
    if (len > LP_ROWS) return fail(fn + ": block " + std::to_string(k) + " has " + std::to_string(len) + " observations, above 64");
    if (block_curve[k] < 0 || block_curve[k] >= n)
      return fail(fn + ": 'block_curve'[" + std::to_string(k) + "] = " + std::to_string(block_curve[k]) + " outside 0 .. " + std::to_string(n - 1));
  }
  const int64_t total = block_offsets[n_blocks];
  if (block_capacity < n_blocks) return fail(fn + ": 'block_capacity' below " + std::to_string(n_blocks) + " blocks");
  if (row_capacity < total) return fail(fn + ": 'row_capacity' below " + std::to_string(total) + " rows");
  if (ck.range() || ck.budget_sign(max_workspace_bytes) || ck.row_limit()) return 1;
  const std::string bad = loo_blocks_check(c);
  if (!bad.empty()) return fail(fn + ": " + bad);
  HIPCHK(hipSetDevice(h->device));
  DenseBasis basis(h);
  if (basis.counts()) return 1;
  // the indices of every block, then the tiles and the rows of the whole list
  struct Tile { LbTile t; int64_t blk0, blk1; };
  std::vector<Tile> tiles;
  std::vector<LbRow> rows_all((size_t)total);
  {
    std::vector<int64_t> seen;                      // per observation of the block's curve: the last block that listed it, plus one
    int seen_curve = -1;
    for (int64_t k = 0; k < n_blocks; ++k) {
      const int i = block_curve[k], ni = basis.ni[i];
      const int64_t j0 = block_offsets[k], len = block_offsets[k + 1] - j0;
      if (seen_curve != i) { seen.assign((size_t)ni, 0); seen_curve = i; }
      for (int64_t j = j0; j < j0 + len; ++j) {
        const int o = block_obs[j];
        if (o < 0 || o >= ni)
          return fail(fn + ": 'block_obs'[" + std::to_string(j) + "] = " + std::to_string(o) + " outside 0 .. " + std::to_string(ni - 1) +
                      " (block " + std::to_string(k) + " of curve " + std::to_string(i) + ")");
        if (seen[(size_t)o] == k + 1) return fail(fn + ": 'block_obs'[" + std::to_string(j) + "] = " + std::to_string(o) + " is repeated in block " + std::to_string(k));
        seen[(size_t)o] = k + 1;
      }
      if (tiles.empty() || tiles.back().t.curve != i || tiles.back().t.rows + len > LP_ROWS) tiles.push_back({{i, 0, basis.off[i], j0}, k, k});
      Tile& tl = tiles.back();
      for (int64_t j = j0; j < j0 + len; ++j)
        rows_all[(size_t)j] = {basis.off[i] + block_obs[j], block_obs[j], (int16_t)tl.t.rows, (int16_t)len};
      tl.t.rows += (int32_t)len;
      tl.blk1 = k + 1;
    }
  }
  const size_t N = (size_t)ck.CS();
  // a tile: its rows of the four matrices, the nine results a row, its entry of the list, its rows of the table and what DenseBasis takes
  const size_t per_tile = sizeof(double) * (size_t)LP_ROWS * (4 * N + 9) + basis.tile_bytes() + sizeof(LbTile) + sizeof(LbRow) * (size_t)LP_ROWS;
  int64_t chunk = 0;
  if (ck.units(budget_of(max_workspace_bytes), basis.shared_bytes(), per_tile, (int64_t)tiles.size(), (int64_t)1 << 24, "tile", &chunk)) return 1;
  reset_timers(h, PT_LOO_BLOCKS, PT_LOO_BLOCKS_PSIS);
  CallBufs b;
  double* d_x = nullptr;
  LbTile* d_tiles = nullptr;
  LbRow* d_rows = nullptr;
  Timer kern, vark, psis;
  HIPCHK(b.timers({&kern, &vark, &psis}));
  const size_t stride = (size_t)chunk * LP_ROWS * N;
  HIPCHK(b.get(&d_x, 4 * stride));
  HIPCHK(b.get(&d_tiles, (size_t)chunk));
  HIPCHK(b.get(&d_rows, (size_t)chunk * LP_ROWS));
  if (basis.prepare(ck, b, chunk, PT_LOO_BLOCKS)) return 1;
  std::vector<LbTile> ht((size_t)chunk);
  std::vector<double> hexp, hpw, hll;
  return for_chunks(ck, (int64_t)tiles.size(), chunk, [&](int64_t p0, int cnt) {
    const int64_t base = tiles[(size_t)p0].t.row0;
    const int64_t blk0 = tiles[(size_t)p0].blk0, blk1 = tiles[(size_t)p0 + cnt - 1].blk1;
    int64_t rows64 = 0;
    for (int q = 0; q < cnt; ++q) {
      LbTile t = tiles[(size_t)p0 + q].t;
      t.row0 -= base;
      ht[(size_t)q] = t;
      rows64 = t.row0 + t.rows;
    }
    const int rows = (int)rows64;
    std::vector<LbRow> hr(rows_all.begin() + (size_t)base, rows_all.begin() + (size_t)(base + rows));
    for (int r = 0; r < rows; ++r) {
      basis.stage(hr[(size_t)r].b, 1, r);                // the observation's row of the handle's host basis
      if (basis.from_basis) hr[(size_t)r].b = r;
    }
    if (copy_sync(h, d_tiles, ht.data(), sizeof(LbTile) * (size_t)cnt, hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(h, d_rows, hr.data(), sizeof(LbRow) * (size_t)rows, hipMemcpyHostToDevice) != hipSuccess || !basis.upload(rows))
      return std::string(kBackFailed);
    std::string err = timed(kern, h->st, [&] {
      return launch_loo_blocks(c, d_tiles, cnt, d_rows, basis.d_B, h->d_y, first_slot, n_slots, d_x, stride, h->st);
    });
    if (err.empty() && loglik_trace) {
      hll.resize((size_t)rows * N);
      err = Back{h, 0, rows}(hll.data(), (const double*)d_x, N).queued();
    }
    if (err.empty())
      err = Back{h, base, rows}(pit_trace, (const double*)(d_x + stride), N)(mean_trace, (const double*)(d_x + 2 * stride), N).done();
    if (err.empty() && hipGetLastError() != hipSuccess) err = kBackFailed;
    if (!err.empty()) return err;
    collect(h, kern, PT_LOO_BLOCKS);
    if (loglik_trace)
      for (int64_t k = blk0; k < blk1; ++k)
        std::copy(hll.begin() + (size_t)(block_offsets[k] - base) * N, hll.begin() + (size_t)(block_offsets[k] - base + 1) * N, loglik_trace + (size_t)k * N);
    // PSIS row by row, then the six results of each block's first row
    hpw.resize(6 * (size_t)rows);
    double* const pw[6] = {hpw.data(), hpw.data() + rows, hpw.data() + 2 * (size_t)rows, hpw.data() + 3 * (size_t)rows,
                           hpw.data() + 4 * (size_t)rows, hpw.data() + 5 * (size_t)rows};
    hexp.resize(3 * (size_t)rows);
    err = psis_step(h, d_x, N, rows, pw, 0, &psis, PT_LOO_BLOCKS_PSIS, d_x + stride, 3, stride, hexp.data());
    if (!err.empty()) return err;
    for (int64_t k = blk0; k < blk1; ++k)
      for (int v = 0; v < 6; ++v) res[v][k] = pw[v][block_offsets[k] - base];
    return row_chunk_end(h, hexp, base, rows, pit, mean, sd, d_x, stride, N, var_trace, vark, PT_LOO_BLOCKS);
  });
}
