// What the three files of chain-slot entry points share (capi_chain.hip, what is read off the chain slots after a run,
// capi_cluster.hip, the cluster-level calls under aligned or rescaled labels, and capi_loo.hip, the PSIS-LOO family): an entry
// point is its argument checks (SlotCheck: slots, curve selection, the grid pair, x, perm, alpha, probs and `units`, the one budget
// rule), its workspace and the event pairs that time its launches into the handle's PT_* timers (CallBufs owns both) and one
// for_chunks.  What several of them do is written once: `once` for a launch that runs once per call (the projections), Back for a
// chunk's copies to the host, chain_array for the layout of a chain array, SortWs for the rule that long rows sort in a workspace,
// RowReducer for a chunk of rows of C S pooled values (its layout in one allocation, its reduction and its copies back) and
// RowCall for a call that is such rows and nothing else.
#pragma once
#include "handle.hpp"
#include "launchers.hpp"
#include "../../include/bfmmm_entry.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <utility>

using namespace bfmmm;

namespace {      // internal to each including file: the library exports nothing from here

// ---- argument checks ----------------------------------------------------------------------------------------------------
// The checks of a call over slots [first_slot, first_slot + n_slots) of every chain, each answering 0 or fail() with the entry
// point's name in front; an entry point chains them with || in the order of its messages.  ptrs() first: the others read h.
struct SlotCheck {
  std::string fn;
  bfmmm_handle* h;
  int first_slot, n_slots;
  std::string tag = "";      // bfmmm_chain_diagnostics: "(name)", shown by capacity() and the chunk loop's failure

  long long CS() const { return (long long)h->nch * n_slots; }      // draws per row
  int ptrs(std::initializer_list<std::pair<const char*, const void*>> l) const {
    for (const auto& e : l)
      if (!e.second) return fail(fn + ": '" + e.first + "' is null");
    return 0;
  }
  int range() const {
    if (first_slot < 0 || first_slot >= h->T) return fail(fn + ": 'first_slot' out of range");
    if (n_slots < 1 || n_slots > h->T - first_slot) return fail(fn + ": 'n_slots' out of range (first_slot + n_slots > T)");
    return 0;
  }
  int row_limit() const { return row_limit(CS(), "n_chains x n_slots"); }
  int row_limit(long long draws, const char* what) const {      // a call whose rows are not the pooled n_chains x n_slots draws
    if (draws <= diag_row_max()) return 0;
    return fail(fn + ": at most 4194304 (2^22) draws per row (" + what + ") in this build, got " + std::to_string(draws));
  }
  int budget_sign(int64_t bytes) const { return bytes < 0 ? fail(fn + ": 'max_workspace_bytes' must not be negative") : 0; }
  // The budget rule: a workspace of `shared` bytes for the whole call and `per_unit` for every unit (noun: "curve", "block", "row")
  // of a chunk; *chunk units fit the budget, at most `count` and `cap`.  No noun: rows with nothing shared.  per_unit 0: nothing
  // to chunk, the shared part alone has to fit.
  int units(size_t budget, size_t shared, size_t per_unit, int64_t count, int64_t cap, const char* noun, int64_t* chunk) const {
    if (budget < shared + per_unit) {
      const std::string need = fn + ": 'max_workspace_bytes' below the " + std::to_string(shared + per_unit) + " bytes ";
      return fail(noun ? need + "one " + noun + " needs " + plan_text(shared, per_unit, noun) : need + "of one row");
    }
    *chunk = per_unit ? std::min<int64_t>(std::min<int64_t>(count, (int64_t)((budget - shared) / per_unit)), cap) : 1;
    return 0;
  }
  static std::string plan_text(size_t shared, size_t per_unit, const std::string& noun) {
    return "(" + std::to_string(shared) + " shared by all " + noun + "s + " + std::to_string(per_unit) + " per " + noun + ")";
  }
  int capacity(int64_t have, int64_t want, const char* unit = "entries") const { return have < want ? fail(fn + tag + ": 'capacity' below " + std::to_string(want) + " " + unit) : 0; }
  // a selection of curves (null: all n): every index is one; *m: the curves of the result.  The caller checks n_curves by its own rule.
  int curve_list(const int32_t* curves, int n_curves, int64_t* m) const {
    const int n = h->c.d.n;
    for (int j = 0; curves && j < n_curves; ++j)
      if (curves[j] < 0 || curves[j] >= n)
        return fail(fn + ": 'curves'[" + std::to_string(j) + "] = " + std::to_string(curves[j]) + " outside 0 .. " + std::to_string(n - 1));
    *m = curves ? n_curves : n;
    return 0;
  }
  // the grid pair of a covariance surface: E1 of G1 rows, E2 of G2 rows where given, `diagonal` only without E2
  int grid_pair(int G1, const double* E2, int G2, int diagonal) const {
    if (G1 < 1) return fail(fn + ": 'G1' must be at least 1");
    if (E2 && G2 < 1) return fail(fn + ": 'G2' must be at least 1 where 'E2' is given");
    if (diagonal && E2) return fail(fn + ": 'diagonal' requires 'E2' to be null");
    return 0;
  }
  // a covariate setting x (null: none) of D finite entries, for covariance-adjusted samplers only
  int covariate_setting(const double* x) const {
    if (x && !(h->c.covariance_adj && h->c.d.D > 0)) return fail(fn + ": 'x' is given but the sampler is not covariance-adjusted");
    return x_finite(x);
  }
  int x_finite(const double* x) const {
    for (int d = 0; x && d < h->c.d.D; ++d)
      if (!std::isfinite(x[d])) return fail(fn + ": 'x'[" + std::to_string(d) + "] is not finite");
    return 0;
  }
  // an argument `what` (null: not given) that only a sampler with covariates takes, at most 8 of them
  int covariates(const char* what, const void* given) const {
    if (!given) return 0;
    if (!(h->c.d.D > 0 && h->c.c_eta)) return fail(fn + ": '" + what + "' is given but the sampler has no covariates");
    return h->c.d.D > 8 ? fail(fn + ": more than 8 covariates") : 0;
  }
  // every row perm[(q S + s) K + .] a permutation of 0 .. K - 1, or fail() naming the first draw that is not
  int perm_check(const int32_t* perm) const {
    const int K = h->c.d.K, S = n_slots;
    for (long long o = 0; o < CS(); ++o) {
      unsigned seen = 0;
      for (int l = 0; l < K; ++l) {
        const int32_t v = perm[o * K + l];
        if (v < 0 || v >= K || (seen >> v & 1u))
          return fail(fn + ": 'perm' of chain " + std::to_string(o / S) + ", slot " + std::to_string(first_slot + o % S) +
                      " is not a permutation of 0 .. " + std::to_string(K - 1));
        seen |= 1u << v;
      }
    }
    return 0;
  }
  int alpha_inside(double alpha) const { return alpha > 0.0 && alpha < 1.0 ? 0 : fail(fn + ": 'alpha' must be inside (0, 1)"); }
  // nq in nq_min .. 16, with probs inside [0, 1] and somewhere to put the quantiles where nq > 0
  int probs_list(const double* probs, int nq, int nq_min, const double* quant) const {
    if (nq < nq_min || nq > 16) return fail(fn + ": 'nq' outside " + std::to_string(nq_min) + " .. 16");
    if (nq > 0 && ptrs({{"probs", probs}, {"quant", quant}})) return 1;
    for (int q = 0; q < nq; ++q)
      if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return fail(fn + ": 'probs'[" + std::to_string(q) + "] outside [0, 1]");
    return 0;
  }
};
constexpr int64_t kNoCap = INT64_MAX;      // SlotCheck::units without a cap of the call's own
// the cap of a call whose kernels index 2^30 result entries of `cells` a curve
int64_t cells_cap(int64_t cells) { return std::max<int64_t>(1, (1LL << 30) / cells); }
size_t budget_of(int64_t max_workspace_bytes) { return max_workspace_bytes ? (size_t)max_workspace_bytes : (size_t)256 << 20; }

// ---- what a call owns, its chunk loop and its timing ----------------------------------------------------------------------
// A pair of events around a launch, or a sequence of launches, of a call.
struct Timer { hipEvent_t from = nullptr, to = nullptr; };

// The device buffers and events of one call: released when the call returns, whichever way.
struct CallBufs {
  std::vector<void*> p;
  std::vector<hipEvent_t> ev;
  ~CallBufs() {
    for (void* q : p) (void)hipFree(q);
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  template <typename T>
  hipError_t get(T** out, size_t count) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
    return e;
  }
  // a device copy of the `count` elements at src
  template <typename T>
  hipError_t put(bfmmm_handle* h, T** out, const T* src, size_t count) {
    const hipError_t e = get(out, count);
    return e != hipSuccess ? e : copy_sync(h, *out, src, sizeof(T) * count, hipMemcpyHostToDevice);
  }
  hipError_t timers(std::initializer_list<Timer*> l) {
    for (Timer* t : l)
      for (hipEvent_t* e : {&t->from, &t->to}) {
        const hipError_t err = hipEventCreate(e);
        if (err != hipSuccess) return err;
        ev.push_back(*e);
      }
    return hipSuccess;
  }
};

// Rows [0, len) in chunks of `chunk`: body(p0, rows) launches, copies back and collects the times of one chunk and answers
// "" or what failed, which ends the loop.  Then the stream is drained and a failure reported under the call's name.
template <typename Body>
int for_chunks(const SlotCheck& ck, int64_t len, int64_t chunk, Body body) {
  std::string err;
  for (int64_t p0 = 0; p0 < len && err.empty(); p0 += chunk) err = body(p0, (int)std::min<int64_t>(chunk, len - p0));
  (void)hipStreamSynchronize(ck.h->st);
  if (!err.empty()) { (void)hipGetLastError(); return fail(ck.fn + ck.tag + ": " + err); }
  return 0;
}

// launch(), which answers "" or what failed, between the events of t on the stream; once the stream has been synchronised,
// collect adds the device time between them to timer pt of the handle (handle.hpp) and counts it
template <typename Launch>
std::string timed(const Timer& t, hipStream_t st, Launch launch) {
  (void)hipEventRecord(t.from, st);
  const std::string err = launch();
  (void)hipEventRecord(t.to, st);
  return err;
}
void collect(bfmmm_handle* h, const Timer& t, int pt) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, t.from, t.to) != hipSuccess) { (void)hipGetLastError(); return; }
  h->post_ms[pt] += ms;
  h->post_launches[pt] += 1;
}
void reset_timers(bfmmm_handle* h, int first, int last) {
  for (int pt = first; pt <= last; ++pt) { h->post_ms[pt] = 0; h->post_launches[pt] = 0; }
}

// one launch of k_chain_curve_ll between the handle's two events; curve_ll_collect adds its device time after a synchronise
std::string curve_ll_timed(const SlotCheck& ck, int i0, int rows, double* d_x) {
  bfmmm_handle* h = ck.h;
  return timed({h->ev0, h->ev1}, h->st, [&] { return launch_chain_curve_ll(h->c, ck.first_slot, ck.n_slots, i0, rows, d_x, h->st); });
}
void curve_ll_collect(bfmmm_handle* h) { collect(h, {h->ev0, h->ev1}, PT_CURVE_LL); }

// A launch that runs once per call (the projection tables), between an event pair of its own: launch, synchronise, a failure
// under the call's name, the device time into timer pt.  count > 0: the timer reports that (the tables filled), not the launch.
template <typename Launch>
int once(const SlotCheck& ck, CallBufs& b, int pt, int count, Launch launch) {
  bfmmm_handle* h = ck.h;
  Timer t;
  HIPCHK(b.timers({&t}));
  const std::string err = timed(t, h->st, launch);
  if (!err.empty()) { (void)hipStreamSynchronize(h->st); return fail(ck.fn + ": " + err); }
  HIPCHK(hipStreamSynchronize(h->st));
  collect(h, t, pt);
  if (count) h->post_launches[pt] = count;
  return 0;
}

// The copies of a chunk to the host: back(dst, src, per_row) queues rows [r0, r0 + rows) of per_row entries each from the chunk's
// device buffer src to dst + r0 per_row (dst null: not asked for, skipped); done() synchronises the stream and answers "" or what
// a body of for_chunks reports.
constexpr const char* kBackFailed = "kernel or copy back failed";
struct Back {
  bfmmm_handle* h;
  int64_t r0;
  int rows;
  bool ok = true;
  template <typename T>
  Back& operator()(T* dst, const T* src, size_t per_row) {
    if (ok && dst)
      ok = hipMemcpyAsync(dst + (size_t)r0 * per_row, src, sizeof(T) * (size_t)rows * per_row, hipMemcpyDeviceToHost, h->st) == hipSuccess;
    return *this;
  }
  std::string done() const { return ok && hipStreamSynchronize(h->st) == hipSuccess ? "" : kBackFailed; }
  std::string queued() const { return ok ? "" : kBackFailed; }      // more copies of the chunk follow: their done() synchronises
};

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

// A call that is `len` rows and their reduction (split R-hat, ESS and MCSE of the chain arrays and of the per-curve log-density,
// DESIGN.md 7c; the cluster summaries, mean functions and eigenfunctions of capi_cluster.hip), in two steps, since what a call puts
// on the device comes after the refusal of its budget.  plan(): the budget rule (`shared` bytes for the whole call, a row of the
// reducer for every row of a chunk, at most `cap` rows; SlotCheck::units), the device, the chunk's workspace and the probabilities.
// run(): per chunk, fill(r0, rows, d_x) puts rows [r0, r0 + rows) into the workspace (row-major: draw fastest, then chain), the
// reducer reduces them and outs (mean and sd, or the seven statistics), quant and trace go to the host (null: not asked for).
// pt >= 0: timer pt of the handle starts from zero, fill runs between a pair of events and the timer collects their device time
// chunk by chunk.
struct RowCall {
  const SlotCheck& ck;
  int64_t len;
  RowReducer r;
  CallBufs b;      // owns the workspace; what the caller's kernels read goes here too
  int64_t chunk = 0;
  int pt;

  RowCall(const SlotCheck& ck, int64_t len, int nq, bool seven, int pt) : ck(ck), len(len), r(ck, nq, seven), pt(pt) {}
  int plan(int64_t max_workspace_bytes, size_t shared, int64_t cap, const char* noun, const double* probs) {
    if (ck.units(budget_of(max_workspace_bytes), shared, len > 0 ? r.row_bytes() : 0, len, cap, noun, &chunk)) return 1;
    HIPCHK(hipSetDevice(ck.h->device));
    if (pt >= 0) reset_timers(ck.h, pt, pt);
    if (len > 0) HIPCHK(r.alloc(b, chunk));
    double* d_probs = nullptr;
    if (r.nq) HIPCHK(probs_put(b, ck.h, probs, r.nq, &d_probs));
    r.probs = d_probs;
    return 0;
  }
  template <typename Fill>
  int run(double* const* outs, double* quant, double* trace, Fill fill) {
    bfmmm_handle* h = ck.h;
    Timer t;
    if (pt >= 0) HIPCHK(b.timers({&t}));
    return for_chunks(ck, len, chunk, [&](int64_t r0, int rows) {
      std::string err = pt >= 0 ? timed(t, h->st, [&] { return fill(r0, rows, r.x); }) : fill(r0, rows, r.x);
      if (err.empty()) err = r.reduce(rows);
      if (err.empty()) err = r.to_host(r0, rows, outs, quant, trace);
      if (err.empty() && pt >= 0) collect(h, t, pt);
      return err;
    });
  }
};

}  // namespace
