// What the two files of chain-slot entry points share (capi_chain.hip, what is read off the chain slots after a run, and
// capi_loo.hip, the PSIS-LOO family over them): an entry point is its argument checks (SlotCheck: slots, curve selection, the grid
// pair, x, alpha, probs and `units`, the one budget rule), its workspace and the event pairs that time its launches into the
// handle's PT_* timers (CallBufs owns both) and one for_chunks.  What several of them do is written once: `once` for a launch that
// runs once per call (the projections), Back for a chunk's copies to the host.
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
    const int D = h->c.d.D;
    if (x && !(h->c.covariance_adj && D > 0)) return fail(fn + ": 'x' is given but the sampler is not covariance-adjusted");
    for (int d = 0; x && d < D; ++d)
      if (!std::isfinite(x[d])) return fail(fn + ": 'x'[" + std::to_string(d) + "] is not finite");
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

}  // namespace
