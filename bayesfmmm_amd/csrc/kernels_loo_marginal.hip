// The refinement of the marginal PSIS-LOO over curves (bfmmm_chain_loo_marginal).  The first pass of that call is
// k_predict on the resident records of the training curves: per (curve i, chain q, slot t) the staged importance-sampling estimate
// of log p(y_i | draw) with the memberships integrated out, its ess and the proposal a_last of its last stage.  A pair whose
// estimate cannot be trusted gets the largest importance ratio 1 / p of its curve in the LOO, so such pairs are run once more:
//   selected:   ess_t < ess_floor, or lpd_t not finite                                    (lz_selected, the one rule of this file)
//   k_lz_count  one workgroup per curve row of the chunk: the number of selected pairs and, where asked for, the mean and the
//               least ess of the row (the call runs it before the refinement for the list and after it for what it reports)
//   (the host copies `rows` counts and forms their exclusive prefix)
//   k_lz_list   one workgroup per row writes its selected pairs (curve, chain, slot) in increasing cs at the row's offset: a
//               ballot and a popcount per wave, the four waves in order, no atomics -- the list is the same on every call
//   k_lz_refine one workgroup of 256 threads per listed pair: pred_setup and pred_draw<KT, true> of predict_core.hpp with J2
//               samples in each of R2 stages, stage 0 proposing from a_last, so the Dirichlet correction
//               sum_k (alpha_3 pi_k - a_k) log z_k + lB(a) - lB(alpha_3 pi) applies from stage 0 on (zero where a is the prior);
//               variates under UPD_LOO_REFINE with index ((i R2 + st) J2 + j) K + k, i the curve's index in the data.  It
//               overwrites the pair's lpd_t and ess_t in place, once: there is no loop until the floor is met.
// fp64, vector stores only, no atomics; every sum in the order of predict_core.hpp.  A value's bits depend on (curve, chain, slot,
// seed, J, R, J2, R2, ess_floor) alone, not on the chunk, the grid or a repeated call.
#include "model.hpp"
#include "launchers.hpp"
#include "predict_core.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

__device__ inline bool lz_selected(double lpd, double ess, double ess_floor) { return ess < ess_floor || !(fabs(lpd) < INFINITY); }

__global__ __launch_bounds__(PR_NT) void k_lz_count(long long N, const double* lpd_t, const double* ess_t, double ess_floor, int32_t* cnt,
                                                    double* ess_mean, double* ess_min) {
  __shared__ double sRed[4 * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const double* lp = lpd_t + r * (size_t)N;
  const double* es = ess_t + r * (size_t)N;
  double v[2] = {0.0, 0.0}, mn = INFINITY;      // (a count below 2^22 is exact in a double)
  for (long long o = tid; o < N; o += PR_NT) {
    const double e = es[o];
    v[0] += lz_selected(lp[o], e, ess_floor) ? 1.0 : 0.0;
    v[1] += e;
    mn = fmin(mn, e);
  }
  block_sum<2>(v, sRed, lane, wave);
  mn = block_extreme<false>(mn, sRed, lane, wave);
  if (tid == 0) {
    cnt[r] = (int32_t)v[0];
    if (ess_mean) ess_mean[r] = v[1] / (double)N;
    if (ess_min) ess_min[r] = mn;
  }
}

// n_list: the entries the list holds, the sum of the counts (a bound, not a part of the result)
__global__ __launch_bounds__(PR_NT) void k_lz_list(long long N, int S, int r0, const double* lpd_t, const double* ess_t, double ess_floor,
                                                   const int64_t* off, long long n_list, int32_t* list) {
  __shared__ int sCnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const double* lp = lpd_t + r * (size_t)N;
  const double* es = ess_t + r * (size_t)N;
  long long base = off[r];
  for (long long o0 = 0; o0 < N; o0 += PR_NT) {
    const long long o = o0 + tid;
    const bool sel = o < N && lz_selected(lp[o], es[o], ess_floor);
    const unsigned long long m = __ballot(sel);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) sCnt[wave] = __popcll(m);
    __syncthreads();
    int wb = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = sCnt[w];
      wb += w < wave ? c : 0;
      tot += c;
    }
    const long long e = base + wb + before;
    if (sel && e < n_list) {
      int32_t* p = list + 3 * e;
      p[0] = r0 + (int)r;
      p[1] = (int)(o / S);
      p[2] = (int)(o - (o / S) * S);
    }
    base += tot;
    __syncthreads();
  }
}

template <int KT>
__global__ __launch_bounds__(PR_NT) void k_lz_refine(PredArgs a, const int32_t* list) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const PredLds L = pred_lds(a.K, a.P, a.M, a.LG, a.J, KT);
  const size_t e = blockIdx.x;                     // the pair's place in the chunk's list
  const int r = list[3 * e], q_chain = list[3 * e + 1], s = list[3 * e + 2];
  const PredSlots ch = pred_slots(a, q_chain);
  double yy;
  int ni;
  pred_setup(a, L, sm, r, &yy, &ni);
  pred_draw<KT, true>(a, L, sm, ch, r, r - a.r0, q_chain, s, yy, ni, e);
}

}  // namespace

std::string lz_check(const Ctx& c, int J2, int R2, size_t* lds_bytes) {
  const Dims& d = c.d;
  if (J2 < 1 || R2 < 1) return "k_lz_refine: fewer than 1 sample or stage";
  const PredLds L = pred_lds(d.K, d.P, d.M, d.LG, std::min(J2, 1 << 24), pred_kt(d.K));
  const size_t bytes = L.total * sizeof(double);
  if (lds_bytes) *lds_bytes = bytes;
  if (bytes > PR_LDS_HARD || J2 > (1 << 24))
    return "k_lz_refine: the tables of a draw (Gamma of " + std::to_string(L.AP) + " x " + std::to_string(L.AP) + ") and the " +
           std::to_string((long long)J2) + " x (K + 1) values of a refinement stage's samples ('refine_samples') need " +
           (J2 > (1 << 24) ? std::string("more than 1073741824") : std::to_string(bytes)) + " bytes of LDS, above the limit of " +
           std::to_string(PR_LDS_HARD) + " (160 KiB)";
  return "";
}

std::string launch_lz_count(long long N, int rows, const double* lpd_t, const double* ess_t, double ess_floor, int32_t* cnt, double* ess_mean,
                            double* ess_min, hipStream_t st) {
  if (N < 1 || rows < 1 || !lpd_t || !ess_t || !cnt) return "k_lz_count: bad shape";
  hipLaunchKernelGGL(k_lz_count, dim3((unsigned)rows), dim3(PR_NT), 0, st, N, lpd_t, ess_t, ess_floor, cnt, ess_mean, ess_min);
  if (hipGetLastError() != hipSuccess) return "k_lz_count: launch failed";
  return "";
}

std::string launch_lz_list(long long N, int S, int r0, int rows, const double* lpd_t, const double* ess_t, double ess_floor, const int64_t* off,
                           long long n_list, int32_t* list, hipStream_t st) {
  if (N < 1 || S < 1 || N % S != 0 || rows < 1 || r0 < 0 || n_list < 1 || !off || !list) return "k_lz_list: bad shape";
  hipLaunchKernelGGL(k_lz_list, dim3((unsigned)rows), dim3(PR_NT), 0, st, N, S, r0, lpd_t, ess_t, ess_floor, off, n_list, list);
  if (hipGetLastError() != hipSuccess) return "k_lz_list: launch failed";
  return "";
}

std::string launch_lz_refine(const Ctx& c, const PredictCall& f, int r0, int rows, const int32_t* list, long long n_list, double* lpd_t,
                             double* ess_t, const double* a_last, double* prop, double* samples, hipStream_t st) {
  size_t lds = 0;
  const std::string bad = lz_check(c, f.J, f.R, &lds);
  if (!bad.empty()) return bad;
  if (rows < 1 || r0 < 0 || (long long)r0 + rows > f.n_new) return "k_lz_refine: curves outside the call";
  if (n_list < 1 || n_list > 2147483647LL || !list || !a_last || !lpd_t || !ess_t) return "k_lz_refine: bad list";
  PredArgs a = pred_args(c, f, r0, rows, lpd_t, ess_t, nullptr, nullptr, prop, samples);
  a.a_start = a_last;
  void (*fn)(PredArgs, const int32_t*) = pred_kt(c.d.K) == 4 ? k_lz_refine<4> : k_lz_refine<KMAX>;
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_lz_refine: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)n_list), dim3(PR_NT), lds, st, a, list);
  if (hipGetLastError() != hipSuccess) return "k_lz_refine: launch failed";
  return "";
}

}  // namespace bfmmm
