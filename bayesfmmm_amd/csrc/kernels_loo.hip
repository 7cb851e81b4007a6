// Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO) and WAIC of every row of a pointwise log-likelihood matrix
// (include/bfmmm_post.h): row i = the log-density of curve i under each of S kept draws, draw fastest.  The procedure is
// psis() / gpdfit() of the R package loo with relative efficiency 1 (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson,
// Gelman, Yao & Gabry 2024), in the numbered steps DESIGN.md 7b states; everything in fp64.
//
// k_post_psis: one workgroup of 256 threads per row.  Every sum is a fixed-order reduction (thread-strided partials, then an
// LDS tree), the only atomics are integer ones (histogram counts, gather slots) and the gathered set is sorted by a unique
// key, so two calls give the same bits.
//   pass 1  min, max, sum of the row
//   pass 2  sum exp(l - max) (lppd), sum (l - mean)^2 (p_waic), 256-bin histogram of the first digit of the tail key
//   pass 3+ radix select of the (L + 1)-th largest composite key (the order-preserving 64-bit image of lw, then the draw
//           index: the stable sort's tie order), one 8-bit digit per pass over the entries that share the chosen prefix,
//           until the entries at or above the prefix fit the on-chip table (usually after one or two digits)
//   gather  those entries -> LDS, bitonic sort by (key, index): the tail is the last L, the cutoff the one before
//   fit     the generalized Pareto fit of the tail: the m <= 30 + sqrt(L) candidate thetas over lanes (a few lanes per
//           candidate, fixed segments), the weights and k in one thread / one reduction; the smoothed tail -> LDS
//   last    elpd_loo = logsumexp(lw + l) - logsumexp(lw): non-tail draws from the row, tail draws from the LDS table
// k_post_psis<NAUX>, NAUX > 0: the last pass also takes the expectation of NAUX auxiliary rows h_a (the layout and leading
// dimension of the log-likelihood matrix, aux_stride doubles from one matrix to the next) under the smoothed weights,
// E_a = sum_t exp(w_t - sh2) h_a(t) / s2, the terms in the order of s2.  NAUX = 0 is the kernel without them, bit for bit.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bfmmm_post.h"
#include "launchers.hpp"
#include "post_host.hpp"
#include "row_stats.hpp"

namespace {

using namespace rs;

constexpr int NT = 256;                        // threads per workgroup = histogram bins
constexpr int CAP_MAX = 8192;                  // largest on-chip table of gathered tail candidates
constexpr long long S_MAX = 1LL << 22;         // kept draws per row in this build (L <= 6144 < CAP_MAX)

constexpr int NAUX_MAX = 4;                    // auxiliary matrices of one launch (more: further launches)

struct PsisOut {
  double *lppd, *elpd_loo, *p_loo, *khat, *elpd_waic, *p_waic;
};
struct PsisAux {
  const double* h;       // matrix a at h + a * stride, row i at + i * ld
  long long stride;
  double* expect;        // E_a of row i at [a * n + i]
  int n;
};

// digit p (0..11) of the 96-bit composite (key, draw index), most significant first
__device__ inline unsigned digit(u64 key, unsigned idx, int p) {
  return p < 8 ? (unsigned)(key >> (56 - 8 * p)) & 255u : (idx >> (24 - 8 * (p - 8))) & 255u;
}

// histogram count with the adds of a wave's lanes that share a bin merged (a concentrated row puts most lanes in one bin)
__device__ inline void hist_add(unsigned* hist, unsigned d, bool on) {
  u64 pending = __ballot(on);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const unsigned dl = (unsigned)__shfl((int)d, leader);
    const u64 same = __ballot(on && d == dl) & pending;
    if ((int)__lane_id() == leader) atomicAdd(&hist[dl], (unsigned)__popcll(same));
    pending &= ~same;
  }
}

template <int NAUX>
__global__ __launch_bounds__(NT) void k_post_psis(const double* ll, long long ld, int S, int L, int cap, PsisOut o, PsisAux ax) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, i = blockIdx.x;
  double* red = sm;                                    // NT
  double* sTh = red + NT;                              // 2 x 128: candidate thetas and their profile log-likelihoods
  unsigned* hist = (unsigned*)(sTh + 256);             // NT
  unsigned* scan = hist + NT;                          // NT
  unsigned* sI = scan + NT;                            // 8: selected bin, its count, the count above it, gather slots
  u64* sKey = (u64*)(sI + 8);                          // cap (after the fit: e_j, then the smoothed tail, as doubles)
  unsigned* sIdx = (unsigned*)(sKey + cap);            // cap
  double* sE = (double*)sKey;
  const double* row = ll + (size_t)i * (size_t)ld;

  // ---- pass 1 ----
  double mx = -INFINITY, mn = INFINITY, sum = 0.0;
  for (int t = tid; t < S; t += NT) { const double x = row[t]; mx = fmax(mx, x); mn = fmin(mn, x); sum += x; }
  mx = block_reduce<NT>(mx, red, OpMax());
  mn = block_reduce<NT>(mn, red, OpMin());
  sum = block_reduce<NT>(sum, red, OpSum());
  const double mean = sum / (double)S;
  const double rmax = -mn;                             // max_t r_t, r_t = -l_t;  lw_t = r_t - rmax
  const bool select = L >= 5;

  // ---- pass 2 (+ the first digit's histogram) ----
  hist[tid] = 0;
  __syncthreads();
  double se = 0.0, sq = 0.0;
  for (int b = 0; b < S; b += NT) {
    const int t = b + tid;
    const bool on = t < S;
    const double x = on ? row[t] : mn;
    if (on) { se += exp(x - mx); const double d = x - mean; sq += d * d; }
    if (select) hist_add(hist, digit(okey(-x - rmax), (unsigned)t, 0), on);
  }
  se = block_reduce<NT>(se, red, OpSum());
  sq = block_reduce<NT>(sq, red, OpSum());
  const double lppd = mx + log(se) - log((double)S);
  const double p_waic = S > 1 ? sq / (double)(S - 1) : 0.0;

  double khat = INFINITY;
  bool smooth = false;
  int base = 0;                                        // sorted position of the first tail entry
  u64 kc = 0;                                          // composite of the cutoff
  unsigned ic = 0;
  double c = 0.0;
  if (select) {
    // ---- radix select: the entries at or above a prefix of the composite key, until they fit the table ----
    u64 kmask = 0, kval = 0;
    unsigned imask = 0, ival = 0, above = 0;
    for (int p = 0; p < 12; ++p) {
      if (p > 0) {
        __syncthreads();
        hist[tid] = 0;
        __syncthreads();
        for (int b = 0; b < S; b += NT) {
          const int t = b + tid;
          bool on = t < S;
          u64 key = 0;
          if (on) { key = okey(-row[t] - rmax); on = (key & kmask) == kval && ((unsigned)t & imask) == ival; }
          hist_add(hist, digit(key, (unsigned)t, p), on);
        }
      }
      __syncthreads();
      // inclusive suffix sums of the bins; the bin holding rank need = L + 1 - above from the top
      scan[tid] = hist[tid];
      __syncthreads();
      for (int off = 1; off < NT; off <<= 1) {
        const unsigned v = (tid + off < NT) ? scan[tid + off] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
      }
      const unsigned need = (unsigned)(L + 1) - above;
      if (scan[tid] >= need && scan[tid] - hist[tid] < need) { sI[0] = (unsigned)tid; sI[1] = hist[tid]; sI[2] = scan[tid] - hist[tid]; }
      __syncthreads();
      const unsigned sel = sI[0], inbin = sI[1];
      above += sI[2];
      if (p < 8) { kmask |= 255ULL << (56 - 8 * p); kval |= (u64)sel << (56 - 8 * p); }
      else { imask |= 255u << (24 - 8 * (p - 8)); ival |= sel << (24 - 8 * (p - 8)); }
      if (above + inbin <= (unsigned)cap) break;
    }
    // ---- gather every entry at or above the prefix, sort by (key, index) ----
    if (tid == 0) sI[3] = 0;
    __syncthreads();
    for (int t = tid; t < S; t += NT) {
      const u64 key = okey(-row[t] - rmax), km = key & kmask;
      if (km > kval || (km == kval && ((unsigned)t & imask) >= ival)) {
        const unsigned s = atomicAdd(&sI[3], 1u);
        if (s < (unsigned)cap) { sKey[s] = key; sIdx[s] = (unsigned)t; }      // s < cap by the selection; kept in bounds regardless
      }
    }
    __syncthreads();
    const int G = min((int)sI[3], cap);
    const int npow = pow2_ceil(G);
    for (int e = G + tid; e < npow; e += NT) { sKey[e] = 0; sIdx[e] = 0; }      // below every finite key
    __syncthreads();
    bitonic_sort<NT>(KeyIdxRows{sKey, sIdx}, 1, npow);
    base = npow - L;
    kc = sKey[base - 1];
    ic = sIdx[base - 1];
    c = key_value(kc);
    const double x1 = key_value(sKey[base]), xL = key_value(sKey[npow - 1]);
    __syncthreads();
    if (!(xL - x1 < DBL_EPSILON / 100)) {
      // ---- generalized Pareto fit of e_j = exp(x_j) - exp(c), ascending, N = L ----
      const double ec = exp(c);
      for (int j = tid; j < L; j += NT) sE[base + j] = exp(key_value(sKey[base + j])) - ec;     // in place, own entries
      __syncthreads();
      const double* e = sE + base;
      const int N = L;
      const int m = 30 + (int)floor(sqrt((double)N));
      const double xstar = e[(int)floor(N / 4.0 + 0.5) - 1], eN = e[N - 1];
      const int nseg = max(1, NT / m);
      {
        const int j = tid / nseg, s = tid - j * nseg;
        double part = 0.0;
        if (j < m) {
          const double th = 1.0 / eN + (1.0 - sqrt((double)m / ((j + 1) - 0.5))) / (3.0 * xstar);
          const int l0 = (int)((long long)N * s / nseg), l1 = (int)((long long)N * (s + 1) / nseg);
          for (int l = l0; l < l1; ++l) part += log1p(-th * e[l]);
          if (s == 0) sTh[j] = th;
        }
        red[tid] = part;
      }
      __syncthreads();
      if (tid < m) {
        double kap = 0.0;
        for (int s = 0; s < nseg; ++s) kap += red[tid * nseg + s];
        kap /= (double)N;
        sTh[128 + tid] = (double)N * (log(-sTh[tid] / kap) - kap - 1.0);
      }
      __syncthreads();
      if (tid == 0) {
        double lmax = -INFINITY;
        for (int j = 0; j < m; ++j) { const double v = sTh[128 + j]; lmax = (isnan(lmax) || isnan(v)) ? NAN : fmax(lmax, v); }
        double z = 0.0;
        for (int j = 0; j < m; ++j) z += exp(sTh[128 + j] - lmax);
        const double lse = lmax + log(z);
        double th = 0.0;
        for (int j = 0; j < m; ++j) th += exp(sTh[128 + j] - lse) * sTh[j];
        red[NT - 1] = th;      // handed over through the reduction scratch (read before its next use)
      }
      __syncthreads();
      const double that = red[NT - 1];
      __syncthreads();
      double kp = 0.0;
      for (int l = tid; l < N; l += NT) kp += log1p(-that * e[l]);
      const double kk = block_reduce<NT>(kp, red, OpSum()) / (double)N;
      const double sigma = -kk / that;
      khat = ((double)N * kk + 5.0) / ((double)N + 10.0);
      if (isnan(khat)) khat = INFINITY;
      if (isfinite(khat)) {
        smooth = true;
        for (int j = tid; j < L; j += NT) {
          const double pj = (j + 0.5) / (double)L;
          sE[base + j] = log(sigma * expm1(-khat * log1p(-pj)) / khat + ec);
        }
      }
      __syncthreads();
    }
  }

  // ---- last pass: logsumexp(lw + l) - logsumexp(lw), lw <- min(lw, 0) ----
  double sh1 = mn, sh2 = 0.0;
  if (smooth) {
    double a1 = -INFINITY, a2 = -INFINITY;
    for (int j = tid; j < L; j += NT) {
      const double w = fmin(sE[base + j], 0.0);
      a1 = fmax(a1, w + row[sIdx[base + j]]);
      a2 = fmax(a2, w);
    }
    sh1 = fmax(mn, block_reduce<NT>(a1, red, OpMax()));
    sh2 = fmax(c, block_reduce<NT>(a2, red, OpMax()));
  }
  double s1 = 0.0, s2 = 0.0;
  double sa[NAUX > 0 ? NAUX : 1] = {};
  const double* hrow = NAUX > 0 ? ax.h + (size_t)i * (size_t)ld : nullptr;
  for (int t = tid; t < S; t += NT) {
    const double x = row[t], lw = -x - rmax;
    if (smooth) {
      const u64 key = okey(lw);
      if (key > kc || (key == kc && (unsigned)t > ic)) continue;     // a tail draw: taken from the table below
    }
    const double w = fmin(lw, 0.0);
    s1 += exp(w + x - sh1);
    const double e2 = exp(w - sh2);
    s2 += e2;
    if constexpr (NAUX > 0) {
#pragma unroll
      for (int a = 0; a < NAUX; ++a) sa[a] += e2 * hrow[(size_t)a * (size_t)ax.stride + t];
    }
  }
  if (smooth)
    for (int j = tid; j < L; j += NT) {
      const double w = fmin(sE[base + j], 0.0);
      s1 += exp(w + row[sIdx[base + j]] - sh1);
      const double e2 = exp(w - sh2);
      s2 += e2;
      if constexpr (NAUX > 0) {
#pragma unroll
        for (int a = 0; a < NAUX; ++a) sa[a] += e2 * hrow[(size_t)a * (size_t)ax.stride + sIdx[base + j]];
      }
    }
  s1 = block_reduce<NT>(s1, red, OpSum());
  s2 = block_reduce<NT>(s2, red, OpSum());
  if constexpr (NAUX > 0) {
#pragma unroll
    for (int a = 0; a < NAUX; ++a) {
      const double v = block_reduce<NT>(sa[a], red, OpSum());
      if (tid == 0) ax.expect[(size_t)a * ax.n + i] = v / s2;
    }
  }
  if (tid == 0) {
    const double elpd = (sh1 + log(s1)) - (sh2 + log(s2));
    o.lppd[i] = lppd;
    o.elpd_loo[i] = elpd;
    o.p_loo[i] = lppd - elpd;
    o.khat[i] = khat;
    o.elpd_waic[i] = lppd - p_waic;
    o.p_waic[i] = p_waic;
  }
}

}  // namespace

namespace {

using PsisKernel = void (*)(const double*, long long, int, int, int, PsisOut, PsisAux);
PsisKernel psis_pick(int n_aux) {
  switch (n_aux) {
    case 0: return k_post_psis<0>;
    case 1: return k_post_psis<1>;
    case 2: return k_post_psis<2>;
    case 3: return k_post_psis<3>;
    default: return k_post_psis<4>;
  }
}

// one launch per group of up to NAUX_MAX auxiliary matrices (one without any); the six arrays of every launch are the same
int psis_run(const char* who, const double* d_ll, long long ld, int n, int S, const double* d_aux, int n_aux, long long aux_stride,
             double* const out[6], double* expect_host) {
  const std::string fn(who);
  if (S > S_MAX) return bfmmm_io_fail(fn + ": at most 4194304 (2^22) kept draws per curve in this build, got " + std::to_string(S));
  const int L = (int)std::ceil(std::min(0.2 * S, 3.0 * std::sqrt((double)S)));
  int cap = 256;
  while (cap < 2 * (L + 1) && cap < CAP_MAX) cap <<= 1;
  DevBufs b;
  double* d_out;
  if (!b.put(&d_out, nullptr, (6 + (size_t)n_aux) * (size_t)n)) { (void)hipGetLastError(); return bfmmm_io_fail(fn + ": device allocation failed"); }
  PsisOut o{d_out, d_out + n, d_out + 2 * (size_t)n, d_out + 3 * (size_t)n, d_out + 4 * (size_t)n, d_out + 5 * (size_t)n};
  const size_t lds = (size_t)(NT + 256) * sizeof(double) + (size_t)(3 * NT + 8) * sizeof(unsigned) + (size_t)cap * (sizeof(u64) + sizeof(unsigned));
  float ms = 0.f;
  for (int a0 = 0; a0 == 0 || a0 < n_aux; a0 += NAUX_MAX) {
    const int na = std::min(NAUX_MAX, n_aux - a0);
    const PsisKernel fn_k = psis_pick(na);
    const PsisAux ax{na ? d_aux + (size_t)a0 * (size_t)aux_stride : nullptr, aux_stride, d_out + (6 + (size_t)a0) * (size_t)n, n};
    (void)hipFuncSetAttribute((const void*)fn_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (!timed_launch([&] { hipLaunchKernelGGL(fn_k, dim3(n), dim3(NT), lds, 0, d_ll, ld, S, L, cap, o, ax); return true; }))
      return bfmmm_io_fail(fn + ": kernel launch or copy back failed");
    ms += (float)bfmmm_post_last_kernel_ms();
  }
  bfmmm_post_set_kernel_ms(ms);
  std::vector<double> h((6 + (size_t)n_aux) * (size_t)n);
  if (hipMemcpy(h.data(), d_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return bfmmm_io_fail(fn + ": kernel launch or copy back failed");
  for (int q = 0; q < 6; ++q)
    if (out[q]) std::copy(h.begin() + (size_t)q * n, h.begin() + (size_t)(q + 1) * n, out[q]);
  if (expect_host) std::copy(h.begin() + 6 * (size_t)n, h.end(), expect_host);
  return 0;
}

}  // namespace

// the PSIS / WAIC pass over n rows of S values on the current device (row i at d_ll + i * ld); out: six host arrays of n
// (lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic).  Shared by bfmmm_post_psis and the file-based entry points, which
// keep the matrix on the device.
int post_psis_device(const double* d_ll, long long ld, int n, int S, double* const out[6]) {
  return psis_run("bfmmm_post_psis", d_ll, ld, n, S, nullptr, 0, 0, out, nullptr);
}

// the same pass, and the expectations of n_aux auxiliary matrices (matrix a at d_aux + a * aux_stride, rows as d_ll's) under each
// row's smoothed weights: expect_host[a * n + i].  The six arrays are post_psis_device's, bit for bit.
int post_psis_expect_device(const double* d_ll, long long ld, int n, int S, const double* d_aux, int n_aux, long long aux_stride,
                            double* const out[6], double* expect_host) {
  if (n_aux < 1 || !d_aux || !expect_host) return bfmmm_io_fail("bfmmm_post_psis_expect: no auxiliary matrix");
  return psis_run("bfmmm_post_psis_expect", d_ll, ld, n, S, d_aux, n_aux, aux_stride, out, expect_host);
}

extern "C" int bfmmm_post_psis(const double* ll, int32_t n, int32_t S, int32_t device, double* lppd, double* elpd_loo, double* p_loo,
                               double* pareto_k, double* elpd_waic, double* p_waic) {
  if (!ll || !lppd || !elpd_loo || !p_loo || !pareto_k || !elpd_waic || !p_waic) return bfmmm_io_fail("bfmmm_post_psis: null argument");
  if (n < 1 || S < 1) return bfmmm_io_fail("bfmmm_post_psis: bad dimensions");
  if (S > S_MAX)
    return bfmmm_io_fail("bfmmm_post_psis: at most 4194304 (2^22) kept draws per curve in this build, got " + std::to_string(S));
  if (select_device(device, "bfmmm_post_psis")) return 1;
  DevBufs b;
  double* d_ll;
  const size_t count = (size_t)n * (size_t)S;
  if (!b.put(&d_ll, nullptr, count)) { (void)hipGetLastError(); return bfmmm_io_fail("bfmmm_post_psis: device allocation failed"); }
  if (hipMemcpy(d_ll, ll, sizeof(double) * count, hipMemcpyHostToDevice) != hipSuccess) return bfmmm_io_fail("bfmmm_post_psis: copy failed");
  double* const out[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  return post_psis_device(d_ll, S, n, S, out);
}

extern "C" int bfmmm_post_psis_expect(const double* ll, const double* h, int32_t n, int32_t S, int32_t n_aux, int32_t device, double* lppd,
                                      double* elpd_loo, double* p_loo, double* pareto_k, double* elpd_waic, double* p_waic, double* expect) {
  const std::pair<const char*, const void*> ptrs[] = {{"ll", ll}, {"h", h}, {"lppd", lppd}, {"elpd_loo", elpd_loo}, {"p_loo", p_loo},
                                                      {"pareto_k", pareto_k}, {"elpd_waic", elpd_waic}, {"p_waic", p_waic}, {"expect", expect}};
  for (const auto& e : ptrs)
    if (!e.second) return bfmmm_io_fail(std::string("bfmmm_post_psis_expect: '") + e.first + "' is null");
  if (n < 1 || S < 1 || n_aux < 1) return bfmmm_io_fail("bfmmm_post_psis_expect: bad dimensions");
  if (S > S_MAX)
    return bfmmm_io_fail("bfmmm_post_psis_expect: at most 4194304 (2^22) kept draws per curve in this build, got " + std::to_string(S));
  if (select_device(device, "bfmmm_post_psis_expect")) return 1;
  DevBufs b;
  double *d_ll, *d_h;
  const size_t count = (size_t)n * (size_t)S;
  if (!b.put(&d_ll, nullptr, count) || !b.put(&d_h, nullptr, count * (size_t)n_aux)) { (void)hipGetLastError(); return bfmmm_io_fail("bfmmm_post_psis_expect: device allocation failed"); }
  if (hipMemcpy(d_ll, ll, sizeof(double) * count, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_h, h, sizeof(double) * count * (size_t)n_aux, hipMemcpyHostToDevice) != hipSuccess)
    return bfmmm_io_fail("bfmmm_post_psis_expect: copy failed");
  double* const out[6] = {lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic};
  return post_psis_expect_device(d_ll, S, n, S, d_h, n_aux, (long long)count, out, expect);
}
