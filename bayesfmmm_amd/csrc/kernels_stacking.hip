// Stacking of predictive distributions (Yao, Vehtari, Simpson & Gelman 2018; for chains that do not mix, Yao, Vehtari & Gelman
// 2022): the simplex weights w that maximise f(w) = sum_i log sum_q w_q exp(L_iq) for an n x Q matrix of
// leave-one-out log predictive densities, candidate-major (L[q n + i]), 1 <= Q <= 64.  Everything in fp64.
//
//   k_stack_prepare  a thread a row: m_i = max_q L_iq, P_iq = exp(L_iq - m_i) in place of L (0 for -inf); the entries that are NaN or
//                    +inf and the rows that are -inf throughout are counted and the first of them kept (integer atomics)
//   k_stack_em       launch j derives the iterate w_j, the same bits in every workgroup: w_0 is the start, otherwise thread q adds
//                    the partial rows of launch j - 1 in workgroup order (in a few segments, then the segments in order) to
//                    g_q(w_(j-1)) and w_j = w_(j-1) g / n; workgroup 0 writes
//                    w_j to the weight buffer j & 1 and (gap, f, j - 1) of w_(j-1) where the host reads them.  Then the threads
//                    own the rows grid-stride, d_i = sum_q w_q P_iq, and add P_iq / d_i and m_i + log d_i into Q + 1 registers;
//                    a butterfly inside the wave, the four waves in order through LDS, one partial row per workgroup into the
//                    partial buffer j & 1.  Every launch ends by itself: nothing waits on another workgroup.
//   k_stack_final    l_i = m_i + log d_i(w) of the returned iterate
//
// The order of every sum is a function of (n, Q) alone: the grid is min(ST_GRID_MAX, ceil(n / ST_NT)) workgroups of ST_NT threads,
// and there are no floating-point atomics, so two calls give the same bits whatever check_every is.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/bfmmm_post.h"
#include "launchers.hpp"
#include "post_host.hpp"
#include "row_stats.hpp"

namespace {

using namespace rs;

constexpr int ST_NT = 256;            // threads per workgroup
constexpr int ST_GRID_MAX = 256;      // workgroups of k_stack_em: one a CU, one grid-stride pass covers ST_NT ST_GRID_MAX rows
constexpr int ST_QMAX = 64;           // candidates
constexpr int ST_WAVES = ST_NT / 64;

// [0] the offending entries and rows, [1] the smallest i 64 + q among them (a row that is -inf throughout: q = 0)
__global__ __launch_bounds__(ST_NT) void k_stack_prepare(double* L, long long n, int Q, double* m, unsigned long long* bad) {
  const long long i = (long long)blockIdx.x * ST_NT + threadIdx.x;
  if (i >= n) return;
  double mx = -INFINITY;
  unsigned cnt = 0;
  int first = -1;
  for (int q = 0; q < Q; ++q) {
    const double x = L[(size_t)q * (size_t)n + (size_t)i];
    if (x != x || x == INFINITY) { ++cnt; if (first < 0) first = q; }
    mx = fmax(mx, x);
  }
  if (cnt == 0 && mx == -INFINITY) { cnt = 1; first = 0; }
  if (cnt) {
    atomicAdd(&bad[0], (unsigned long long)cnt);
    atomicMin(&bad[1], (unsigned long long)i * 64ull + (unsigned long long)first);
    return;
  }
  m[i] = mx;
  for (int q = 0; q < Q; ++q) {
    const size_t e = (size_t)q * (size_t)n + (size_t)i;
    L[e] = exp(L[e] - mx);
  }
}

struct EmArgs {
  const double* P;         // Q x n
  const double* m;         // n
  long long n;
  int Q, nblk, j;          // j: the launch, which forms w_j
  int wp_log2, seg;        // the partial rows are added in ST_NT >> wp_log2 segments of seg workgroups, 2^wp_log2 >= Q + 1 columns each
  double* wbuf;            // 2 x ST_QMAX
  double* part;            // 2 x nblk x (Q + 1)
  double* rec;             // gap, f and the index of the iterate they belong to
};

template <int QT>
__global__ __launch_bounds__(ST_NT) void k_stack_em(EmArgs a) {
  __shared__ double sW[ST_QMAX];
  __shared__ double sG[ST_QMAX + 1];
  __shared__ double sRed[ST_WAVES][ST_QMAX + 1];
  __shared__ double sSeg[ST_NT];
  const int tid = threadIdx.x, Q = a.Q, j = a.j, W = Q + 1;
  const double nd = (double)a.n;
  // ---- the iterate of this launch, the same bits in every workgroup ----
  // Thread (s, q) adds column q of the partial rows of segment s, seg consecutive workgroups, in their order; thread q then adds the
  // segments in theirs.  The loads of a segment are independent and go out ahead of the additions.
  if (j == 0) {
    if (tid < Q) sW[tid] = a.wbuf[tid];
  } else {
    const double* prev = a.part + (size_t)((j - 1) & 1) * (size_t)a.nblk * W;
    const int q = tid & ((1 << a.wp_log2) - 1), s = tid >> a.wp_log2;
    double g = 0.0;
    if (q < W) {
      const int b1 = min(a.nblk, (s + 1) * a.seg);
#pragma unroll 8
      for (int b = s * a.seg; b < b1; ++b) g += prev[(size_t)b * W + q];
    }
    sSeg[tid] = g;
    __syncthreads();
    if (tid < W) {
      double t = sSeg[tid];
      for (int k = 1; k < (ST_NT >> a.wp_log2); ++k) t += sSeg[(k << a.wp_log2) + tid];
      sG[tid] = t;
      if (tid < Q) sW[tid] = a.wbuf[(size_t)((j - 1) & 1) * ST_QMAX + tid] * t / nd;
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid < Q) a.wbuf[(size_t)(j & 1) * ST_QMAX + tid] = sW[tid];
    if (j > 0 && tid == 0) {
      double gmax = sG[0];
      for (int q = 1; q < Q; ++q) gmax = fmax(gmax, sG[q]);
      a.rec[0] = gmax / nd - 1.0;
      a.rec[1] = sG[Q];
      a.rec[2] = (double)(j - 1);
    }
  }
  // ---- the rows of this thread ----
  // Q <= QT accumulators in registers, the weights from LDS (one address a wave).  Every one of the QT loads is issued, those
  // past Q from column Q - 1 once more, so that no load sits behind a branch; their products are not used.
  double acc[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) acc[q] = 0.0;
  double fs = 0.0;
  const size_t n = (size_t)a.n, step = (size_t)a.nblk * ST_NT;
  for (size_t i = (size_t)blockIdx.x * ST_NT + tid; i < n; i += step) {
    double p[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) p[q] = a.P[(size_t)(q < Q ? q : Q - 1) * n + i];
    double d = 0.0;
#pragma unroll
    for (int q = 0; q < QT; ++q)
      if (q < Q) d += sW[q] * p[q];
#pragma unroll
    for (int q = 0; q < QT; ++q)
      if (q < Q) acc[q] += p[q] / d;
    fs += a.m[i] + log(d);
  }
  // ---- wave butterfly, then the waves in order ----
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < QT; ++q)
    if (q < Q) {
      const double v = wave_reduce(acc[q], OpSum());
      if (lane == 0) sRed[wave][q] = v;
    }
  fs = wave_reduce(fs, OpSum());
  if (lane == 0) sRed[wave][Q] = fs;
  __syncthreads();
  if (tid < W) {
    double v = sRed[0][tid];
    for (int k = 1; k < ST_WAVES; ++k) v += sRed[k][tid];
    a.part[((size_t)(j & 1) * (size_t)a.nblk + blockIdx.x) * W + tid] = v;
  }
}

__global__ __launch_bounds__(ST_NT) void k_stack_final(const double* P, const double* m, long long n, int Q, const double* w, double* out) {
  __shared__ double sW[ST_QMAX];
  if ((int)threadIdx.x < Q) sW[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * ST_NT + threadIdx.x;
  if (i >= n) return;
  double d = 0.0;
  for (int q = 0; q < Q; ++q) d += sW[q] * P[(size_t)q * (size_t)n + (size_t)i];
  out[i] = m[i] + log(d);
}

using EmKernel = void (*)(EmArgs);
EmKernel em_pick(int Q) {
  if (Q <= 1) return k_stack_em<1>;
  if (Q <= 2) return k_stack_em<2>;
  if (Q <= 4) return k_stack_em<4>;
  if (Q <= 8) return k_stack_em<8>;
  if (Q <= 16) return k_stack_em<16>;
  if (Q <= 32) return k_stack_em<32>;
  return k_stack_em<64>;
}

const char* const kFn = "bfmmm_post_stacking";

std::string describe(double x) { return x != x ? "NaN" : x == INFINITY ? "+inf" : "-inf for every candidate of the unit"; }

}  // namespace

void post_stacking_geometry(int* threads, int* max_workgroups) {
  *threads = ST_NT;
  *max_workgroups = ST_GRID_MAX;
}

// The whole computation on the current device, on its default stream.  d_L: Q x n log densities, candidate-major, which become P;
// init: Q host weights or null (uniform), checked by the caller.  The results go to the host; see bfmmm_post_stacking.
int post_stacking_device(double* d_L, long long n, int Q, const double* init, int max_iter, int check_every, double tol, double* weights,
                         double* pointwise, double* objective, double* gap, int* n_iter, int* converged) {
  const std::string fn(kFn);
  const int nblk = (int)std::min<long long>(ST_GRID_MAX, (n + ST_NT - 1) / ST_NT);
  const long long rows_blk = (n + ST_NT - 1) / ST_NT;
  if (rows_blk > 2147483647LL) return bfmmm_io_fail(fn + ": at most 2147483647 x 256 units in this build, got " + std::to_string(n));
  DevBufs b;
  double *d_m, *d_w, *d_part, *d_rec, *d_out;
  unsigned long long* d_bad;
  const unsigned long long bad0[2] = {0ull, ~0ull};
  std::vector<double> w0((size_t)2 * ST_QMAX, 0.0);
  for (int q = 0; q < Q; ++q) w0[(size_t)q] = init ? init[q] : 1.0 / (double)Q;
  if (!b.put(&d_m, nullptr, (size_t)n) || !b.put(&d_w, w0.data(), w0.size()) || !b.put(&d_part, nullptr, (size_t)2 * nblk * (Q + 1)) ||
      !b.put(&d_rec, nullptr, 4) || !b.put(&d_out, nullptr, (size_t)n) || !b.put(&d_bad, bad0, 2)) {
    (void)hipGetLastError();
    return bfmmm_io_fail(fn + ": device allocation failed");
  }
  hipLaunchKernelGGL(k_stack_prepare, dim3((unsigned)rows_blk), dim3(ST_NT), 0, 0, d_L, n, Q, d_m, d_bad);
  unsigned long long bad[2];
  if (hipMemcpy(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
    return bfmmm_io_fail(fn + ": kernel launch or copy back failed");
  if (bad[0]) {
    const long long i = (long long)(bad[1] / 64ull);
    const int q = (int)(bad[1] % 64ull);
    double x = 0.0;      // the prepare kernel leaves an offending row as it was
    if (hipMemcpy(&x, d_L + (size_t)q * (size_t)n + (size_t)i, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return bfmmm_io_fail(fn + ": kernel launch or copy back failed");
    return bfmmm_io_fail(fn + ": 'lpd' must hold finite values or -inf, with a finite value in every unit: " + std::to_string(bad[0]) +
                         " offending entries or units, the first at unit " + std::to_string(i) + ", candidate " + std::to_string(q) +
                         " (" + describe(x) + ")");
  }
  // Launch j forms w_j and the partial sums of g(w_j) and f(w_j); launch j + 1 reports gap and f of w_j.  A candidate t (a multiple
  // of check_every, or max_iter) is therefore read after launch t + 1; w_t is still in weight buffer t & 1 then.
  const EmKernel em = em_pick(Q);
  int wp_log2 = 0;
  while ((1 << wp_log2) < Q + 1) ++wp_log2;
  const int nseg = ST_NT >> wp_log2;
  EmArgs a{d_L, d_m, n, Q, nblk, 0, wp_log2, (nblk + nseg - 1) / nseg, d_w, d_part, d_rec};
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, 0);
  int j = 0, t = 0, conv = 0;
  double rec[3] = {0.0, 0.0, 0.0};
  bool ok = true;
  while (ok) {
    t = (int)std::min<long long>(max_iter, ((long long)t / check_every + 1) * check_every);      // the next candidate
    for (; j <= t + 1; ++j) { a.j = j; hipLaunchKernelGGL(em, dim3(nblk), dim3(ST_NT), 0, 0, a); }
    ok = hipMemcpy(rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost) == hipSuccess && hipGetLastError() == hipSuccess && rec[2] == (double)t;
    if (!ok) break;
    conv = rec[0] <= tol;
    if (t == max_iter || (conv && tol > 0.0)) break;
  }
  (void)hipEventRecord(e1, 0);
  if (ok) ok = hipEventSynchronize(e1) == hipSuccess;
  float ms = 0.f;
  if (ok) { (void)hipEventElapsedTime(&ms, e0, e1); bfmmm_post_set_kernel_ms(ms); }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (!ok) { (void)hipGetLastError(); return bfmmm_io_fail(fn + ": kernel launch or copy back failed"); }
  const double* d_wt = d_w + (size_t)(t & 1) * ST_QMAX;
  hipLaunchKernelGGL(k_stack_final, dim3((unsigned)rows_blk), dim3(ST_NT), 0, 0, d_L, d_m, n, Q, d_wt, d_out);
  if (hipMemcpy(weights, d_wt, sizeof(double) * (size_t)Q, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(pointwise, d_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
    return bfmmm_io_fail(fn + ": kernel launch or copy back failed");
  *gap = rec[0];
  *objective = rec[1];
  *n_iter = t;
  *converged = conv;
  return 0;
}

extern "C" void bfmmm_post_stacking_geometry(int32_t* threads, int32_t* max_workgroups) {
  int t = 0, g = 0;
  post_stacking_geometry(&t, &g);
  if (threads) *threads = t;
  if (max_workgroups) *max_workgroups = g;
}

extern "C" int bfmmm_post_stacking(const double* lpd, int64_t n, int Q, int device, const double* init, int max_iter, int check_every,
                                   double tol, double* weights, double* pointwise, double* objective, double* gap, int* n_iter,
                                   int* converged) {
  const std::string fn(kFn);
  const std::pair<const char*, const void*> ptrs[] = {{"lpd", lpd}, {"weights", weights}, {"pointwise", pointwise}, {"objective", objective},
                                                      {"gap", gap}, {"n_iter", n_iter}, {"converged", converged}};
  for (const auto& e : ptrs)
    if (!e.second) return bfmmm_io_fail(fn + ": '" + e.first + "' is null");
  if (n < 1) return bfmmm_io_fail(fn + ": 'n' must be at least 1, got " + std::to_string(n));
  if (Q < 1 || Q > ST_QMAX) return bfmmm_io_fail(fn + ": 'Q' must lie in 1 .. 64 (at most 64 candidates in this build), got " + std::to_string(Q));
  if (max_iter < 1) return bfmmm_io_fail(fn + ": 'max_iter' must be at least 1, got " + std::to_string(max_iter));
  if (check_every < 1) return bfmmm_io_fail(fn + ": 'check_every' must be at least 1, got " + std::to_string(check_every));
  if (!(tol >= 0.0) || tol == INFINITY) return bfmmm_io_fail(fn + ": 'tol' must be finite and not negative");
  if (init) {
    double s = 0.0;
    for (int q = 0; q < Q; ++q) {
      if (!(init[q] > 0.0) || init[q] == INFINITY)
        return bfmmm_io_fail(fn + ": 'init' must lie on the simplex with every weight positive: 'init'[" + std::to_string(q) + "] = " + std::to_string(init[q]));
      s += init[q];
    }
    if (std::fabs(s - 1.0) > 1e-10) return bfmmm_io_fail(fn + ": 'init' must lie on the simplex: its weights add to " + std::to_string(s));
  }
  if (select_device(device, kFn)) return 1;
  DevBufs b;
  double* d_L;
  if (!b.put(&d_L, lpd, (size_t)n * (size_t)Q)) { (void)hipGetLastError(); return bfmmm_io_fail(fn + ": device allocation or copy failed"); }
  return post_stacking_device(d_L, (long long)n, Q, init, max_iter, check_every, tol, weights, pointwise, objective, gap, n_iter, converged);
}
