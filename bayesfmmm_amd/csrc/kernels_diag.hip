// Convergence diagnostics of chain batches: split R-hat, bulk / tail ESS, ESS and MCSE of the mean, mean and sd of every row
// of a draws array (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021; the definitions DESIGN.md 7c states).  A row is
// one scalar parameter: x[s + S (c + C p)], draw fastest, then chain, then parameter (R's draws_array order); fp64
// throughout.
//
// k_diag: one workgroup of 256 threads per row.  Every sum is a fixed-order reduction (thread-strided partials, per-wave
// shuffle trees or an LDS tree, combined in a fixed order) and there are no atomics, so two calls give the same bits.
//   split    the 2C sequences of h = floor(S / 2) draws (first and last h of every chain), N = 2 C h values
//   sort     order-preserving 64-bit keys of the N values, bitonic sort (LDS tier: in LDS; global tier: in a workspace)
//   ranks    average ranks by binary search (values below / at or below), z = PPND16((r - 3/8) / (N + 1/4)); the folded
//            set |x - med| from the same sorted keys by two monotone searches (fl(x - med) is monotone in x)
//   sets     z, folded z, raw, I[x <= q05], I[x <= q95] in turn in one sequence buffer: sequence means (two passes, one
//            wave per sequence), centred in place, then R-hat from the lag-0 sum and the variance of the means, or ESS from
//            direct lag sums in blocks of 64 lags, thread 0 running Geyer's initial positive / monotone sequence after each
//            block until the truncation is decided
// Tiers: N <= 8192 keeps keys and sequences in LDS (128 KiB); longer rows use a device workspace of (npow + N) doubles
// per row.  Rows with C S > 2^22 are refused by the callers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/bfmmm_post.h"
#include "launchers.hpp"
#include "post_host.hpp"

// The quantiles and the folded values decide ranks and indicators exactly; they must round as the restatement does.
#pragma clang fp contract(off)

#include "row_stats.hpp"

namespace {

using rs::key_value;
using rs::OpMax;
using rs::OpMin;
using rs::OpSum;
using rs::pow2_ceil;
using rs::u64;
using rs::wave_reduce;

constexpr int NT = 256;                        // threads per workgroup
constexpr int WAVES = NT / 64;
constexpr int LAGB = 64;                       // lags per block of the autocovariance sums
constexpr long long LDS_VALUES = 8192;         // N <= LDS_VALUES: the LDS tier
constexpr long long ROW_MAX = 1LL << 22;       // C S per row in this build
constexpr size_t WS_DEFAULT = 256ull << 20;

// the key of a value in the ranks: -0 and +0 tie there, so they share one key
__device__ inline u64 okey(double x) { return rs::okey(x == 0.0 ? 0.0 : x); }

// Wichura's AS241 (PPND16): the standard normal quantile, about 1e-16 relative
__device__ double ppnd16(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                    4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                 1.3314166789178437745e+2) * r + 3.3871328727963666080e0) /
           (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
             4.2313330701600911252e+1) * r + 1.0);
  }
  double r = sqrt(-log(q < 0 ? p : 1.0 - p)), v;
  if (r <= 5.0) {
    r -= 1.6;
    v = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
             1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
          4.63033784615654529590e0) * r + 1.42343711074968357734e0) /
        (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
             1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
          2.05319162663775882187e0) * r + 1.0);
  } else {
    r -= 5.0;
    v = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
             2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r +
          5.46378491116411436990e0) * r + 6.65790464350110377720e0) /
        (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
             7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
          5.99832206555887937690e-1) * r + 1.0);
  }
  return q < 0 ? -v : v;
}

// k_diag keeps a tree, a key sort and a mean / sd head of its own: with row_stats.hpp's block_reduce, bitonic_sort and
// row_mean_sd (the same operations) it ran 3.5 % slower on 12288 rows of 8 x 1000 draws, for a reason not yet found.
// fixed-order tree over the workgroup's 256 partials; every thread gets the result
template <class Op>
__device__ double block_reduce(double v, double* red, Op op) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = op(red[tid], red[tid + s]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// the row's split layout: value idx < N = 2 C h is draw s of sequence j = idx / h (chain j / 2, first or last h draws)
struct Split {
  int S, h;
  __device__ unsigned src(unsigned idx) const {
    const unsigned j = idx / (unsigned)h, s = idx - j * (unsigned)h;
    return (j >> 1) * (unsigned)S + ((j & 1u) ? (unsigned)(S - h) + s : s);
  }
};

// first position in the sorted keys [0, N) whose key is not below k / is above k
__device__ inline unsigned lower_bound(const u64* key, unsigned N, u64 k) {
  unsigned lo = 0, hi = N;
  while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (key[mid] < k) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ inline unsigned upper_bound(const u64* key, unsigned N, u64 k) {
  unsigned lo = 0, hi = N;
  while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (key[mid] <= k) lo = mid + 1; else hi = mid; }
  return lo;
}
// number of sorted values v with fl(v - med) < f (strict) or <= f (!strict): a prefix, fl(v - med) being monotone in v
__device__ inline unsigned count_dev(const u64* key, unsigned N, double med, double f, bool strict) {
  unsigned lo = 0, hi = N;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    const double d = key_value(key[mid]) - med;
    if (strict ? d < f : d <= f) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// type-7 quantile of the sorted values
__device__ inline double quantile7(const u64* key, unsigned N, double p) {
  const double g = (double)(N - 1) * p;
  const unsigned lo = (unsigned)floor(g);
  const double a = key_value(key[lo]);
  if (lo + 1 >= N) return a;
  return a + (g - (double)lo) * (key_value(key[lo + 1]) - a);
}

struct Moments { double W, varmu; bool degenerate; };

// sequence means of the m x n buffer y (one wave per sequence, lane-strided, butterfly), the sequences centred in place;
// W = n / (n - 1) mean_j gamma_j(0), varmu = var_j(mean_j) (m - 1 denominator); degenerate: a non-finite value or
// max - min < 2^-52.  Pass 1 takes the means' mean, pass 2 recomputes every mean bit for bit and centres.
__device__ Moments seq_moments(double* y, int m, int n, double* red) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double* wsum = red + NT;                 // WAVES x 4 scratch past the reduction array
  double smu = 0.0, mn = INFINITY, mx = -INFINITY, bad = 0.0;
  for (int j = w; j < m; j += WAVES) {
    const double* yj = y + (size_t)j * n;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) { const double v = yj[i]; s += v; mn = fmin(mn, v); mx = fmax(mx, v); if (!isfinite(v)) bad = 1.0; }
    smu += wave_reduce(s, OpSum()) / (double)n;
  }
  mn = wave_reduce(mn, OpMin()); mx = wave_reduce(mx, OpMax()); bad = wave_reduce(bad, OpMax());
  if (lane == 0) { wsum[4 * w] = smu; wsum[4 * w + 1] = mn; wsum[4 * w + 2] = mx; wsum[4 * w + 3] = bad; }
  __syncthreads();
  double mbar = 0.0, gmn = INFINITY, gmx = -INFINITY, gbad = 0.0;
  for (int v = 0; v < WAVES; ++v) { mbar += wsum[4 * v]; gmn = fmin(gmn, wsum[4 * v + 1]); gmx = fmax(gmx, wsum[4 * v + 2]); gbad = fmax(gbad, wsum[4 * v + 3]); }
  mbar /= (double)m;
  __syncthreads();
  Moments r;
  r.degenerate = gbad > 0.0 || !(gmx - gmn >= DBL_EPSILON);
  if (r.degenerate) { r.W = r.varmu = NAN; return r; }
  double dmu = 0.0, sq = 0.0;
  for (int j = w; j < m; j += WAVES) {
    double* yj = y + (size_t)j * n;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += yj[i];
    const double mu = wave_reduce(s, OpSum()) / (double)n;
    dmu += (mu - mbar) * (mu - mbar);
    for (int i = lane; i < n; i += 64) { const double c = yj[i] - mu; yj[i] = c; sq += c * c; }
  }
  if (lane == 0) wsum[4 * w] = dmu;
  sq = block_reduce(sq, red, OpSum());     // (its barriers publish wsum and the centred values)
  double vm = 0.0;
  for (int v = 0; v < WAVES; ++v) vm += wsum[4 * v];
  __syncthreads();
  r.varmu = m > 1 ? vm / (double)(m - 1) : 0.0;
  r.W = (double)n / (double)(n - 1) * (sq / ((double)m * (double)n));
  return r;
}

__device__ inline double rhat_of(const Moments& mo, int n) {
  if (mo.degenerate || n < 2) return NAN;
  const double B = (double)n * mo.varmu;
  return sqrt((B / mo.W + (double)(n - 1)) / (double)n);
}

// ESS of the centred m x n buffer y: lag sums in blocks of LAGB lags (lane = lag in the block, wave = a quarter of the
// positions, the quarters added in a fixed order), Geyer's truncation by thread 0 after each block
__device__ double ess_of(const double* y, const Moments& mo, int m, int n, double* red, double* acov, int* flag) {
  if (mo.degenerate || n < 3) return NAN;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const double var_plus = (double)(n - 1) / (double)n * mo.W + mo.varmu;
  const double mn = (double)m * (double)n;
  int t = 0;                               // thread 0's state: current even lag t, (e, o) = rho(t), rho(t + 1)
  double e = 1.0, o = 0.0, runmin = 0.0, psum = 0.0;
  for (int t0 = 0; ; t0 += LAGB) {
    const int lag = t0 + lane;
    double part = 0.0;
    if (lag < n)
      for (int j = 0; j < m; ++j) {
        const double* yj = y + (size_t)j * n;
        for (int s = w; s < n - lag; s += WAVES) part += yj[s] * yj[s + lag];
      }
    red[tid] = part;
    __syncthreads();
    if (tid < LAGB) acov[tid] = (red[tid] + red[tid + 64]) + (red[tid + 128] + red[tid + 192]);
    __syncthreads();
    if (tid == 0) {
      auto rho = [&](int u) { return 1.0 - (mo.W - acov[u - t0] / mn) / var_plus; };
      if (t0 == 0) o = rho(1);
      int done = 0;
      for (;;) {
        if (!(t < n - 5 && e + o > 0)) { done = 1; break; }
        if (t + 2 >= t0 + LAGB) break;     // the next pair lies in the next block
        const double P = e + o;            // a pair before the truncation: monotone (running minimum), summed
        runmin = (t == 0 || P <= runmin) ? P : runmin;
        psum += runmin;
        t += 2;
        e = rho(t);
        o = rho(t + 1);
      }
      if (done) {
        const double last = (e > 0 || e + o >= 0) ? e : 0.0;
        double tau = -1.0 + 2.0 * psum + last;
        const double cap = 1.0 / log10(mn);
        if (tau < cap) tau = cap;
        red[0] = mn / tau;
      }
      flag[0] = done;
    }
    __syncthreads();
    const int done = flag[0];
    const double ess = red[0];
    __syncthreads();
    if (done) return ess;
  }
}

// one row per workgroup; GL: keys and sequences in the workspace (row blockIdx.x at ws + blockIdx.x * ws_stride)
template <bool GL>
__global__ __launch_bounds__(NT) void k_diag(const double* x, int C, int S, u64* ws, long long ws_stride, double* out, long long ld_out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double red[NT + 4 * WAVES];
  __shared__ double acov[LAGB];
  __shared__ int flag[1];
  const int tid = threadIdx.x;
  const long long NS = (long long)C * S;
  const double* row = x + (size_t)blockIdx.x * (size_t)NS;
  const int h = S / 2, m = 2 * C, n = h;
  const unsigned N = (unsigned)m * (unsigned)h;
  const unsigned npow = pow2_ceil(N);
  u64* key = GL ? ws + (size_t)blockIdx.x * (size_t)ws_stride : (u64*)sm;
  double* y = GL ? (double*)(key + npow) : sm + npow;
  const Split sp{S, h};

  // ---- mean, sd over the C S draws (unsplit) ----
  double sum = 0.0;
  for (long long i = tid; i < NS; i += NT) sum += row[i];
  const double mean = block_reduce(sum, red, OpSum()) / (double)NS;
  double sq = 0.0;
  for (long long i = tid; i < NS; i += NT) { const double d = row[i] - mean; sq += d * d; }
  sq = block_reduce(sq, red, OpSum());
  const double sd = NS > 1 ? sqrt(sq / (double)(NS - 1)) : NAN;
  double rhat = NAN, ess_bulk = NAN, ess_tail = NAN, ess_mean = NAN;

  // ---- the split set: degenerate? ----
  double mn = INFINITY, mx = -INFINITY, bad = 0.0;
  for (unsigned i = tid; i < N; i += NT) { const double v = row[sp.src(i)]; mn = fmin(mn, v); mx = fmax(mx, v); if (!isfinite(v)) bad = 1.0; }
  mn = block_reduce(mn, red, OpMin());
  mx = block_reduce(mx, red, OpMax());
  bad = block_reduce(bad, red, OpMax());
  if (N > 0 && bad == 0.0 && mx - mn >= DBL_EPSILON) {
    // ---- bitonic sort of the keys (padding above every finite key) ----
    for (unsigned i = tid; i < npow; i += NT) key[i] = i < N ? okey(row[sp.src(i)]) : ~0ULL;
    __syncthreads();
    for (unsigned k = 2; k <= npow; k <<= 1)
      for (unsigned j = k >> 1; j > 0; j >>= 1) {
        for (unsigned i = tid; i < npow / 2; i += NT) {
          const unsigned a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a + j;
          const u64 ka = key[a], kb = key[b];
          if ((ka > kb) == ((a & k) == 0)) { key[a] = kb; key[b] = ka; }
        }
        __syncthreads();
      }
    const double med = quantile7(key, N, 0.5), q05 = quantile7(key, N, 0.05), q95 = quantile7(key, N, 0.95);
    const double den = (double)N + 0.25;

    // ---- bulk: z over the split set ----
    for (unsigned i = tid; i < N; i += NT) {
      const u64 k = okey(row[sp.src(i)]);
      const double r = (double)(lower_bound(key, N, k) + upper_bound(key, N, k) + 1) * 0.5;
      y[i] = ppnd16((r - 0.375) / den);
    }
    __syncthreads();
    Moments mo = seq_moments(y, m, n, red);
    const double rb = rhat_of(mo, n);
    ess_bulk = ess_of(y, mo, m, n, red, acov, flag);

    // ---- folded: z over |x - med|, ranked from the same sorted keys ----
    for (unsigned i = tid; i < N; i += NT) {
      const double f = fabs(row[sp.src(i)] - med);
      const unsigned lt = f > 0 ? count_dev(key, N, med, f, true) - count_dev(key, N, med, -f, false) : 0u;
      const unsigned le = count_dev(key, N, med, f, false) - count_dev(key, N, med, -f, true);
      y[i] = ppnd16(((double)(lt + le + 1) * 0.5 - 0.375) / den);
    }
    __syncthreads();
    mo = seq_moments(y, m, n, red);
    const double rf = rhat_of(mo, n);
    rhat = (isnan(rb) || isnan(rf)) ? NAN : fmax(rb, rf);

    // ---- the draws themselves: ESS of the mean ----
    for (unsigned i = tid; i < N; i += NT) y[i] = row[sp.src(i)];
    __syncthreads();
    mo = seq_moments(y, m, n, red);
    ess_mean = ess_of(y, mo, m, n, red, acov, flag);

    // ---- tails: the indicators of the 5 % and 95 % quantiles ----
    double et[2];
    for (int side = 0; side < 2; ++side) {
      const double q = side ? q95 : q05;
      for (unsigned i = tid; i < N; i += NT) y[i] = row[sp.src(i)] <= q ? 1.0 : 0.0;
      __syncthreads();
      mo = seq_moments(y, m, n, red);
      et[side] = ess_of(y, mo, m, n, red, acov, flag);
    }
    ess_tail = (isnan(et[0]) || isnan(et[1])) ? NAN : fmin(et[0], et[1]);
  }
  if (tid == 0) {
    double* o = out + blockIdx.x;
    o[0] = rhat;
    o[ld_out] = ess_bulk;
    o[2 * ld_out] = ess_tail;
    o[3 * ld_out] = ess_mean;
    o[4 * ld_out] = sd / sqrt(ess_mean);
    o[5 * ld_out] = mean;
    o[6 * ld_out] = sd;
  }
}

// ws[s + S (c + C p)] = chain c's slot (first + s), element p0 + p: element e of slot t of chain c at
// base + c * chain_bytes (bytes) + t * ss + e * ps (doubles).  32 x 32 tiles through LDS: read along the element index,
// written along the draw index.
__global__ __launch_bounds__(256) void k_diag_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first,
                                                     int S, int C, int p0, int P, double* ws) {
  __shared__ double tile[32][33];
  const int tiles_s = (S + 31) / 32;
  const int ts = (int)(blockIdx.x % (unsigned)tiles_s), tp = (int)(blockIdx.x / (unsigned)tiles_s), c = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double* src = (const double*)((const char*)base + (size_t)c * chain_bytes);
  for (int r = ty; r < 32; r += 8) {
    const int s = ts * 32 + r, p = tp * 32 + tx;
    if (s < S && p < P) tile[r][tx] = src[(long long)(first + s) * ss + (long long)(p0 + p) * ps];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int p = tp * 32 + r, s = ts * 32 + tx;
    if (s < S && p < P) ws[(size_t)s + (size_t)S * ((size_t)c + (size_t)C * (size_t)p)] = tile[tx][r];
  }
}

bool lds_tier(int C, int S) { return (long long)2 * C * (S / 2) <= LDS_VALUES; }

}  // namespace

long long diag_row_max() { return ROW_MAX; }

// workspace doubles one row of the global tier needs (0 in the LDS tier)
size_t diag_row_ws_doubles(int C, int S) {
  if (lds_tier(C, S)) return 0;
  const long long N = (long long)2 * C * (S / 2);
  return pow2_ceil((size_t)N) + (size_t)N;
}

// the diagnostics of rows [0, rows) of d_x (row-major, C S doubles per row) on stream st into d_out (7 arrays of ld_out,
// written at [0, rows)); the global tier needs ws of at least ws_rows * diag_row_ws_doubles(C, S) doubles and runs in
// launches of ws_rows rows.  Returns "" or the failure.
std::string diag_launch(const double* d_x, long long rows, int C, int S, double* d_out, long long ld_out, double* ws, long long ws_rows,
                        hipStream_t st) {
  if ((long long)C * S > ROW_MAX) return "at most 4194304 (2^22) draws per row (n_chains x n_draws) in this build";
  const long long NS = (long long)C * S;
  if (lds_tier(C, S)) {
    const long long N = (long long)2 * C * (S / 2);
    const size_t lds = (pow2_ceil((size_t)N) + (size_t)N) * sizeof(double);
    if (hipFuncSetAttribute((const void*)k_diag<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>(lds, 8)) != hipSuccess) {
      (void)hipGetLastError();
      return "cannot set the LDS size of k_diag";
    }
    for (long long r0 = 0; r0 < rows; r0 += 1 << 30)
      hipLaunchKernelGGL(k_diag<false>, dim3((unsigned)std::min<long long>(rows - r0, 1 << 30)), dim3(NT), lds, st, d_x + r0 * NS, C, S,
                         (u64*)nullptr, 0LL, d_out + r0, ld_out);
  } else {
    const long long per = (long long)diag_row_ws_doubles(C, S);
    if (!ws || ws_rows < 1) return "no workspace for the global tier";
    for (long long r0 = 0; r0 < rows; r0 += ws_rows)
      hipLaunchKernelGGL(k_diag<true>, dim3((unsigned)std::min(rows - r0, ws_rows)), dim3(NT), 0, st, d_x + r0 * NS, C, S, (u64*)ws, per,
                         d_out + r0, ld_out);
  }
  if (hipGetLastError() != hipSuccess) return "kernel launch failed";
  return "";
}

// k_diag_gather over elements [p0, p0 + P) of slots [first, first + S) of all C chains into ws (row-major rows)
std::string diag_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S, int C, int p0, int P,
                        double* ws, hipStream_t st) {
  const long long tiles = (long long)((S + 31) / 32) * ((P + 31) / 32);
  if (tiles > 0x7fffffffLL || C > 65535) return "gather grid too large";
  hipLaunchKernelGGL(k_diag_gather, dim3((unsigned)tiles, 1, (unsigned)C), dim3(256), 0, st, base, chain_bytes, ss, ps, first, S, C, p0, P, ws);
  if (hipGetLastError() != hipSuccess) return "gather launch failed";
  return "";
}

extern "C" int bfmmm_post_diagnostics(const double* draws, int64_t n_param, int32_t n_chains, int32_t n_draws, int32_t device, double* rhat,
                                      double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean, double* mean, double* sd) {
  const char* names[] = {"draws", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd"};
  const void* ptrs[] = {draws, rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  for (int i = 0; i < 8; ++i)
    if (!ptrs[i]) return bfmmm_io_fail(std::string("bfmmm_post_diagnostics: '") + names[i] + "' is null");
  if (n_param < 1) return bfmmm_io_fail("bfmmm_post_diagnostics: 'n_param' must be at least 1");
  if (n_chains < 1) return bfmmm_io_fail("bfmmm_post_diagnostics: 'n_chains' must be at least 1");
  if (n_draws < 1) return bfmmm_io_fail("bfmmm_post_diagnostics: 'n_draws' must be at least 1");
  const long long NS = (long long)n_chains * n_draws;
  if (NS > ROW_MAX)
    return bfmmm_io_fail("bfmmm_post_diagnostics: at most 4194304 (2^22) draws per row (n_chains x n_draws) in this build, got " +
                         std::to_string(NS));
  if (select_device(device, "bfmmm_post_diagnostics")) return 1;
  const size_t per = diag_row_ws_doubles(n_chains, n_draws);
  const long long ws_rows = per ? std::max<long long>(1, std::min<long long>(n_param, (long long)(WS_DEFAULT / (per * sizeof(double))))) : 0;
  DevBufs b;
  double *d_x, *d_out, *d_ws = nullptr;
  const size_t count = (size_t)n_param * (size_t)NS;
  if (!b.put(&d_x, nullptr, count) || !b.put(&d_out, nullptr, 7 * (size_t)n_param) || (per && !b.put(&d_ws, nullptr, per * (size_t)ws_rows))) {
    (void)hipGetLastError();
    return bfmmm_io_fail("bfmmm_post_diagnostics: device allocation failed");
  }
  std::string err;
  if (hipMemcpy(d_x, draws, sizeof(double) * count, hipMemcpyHostToDevice) != hipSuccess) err = "copy failed";
  const auto enqueue = [&] { err = diag_launch(d_x, n_param, n_chains, n_draws, d_out, n_param, d_ws, ws_rows, 0); return err.empty(); };
  if (err.empty() && !timed_launch(enqueue) && err.empty()) err = "kernel failed";
  std::vector<double> hb(7 * (size_t)n_param);
  if (err.empty() && hipMemcpy(hb.data(), d_out, sizeof(double) * hb.size(), hipMemcpyDeviceToHost) != hipSuccess) err = "copy back failed";
  if (!err.empty()) return bfmmm_io_fail("bfmmm_post_diagnostics: " + err);
  double* const outs[7] = {rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, mean, sd};
  for (int q = 0; q < 7; ++q) std::copy(hb.begin() + (size_t)q * n_param, hb.begin() + (size_t)(q + 1) * n_param, outs[q]);
  return 0;
}
