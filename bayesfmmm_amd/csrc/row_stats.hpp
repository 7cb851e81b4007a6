// What the post-processing kernels do to a "row of draws" with one workgroup: fixed-order reductions, the two-pass mean and
// sd, a bitonic sort, the quantile rule and the order-preserving keys.  One copy, so that tiers and routes whose results must
// agree bit for bit run the same statements.
//
// Contraction: this header sets no `fp contract` pragma.  Include it AFTER the including file's own pragma; its functions then
// round as that file does (kernels_bands.hip, kernels_loo.hip: contraction on, the compiler's default; kernels_curve_fit.hip,
// kernels_diag.hip: off).  Two consequences stay in kernels_curve_fit.hip: k_fit_quantiles reads the rule off rows that
// k_bands_quantiles_big has sorted, so that long rows interpolate without an fma as short ones do, and k_fit_sim adds its
// squares with an explicit fma (`fused`) where the long rows' sd must equal k_bands_moments'.
//
// Every function is called by all threads of the workgroup (NT of them) and is inlined; pointers are passed as they are, so a
// row in LDS is read with LDS instructions and a row in global memory with global ones.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace rs {

typedef unsigned long long u64;

// the smallest power of two that is at least n (1 for n <= 1)
template <class I>
__host__ __device__ __forceinline__ I pow2_ceil(I n) {
  I p = 1;
  while (p < n) p <<= 1;
  return p;
}

// order-preserving image of a double (ascending doubles -> ascending unsigned keys; -0 below +0) and its inverse
__device__ __forceinline__ u64 okey(double x) {
  const u64 u = (u64)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double key_value(u64 k) {
  return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ULL) : ~k));
}

struct OpSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };

// Fixed-order tree over the workgroup's NT partials in red[NT]; every thread gets the result.  block_tree leaves it in red[0]:
// a barrier must follow before red is written again.  block_reduce has that barrier.  (The upper partial is read first:
// the compiler orders the add's operands by it, and of two NaN partials the sum takes the sign of the first.)
template <int NT, class Op>
__device__ __forceinline__ double block_tree(double v, double* red, Op op) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) { const double hi = red[tid + s]; red[tid] = op(red[tid], hi); }
    __syncthreads();
  }
  return red[0];
}
template <int NT, class Op>
__device__ __forceinline__ double block_reduce(double v, double* red, Op op) {
  const double r = block_tree<NT>(v, red, op);
  __syncthreads();
  return r;
}

// butterfly over the 64 lanes of a wave (commutative pairs: every lane ends with the same bits)
template <class Op>
__device__ __forceinline__ double wave_reduce(double v, Op op) {
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off));
  return v;
}

// mean and sd (N - 1) of v[0 .. T): thread-strided partials, then the tree; the mean first, then the squares about it
template <int NT, class Len>
__device__ __forceinline__ void row_mean_sd(const double* v, Len T, double* red, double& mean, double& sd) {
  const int tid = threadIdx.x;
  double a = 0.0;
  for (Len e = tid; e < T; e += NT) a += v[e];
  const double m = block_reduce<NT>(a, red, OpSum()) / (double)T;
  double q = 0.0;
  for (Len e = tid; e < T; e += NT) { const double dlt = v[e] - m; q += dlt * dlt; }
  mean = m;
  sd = sqrt(block_reduce<NT>(q, red, OpSum()) / (double)(T - 1));
}

// ---- element access of the sort and of the quantile rule ----
// plain loads and stores: a row in LDS, or one in global memory that only this workgroup touches between its barriers
template <class T>
struct Plain {
  T* s;
  __device__ T ld(int e) const { return s[e]; }
  __device__ void st(int e, T v) const { s[e] = v; }
};
// relaxed agent-scope accesses: a row in global memory that the workgroup's waves hand to each other across barriers
struct Agent {
  double* s;
  __device__ double ld(int e) const { return __hip_atomic_load(s + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void st(int e, double v) const { __hip_atomic_store(s + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// (key, index) pairs in two arrays, ordered by key and then by index
struct KeyIdx {
  u64 key;
  unsigned idx;
  __device__ bool operator>(const KeyIdx& o) const { return key > o.key || (key == o.key && idx > o.idx); }
};
struct KeyIdxRows {
  u64* key;
  unsigned* idx;
  __device__ KeyIdx ld(int e) const { return KeyIdx{key[e], idx[e]}; }
  __device__ void st(int e, KeyIdx v) const { key[e] = v.key; idx[e] = v.idx; }
};
struct Greater {
  template <class T>
  __device__ bool operator()(const T& a, const T& b) const { return a > b; }
};

// The exchanges at distances j_from, j_from / 2, .. down to j_to (>= 1) of merge step k of a bitonic network over rows of NP
// elements (a power of two; ascending in the end).  `a` holds `count` elements (a multiple of 2 j_from), element e being
// element base + e of the rows laid end to end: a pair's direction follows from that index.  Pair pr of a distance exchanges
// e and e | j, the pairs of one distance being disjoint.  The elements must be visible to the workgroup on entry (a barrier
// after they were written); a barrier follows every distance.
template <int NT, class Acc, class Gt = Greater>
__device__ __forceinline__ void bitonic_steps(Acc a, int count, int NP, int base, int k, int j_from, int j_to, Gt gt = Gt()) {
  const int tid = threadIdx.x, half = count / 2, km = k & (NP - 1);     // k = NP: every pair of a row ascends
  for (int j = j_from; j >= j_to; j >>= 1) {
    for (int pr = tid; pr < half; pr += NT) {
      const int e = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), f = e | j;
      const bool up = ((base + e) & km) == 0;
      const auto x = a.ld(e), y = a.ld(f);
      if (gt(x, y) == up) { a.st(e, y); a.st(f, x); }
    }
    __syncthreads();
  }
}

// the whole network over `rows` rows of NP elements at once
template <int NT, class Acc, class Gt = Greater>
__device__ __forceinline__ void bitonic_sort(Acc a, int rows, int NP, Gt gt = Gt()) {
  for (int k = 2; k <= NP; k <<= 1) bitonic_steps<NT>(a, rows * NP, NP, 0, k, k >> 1, 1, gt);
}

// Quantile p of the sorted s.ld(0 .. T) by Armadillo's rule (arma::quantile: Hyndman & Fan definition 5): p_k = (k - 0.5) / N,
// linear in between, the extremes outside [0.5 / N, (N - 0.5) / N]
template <class Acc>
__device__ __forceinline__ double quantile5(Acc s, int T, double p) {
  const double N = (double)T;
  if (p < 0.5 / N) return s.ld(0);
  if (p > (N - 0.5) / N) return s.ld(T - 1);
  const int k = (int)floor(N * p + 0.5);
  const double pk = ((double)k - 0.5) / N, w = (p - pk) * N;
  return (1.0 - w) * s.ld(k - 1) + w * s.ld(min(k, T - 1));
}

}  // namespace rs
