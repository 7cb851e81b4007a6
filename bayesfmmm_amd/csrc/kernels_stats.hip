// B-spline basis evaluation S(t) and per-curve sufficient statistics (setup kernels).
//
// Replaces splines2::BSpline(t_i, internal_knots, degree, boundary_knots).basis(true) at
// BFMMM.h:1017-1025 / 1188-1196 / 1392-1400 and UserFunctions.cpp:289-299, and precomputes what
// every Update*.h loop nest re-derives per observation: G_i = B_i'B_i, s_i = B_i'y_i, yy_i = y_i'y_i.
//
// One 64-lane workgroup per curve.  Observations are processed in chunks: phase 1 evaluates the
// degree+1 non-zero basis functions of each point by the Cox-de Boor triangle and parks them in
// LDS; phase 2 gives every band element of G_i (and every s_p) to one lane, which accumulates
// over the chunk in observation order -- a fixed summation order, so results are reproducible.
#include "model.hpp"
#include "launchers.hpp"

namespace bfmmm {

constexpr int CHUNK = 256;

struct SplineSpec {
  int degree;
  int n_internal;
  const double* knots;   // full clamped knot vector, n_internal + 2*(degree+1) entries (device)
};

template <int DEG>
__device__ inline int eval_basis(double xv, const double* __restrict__ knots, int P, double N[DEG + 1]) {
  // knot span: largest j in [DEG, P-1] with knots[j] <= x; x == right boundary falls in the last interval
  int lo = DEG, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (knots[mid] <= xv) lo = mid; else hi = mid - 1;
  }
  const int j = lo;
  N[0] = 1.0;
#pragma unroll
  for (int d = 1; d <= DEG; ++d) {
    double saved = 0.0;
#pragma unroll
    for (int q = 0; q < d; ++q) {
      const double right = knots[j + q + 1] - xv;
      const double left = xv - knots[j + 1 - d + q];
      const double denom = right + left;
      const double nq = N[q];
      const double temp = (denom != 0.0) ? nq / denom : 0.0;
      // where one difference is 0 the other's weight is denom / denom = 1: N[q] is handed on as it is (x (1 / x) can be
      // 1 - 2^-53), so that B(b0)[0] = B(b1)[P - 1] = 1.0 bit for bit; 0 / 0 = 0 stays
      N[q] = (left == 0.0 && right != 0.0) ? saved + nq : saved + right * temp;
      saved = (right == 0.0 && left != 0.0) ? nq : left * temp;
    }
    N[d] = saved;
  }
  return j - DEG;   // index of the first non-zero basis function
}

// Functional model: rec_i from (t_i, y_i).  Optionally also writes the dense basis rows
// (row-major, P per observation) that the reference returns to the user as "B".
template <int DEG>
__global__ __launch_bounds__(64) void k_stats_functional(int n, int P, int LREC, const int64_t* __restrict__ off,
                                                         const double* __restrict__ t, const double* __restrict__ y,
                                                         const double* __restrict__ knots, int n_knots,
                                                         double* __restrict__ rec, int* __restrict__ ni_out,
                                                         double* __restrict__ B_dense, int* __restrict__ err) {
  __shared__ double sk[PMAX + 2 * (BWMAX + 1)];
  __shared__ double sN[CHUNK][DEG + 1];
  __shared__ int sFirst[CHUNK];
  __shared__ double sY[CHUNK];
  const int i = blockIdx.x;
  const int lane = threadIdx.x;
  for (int q = lane; q < n_knots; q += 64) sk[q] = knots[q];
  __syncthreads();
  const int64_t o0 = off[i];
  const int ni = (int)(off[i + 1] - o0);
  const int LG = (DEG + 1) * P;
  const double b0 = sk[0], b1 = sk[n_knots - 1];
  // every lane owns up to ceil((LG + P + 1) / 64) outputs
  constexpr int OWN = ((BWMAX + 1) * PMAX + PMAX + 1 + 63) / 64;
  double acc[OWN];
#pragma unroll
  for (int q = 0; q < OWN; ++q) acc[q] = 0.0;
  for (int c0 = 0; c0 < ni; c0 += CHUNK) {
    const int cn = min(CHUNK, ni - c0);
    for (int l = lane; l < cn; l += 64) {
      const double xv = t[o0 + c0 + l];
      double N[DEG + 1];
      int first = 0;
      if (!(xv >= b0 && xv <= b1)) {
        atomicOr(err, 1);
#pragma unroll
        for (int q = 0; q <= DEG; ++q) N[q] = 0.0;
      } else {
        first = eval_basis<DEG>(xv, sk, P, N);
      }
#pragma unroll
      for (int q = 0; q <= DEG; ++q) sN[l][q] = N[q];
      sFirst[l] = first;
      sY[l] = y[o0 + c0 + l];
      if (B_dense) {
        double* row = B_dense + (size_t)(o0 + c0 + l) * P;
        for (int p = 0; p < P; ++p) row[p] = 0.0;
#pragma unroll
        for (int q = 0; q <= DEG; ++q) row[first + q] = N[q];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < OWN; ++q) {
      const int e = lane + 64 * q;
      if (e < LG) {
        const int d = e / P, p = e - d * P;
        if (p + d < P) {
          double a = acc[q];
          for (int l = 0; l < cn; ++l) {
            const int f = sFirst[l];
            const int ia = p - f, ib = p + d - f;
            if (ia >= 0 && ib <= DEG) a += sN[l][ia] * sN[l][ib];
          }
          acc[q] = a;
        }
      } else if (e < LG + P) {
        const int p = e - LG;
        double a = acc[q];
        for (int l = 0; l < cn; ++l) {
          const int ia = p - sFirst[l];
          if (ia >= 0 && ia <= DEG) a += sN[l][ia] * sY[l];
        }
        acc[q] = a;
      } else if (e == LG + P) {
        double a = acc[q];
        for (int l = 0; l < cn; ++l) a += sY[l] * sY[l];
        acc[q] = a;
      }
    }
    __syncthreads();
  }
  double* r = rec + (size_t)i * LREC;
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int e = lane + 64 * q;
    if (e < LREC) r[e] = (e <= LG + P) ? acc[q] : 0.0;
  }
  if (lane == 0) ni_out[i] = ni;
}

// Multivariate model (BMVMMM_*): B_i = I, so G_i = I (band width 0), s_i = y_i, yy_i = y_i'y_i.
// Y is the N x P column-major matrix of UserFunctions.cpp:4579.
__global__ __launch_bounds__(64) void k_stats_multivariate(int n, int P, int LREC, const double* __restrict__ Y,
                                                           double* __restrict__ rec, int* __restrict__ ni_out) {
  const int i = blockIdx.x;
  const int lane = threadIdx.x;
  double* r = rec + (size_t)i * LREC;
  double yy = 0.0;
  for (int p = lane; p < P; p += 64) {
    const double v = Y[i + (size_t)n * p];
    r[p] = 1.0;
    r[P + p] = v;
  }
  if (lane == 0) {
    for (int p = 0; p < P; ++p) { const double v = Y[i + (size_t)n * p]; yy += v * v; }
    r[2 * P] = yy;
    for (int e = 2 * P + 1; e < LREC; ++e) r[e] = 0.0;
    ni_out[i] = P;
  }
}

// sum_i yy_i, sum_i n_i, sum_i floor(n_i/2) in a fixed order (single workgroup, setup only)
__global__ __launch_bounds__(256) void k_stats_totals(int n, int LREC, int yy_off, const double* __restrict__ rec,
                                                      const int* __restrict__ ni, double* __restrict__ out_yy,
                                                      long long* __restrict__ out_counts) {
  __shared__ double sy[256];
  __shared__ long long sn[256], sh[256];
  const int tid = threadIdx.x;
  double a = 0.0;
  long long cn = 0, ch = 0;
  // contiguous chunk per thread -> fixed order
  const int per = (n + 255) / 256;
  for (int i = tid * per; i < min(n, (tid + 1) * per); ++i) {
    a += rec[(size_t)i * LREC + yy_off];
    cn += ni[i];
    ch += ni[i] / 2;
  }
  sy[tid] = a; sn[tid] = cn; sh[tid] = ch;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0; long long c1 = 0, c2 = 0;
    for (int q = 0; q < 256; ++q) { s += sy[q]; c1 += sn[q]; c2 += sh[q]; }
    *out_yy = s; out_counts[0] = c1; out_counts[1] = c2;
  }
}

// ---- host launchers -------------------------------------------------------------------------
int launch_stats_functional(int degree, int n, int P, int LREC, const int64_t* off, const double* t, const double* y,
                            const double* knots, int n_knots, double* rec, int* ni, double* B_dense, int* err,
                            hipStream_t st) {
  dim3 g(n), b(64);
  switch (degree) {
    case 1: hipLaunchKernelGGL(k_stats_functional<1>, g, b, 0, st, n, P, LREC, off, t, y, knots, n_knots, rec, ni, B_dense, err); break;
    case 2: hipLaunchKernelGGL(k_stats_functional<2>, g, b, 0, st, n, P, LREC, off, t, y, knots, n_knots, rec, ni, B_dense, err); break;
    case 3: hipLaunchKernelGGL(k_stats_functional<3>, g, b, 0, st, n, P, LREC, off, t, y, knots, n_knots, rec, ni, B_dense, err); break;
    case 4: hipLaunchKernelGGL(k_stats_functional<4>, g, b, 0, st, n, P, LREC, off, t, y, knots, n_knots, rec, ni, B_dense, err); break;
    case 5: hipLaunchKernelGGL(k_stats_functional<5>, g, b, 0, st, n, P, LREC, off, t, y, knots, n_knots, rec, ni, B_dense, err); break;
    default: return 1;
  }
  return 0;
}

void launch_stats_multivariate(int n, int P, int LREC, const double* Y, double* rec, int* ni, hipStream_t st) {
  hipLaunchKernelGGL(k_stats_multivariate, dim3(n), dim3(64), 0, st, n, P, LREC, Y, rec, ni);
}

void launch_stats_totals(int n, int LREC, int yy_off, const double* rec, const int* ni, double* out_yy,
                         long long* out_counts, hipStream_t st) {
  hipLaunchKernelGGL(k_stats_totals, dim3(1), dim3(256), 0, st, n, LREC, yy_off, rec, ni, out_yy, out_counts);
}

}  // namespace bfmmm
