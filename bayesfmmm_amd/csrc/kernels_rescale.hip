// The reference's `rescale` step on chain slots (src/PostProcessing.cpp:204-218 of the reference): a mixed-membership
// model is identified only up to an invertible K x K map of the simplex, and the reference reports every cluster-level quantity
// after the map that makes the purest curve of every component a vertex.  Per draw cs = q S + s, with A the K x K transform whose
// row k (aligned component) holds the memberships of that curve over the raw components c,
//     Z~ = Z A^-1,      nu~_k = sum_c A[k][c] nu_c      (and the same sum for Phi, eta, xi),      Z~ nu~ = Z nu.
//
//   k_rescale_transform  One workgroup of 256 threads per draw.  Rule mode: a thread walks i = tid, tid + 256, .. down the columns
//                        of Z (i-fastest: the reads coalesce) and keeps, for every raw component, the largest entry and its curve
//                        -- a later entry replaces it only where it is > (never >=), so a thread holds its smallest maximiser.
//                        Pairs (value, curve) then meet by a butterfly over the lanes and in wave order from LDS under one rule,
//                        "larger value, or the same value and the smaller curve", which is symmetric: every lane ends with the
//                        same pair, the smallest i that attains the maximum, whatever the grid (arma::index_max).  An entry that
//                        is NaN is never the maximum; a column without any entry above -inf takes curve 0.  curve[k] is the
//                        curve of raw component perm[k], A[k][c] = Z[curve[k], c], copied, so exact.  Given mode: A is the
//                        caller's, curve = -1.  Then thread 0 inverts A in LDS by Gauss-Jordan elimination on [A | I]:
//                            for j = 0 .. K - 1:  p = the smallest r >= j that attains max |a[r][j]|  (>, never >=)
//                                                 pivot a[p][j] == 0 (or A not finite, or, under the rule, two components
//                                                 with the same curve: two equal rows): the draw is singular
//                                                 rows j and p change places;  row j /= pivot  (entry by entry, columns in order)
//                                                 for r = 0 .. K - 1, r != j:  f = a[r][j];  row r -= f * row j
//                        a product and a difference rounded once each (contraction off), so repeated calls give the same bits.
//                        rcond = 1 / (|A|_1 |A^-1|_1), column sums in the order of the rows.  A singular draw gets A^-1 = NaN,
//                        rcond = 0 and z_min = NaN.  z_min = min_{i,k} sum_c Z[i, c] Ainv[c][k] (c in order from 0) is a second
//                        pass over the slot; a minimum is exact and order-free, and a NaN among the rescaled memberships is kept
//                        (the rule of k_ccov_maxdev), as the restatement's z_min keeps it.  singular_flag[cs] says which draws
//                        are singular: rcond alone would not, 1 / (|A|_1 |A^-1|_1) of a finite inverse can underflow to 0.
//   k_rescale_gather     k_align_gather with a sum in place of the index: element e = a + inner (k + K b) of the row is
//                        sum_c w_c src[a + inner (c + K b)], c = 0 .. K - 1 in order from 0.0, w_c = W[cs K K + k sk + c sc]:
//                        (sk, sc) = (K, 1) reads row k of A (nu, Phi, eta, xi), (1, K) column k of A^-1 (Z).
//   k_rescale_project    v[(k + K g)][cs] = sum_p E_gp sum_c A[k][c] (nu_c,p + sum_d x_d eta_c,p,d), p, c and d in order from 0:
//                        k_align_project's sum over p with the mixed coefficient in place of the indexed one.
// With A a permutation matrix every sum is 1 v + 0 w + .., exact: the results are those of the permutation kernels bit for bit
// (but for the sign of a zero).  No atomics, no scratch.
#include "model.hpp"
#include "launchers.hpp"

#include <string>

// one rounding per product and per sum, as the restatement's bounds assume
#pragma clang fp contract(off)

namespace bfmmm {

namespace {

constexpr int RS_NT = 256;
constexpr int RS_WAVES = RS_NT / 64;
constexpr int RS_DMAX = 8;
constexpr int RS_NONE = 0x7fffffff;      // the curve of a pair that holds no entry yet

// (v, i) takes (w, j) where w is larger, or equal with the smaller curve
__device__ inline void rs_take(double& v, int& i, double w, int j) {
  if (w > v || (w == v && j < i)) { v = w; i = j; }
}

template <int KP>
__global__ __launch_bounds__(RS_NT) void k_rescale_transform(const double* c_Z, size_t chain_bytes, int n, int K, int first_slot, int S,
                                                             const int32_t* perm, const double* given, double* mix, double* mix_inv,
                                                             int32_t* curve, double* rcond, double* z_min, int32_t* singular_flag) {
  __shared__ double sV[RS_WAVES][KP];
  __shared__ int sI[RS_WAVES][KP];
  __shared__ int sCurve[KP];              // of the raw components
  __shared__ int sAl[KP];                 // of the aligned ones
  __shared__ double sM[KP][2 * KP];       // [A | I], then [I | A^-1]
  __shared__ double sInv[KP][KP];         // A^-1[c][k]
  __shared__ double sMin[RS_WAVES];
  __shared__ int sSingular;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t cs = blockIdx.x;
  const int q = (int)(blockIdx.x / (unsigned)S), s = (int)(blockIdx.x - (unsigned)q * (unsigned)S);
  const double* Z = ptr_shift(c_Z, (size_t)q * chain_bytes) + (size_t)(first_slot + s) * ((size_t)n * K);
  if (!given) {
    double bv[KP];
    int bi[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) { bv[c] = -INFINITY; bi[c] = RS_NONE; }
    for (int i = tid; i < n; i += RS_NT) {
#pragma unroll
      for (int c = 0; c < KP; ++c)
        if (c < K) {
          const double z = Z[(size_t)c * n + i];
          if (z > bv[c]) { bv[c] = z; bi[c] = i; }
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      for (int off = 32; off > 0; off >>= 1) {
        const double w = __shfl_xor(bv[c], off, 64);
        const int j = __shfl_xor(bi[c], off, 64);
        rs_take(bv[c], bi[c], w, j);
      }
      if (lane == 0) { sV[wave][c] = bv[c]; sI[wave][c] = bi[c]; }
    }
    __syncthreads();
    if (tid < K) {
      double v = sV[0][tid];
      int i = sI[0][tid];
      for (int w = 1; w < RS_WAVES; ++w) rs_take(v, i, sV[w][tid], sI[w][tid]);
      sCurve[tid] = i == RS_NONE ? 0 : i;
    }
    __syncthreads();
  }
  if (tid < K * K) {
    const int k = tid / K, c = tid - k * K;
    double a;
    if (given) a = given[(cs * K + k) * K + c];
    else {
      const int ci = sCurve[perm ? perm[cs * K + k] : k];
      a = Z[(size_t)c * n + ci];
      if (c == 0) { curve[cs * K + k] = ci; sAl[k] = ci; }
    }
    if (given && c == 0) curve[cs * K + k] = -1;
    sM[k][c] = a;
    sM[k][KP + c] = k == c ? 1.0 : 0.0;
    mix[(cs * K + k) * K + c] = a;
  }
  __syncthreads();
  if (tid == 0) {
    bool singular = false;
    // two components with the same pure curve: two equal rows, singular whatever the elimination's roundings leave of them
    for (int k = 1; k < K && !given; ++k)
      for (int l = 0; l < k; ++l)
        if (sAl[k] == sAl[l]) singular = true;
    double n1 = 0.0;                      // |A|_1: the largest column sum
    for (int c = 0; c < K; ++c) {
      double sum = 0.0;
      for (int r = 0; r < K; ++r) {
        const double a = sM[r][c];
        if (!(fabs(a) <= 1.79769313486231570815e308)) singular = true;      // not finite
        sum += fabs(a);
      }
      if (sum > n1) n1 = sum;
    }
    for (int j = 0; j < K && !singular; ++j) {
      int p = j;
      double big = fabs(sM[j][j]);
      for (int r = j + 1; r < K; ++r)
        if (fabs(sM[r][j]) > big) { big = fabs(sM[r][j]); p = r; }
      const double piv = sM[p][j];
      if (piv == 0.0 || piv != piv) { singular = true; break; }
      for (int e = 0; e < K; ++e) {
        const int col0 = e, col1 = KP + e;
        const double t0 = sM[j][col0], t1 = sM[j][col1];
        sM[j][col0] = sM[p][col0] / piv; sM[j][col1] = sM[p][col1] / piv;
        if (p != j) { sM[p][col0] = t0; sM[p][col1] = t1; }
      }
      for (int r = 0; r < K; ++r)
        if (r != j) {
          const double f = sM[r][j];
          for (int e = 0; e < K; ++e) {
            sM[r][e] = sM[r][e] - f * sM[j][e];
            sM[r][KP + e] = sM[r][KP + e] - f * sM[j][KP + e];
          }
        }
    }
    double ni = 0.0;
    for (int k = 0; k < K; ++k) {
      double sum = 0.0;
      for (int c = 0; c < K; ++c) {
        const double v = singular ? NAN : sM[c][KP + k];
        sInv[c][k] = v;
        sum += fabs(v);
      }
      if (sum > ni) ni = sum;
    }
    sSingular = singular ? 1 : 0;
    rcond[cs] = singular ? 0.0 : 1.0 / (n1 * ni);
    singular_flag[cs] = singular ? 1 : 0;
  }
  __syncthreads();
  if (tid < K * K) {
    const int c = tid / K, k = tid - c * K;
    mix_inv[(cs * K + c) * K + k] = sInv[c][k];
  }
  if (sSingular) {
    if (tid == 0) z_min[cs] = NAN;
    return;
  }
  double inv[KP][KP];
#pragma unroll
  for (int c = 0; c < KP; ++c)
#pragma unroll
    for (int k = 0; k < KP; ++k) inv[c][k] = (c < K && k < K) ? sInv[c][k] : 0.0;
  double mn = INFINITY;
  for (int i = tid; i < n; i += RS_NT) {
    double z[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) z[c] = c < K ? Z[(size_t)c * n + i] : 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < KP; ++c)
          if (c < K) v += z[c] * inv[c][k];
        if (v < mn || v != v) mn = v;      // a NaN is kept
      }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double w = __shfl_xor(mn, off, 64);
    if (w < mn || w != w) mn = w;
  }
  if (lane == 0) sMin[wave] = mn;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < RS_WAVES; ++w)
      if (sMin[w] < mn || sMin[w] != sMin[w]) mn = sMin[w];
    z_min[cs] = mn;
  }
}

// ws[s + S (c + C p)] = chain c's slot (first + s), element p0 + p mixed over its component axis by the draw's weights; tiles as in
// k_align_gather
__global__ __launch_bounds__(256) void k_rescale_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S,
                                                        int C, int p0, int P, const double* W, int sk, int sc, int K, long long inner,
                                                        double* ws) {
  __shared__ double tile[32][33];
  const int tiles_s = (S + 31) / 32;
  const int ts = (int)(blockIdx.x % (unsigned)tiles_s), tp = (int)(blockIdx.x / (unsigned)tiles_s), c = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double* src = (const double*)((const char*)base + (size_t)c * chain_bytes);
  for (int r = ty; r < 32; r += 8) {
    const int s = ts * 32 + r, p = tp * 32 + tx;
    if (s < S && p < P) {
      const long long e = (long long)p0 + p;
      const long long a = e % inner, kb = e / inner, k = kb % K, b = kb / K;
      const double* w = W + ((size_t)c * S + s) * K * K + (size_t)k * sk;
      const double* x = src + (long long)(first + s) * ss;
      double v = 0.0;
      for (int cc = 0; cc < K; ++cc) v += w[(size_t)cc * sc] * x[(a + inner * ((long long)cc + (long long)K * b)) * ps];
      tile[r][tx] = v;
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int p = tp * 32 + r, s = ts * 32 + tx;
    if (s < S && p < P) ws[(size_t)s + (size_t)S * ((size_t)c + (size_t)C * (size_t)p)] = tile[tx][r];
  }
}

// rows [r0, r0 + gridDim.y) of the table, row = k + K g: V[cs + CS (row - r0)], cs = q S + s; DX: the covariates that enter (0: nu alone)
__global__ __launch_bounds__(256) void k_rescale_project(const double* c_nu, size_t chain_bytes, const double* c_eta, size_t chain_bytes_cov,
                                                         const double* E, const double* mix, const double* x, int K, int P, int D, int DX,
                                                         int first_slot, int S, long long CS, int r0, double* V) {
  const long long cs = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cs >= CS) return;
  const int row = r0 + (int)blockIdx.y, g = row / K, k = row - g * K;
  const int q = (int)(cs / S), s = (int)(cs - (long long)q * S);
  const double* nu = ptr_shift(c_nu, (size_t)q * chain_bytes) + (size_t)(first_slot + s) * ((size_t)K * P);      // nu: [c + K p]
  const double* eta = DX > 0 ? ptr_shift(c_eta, (size_t)q * chain_bytes_cov) + (size_t)(first_slot + s) * ((size_t)P * D * K) : nullptr;
  const double* e = E + (size_t)g * P;
  double a[KMAX], xs[RS_DMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) a[c] = c < K ? mix[((size_t)cs * K + k) * K + c] : 0.0;
#pragma unroll
  for (int d = 0; d < RS_DMAX; ++d) xs[d] = d < DX ? x[d] : 0.0;
  double v = 0.0;
  for (int p = 0; p < P; ++p) {
    double m = 0.0;
#pragma unroll
    for (int c = 0; c < KMAX; ++c)
      if (c < K) {
        double t = nu[c + (size_t)K * p];
#pragma unroll
        for (int d = 0; d < RS_DMAX; ++d)
          if (d < DX) t += xs[d] * eta[p + (size_t)P * (d + (size_t)D * c)];      // eta: [p + P (d + D c)]
        m += a[c] * t;
      }
    v += e[p] * m;
  }
  V[(size_t)cs + (size_t)CS * blockIdx.y] = v;
}

std::string rescale_range(const char* kernel, const Ctx& c, int first_slot, int n_slots) {
  const std::string k = std::string(kernel) + ": ";
  if (c.d.K < 1 || c.d.K > KMAX) return k + "K outside 1 .. 8";
  if (n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return k + "range outside the chain storage";
  if ((long long)c.nch * n_slots > (1LL << 22)) return k + "more than 2^22 draws";
  return "";
}

}  // namespace

std::string launch_rescale_transform(const Ctx& c, const int32_t* perm, const double* given, int first_slot, int n_slots, double* mix,
                                     double* mix_inv, int32_t* curve, double* rcond, double* z_min, int32_t* singular_flag, hipStream_t st) {
  const std::string bad = rescale_range("k_rescale_transform", c, first_slot, n_slots);
  if (!bad.empty()) return bad;
  if (!mix || !mix_inv || !curve || !rcond || !z_min || !singular_flag) return "k_rescale_transform: an output is null";
  const Dims& d = c.d;
  if (d.n < 1) return "k_rescale_transform: no curves";
  const unsigned grid = (unsigned)((long long)c.nch * n_slots);
  if (d.K <= 4)
    hipLaunchKernelGGL((k_rescale_transform<4>), dim3(grid), dim3(RS_NT), 0, st, c.c_Z, c.chain_bytes, d.n, d.K, first_slot, n_slots, perm, given,
                       mix, mix_inv, curve, rcond, z_min, singular_flag);
  else
    hipLaunchKernelGGL((k_rescale_transform<8>), dim3(grid), dim3(RS_NT), 0, st, c.c_Z, c.chain_bytes, d.n, d.K, first_slot, n_slots, perm, given,
                       mix, mix_inv, curve, rcond, z_min, singular_flag);
  if (hipGetLastError() != hipSuccess) return "k_rescale_transform: launch failed";
  return "";
}

std::string launch_rescale_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S, int C, int p0, int P,
                                  const double* W, int sk, int sc, int K, long long inner, double* ws, hipStream_t st) {
  const long long tiles = (long long)((S + 31) / 32) * ((P + 31) / 32);
  if (tiles > 0x7fffffffLL || C > 65535) return "k_rescale_gather: grid too large";
  if (!base || !W || !ws || K < 1 || K > KMAX || inner < 1) return "k_rescale_gather: bad arguments";
  hipLaunchKernelGGL(k_rescale_gather, dim3((unsigned)tiles, 1, (unsigned)C), dim3(256), 0, st, base, chain_bytes, ss, ps, first, S, C, p0, P, W,
                     sk, sc, K, inner, ws);
  if (hipGetLastError() != hipSuccess) return "k_rescale_gather: launch failed";
  return "";
}

std::string launch_rescale_project(const Ctx& c, const double* E, int G, const double* mix, const double* x, int first_slot, int n_slots,
                                   int r0, int rows, double* V, hipStream_t st) {
  const std::string bad = rescale_range("k_rescale_project", c, first_slot, n_slots);
  if (!bad.empty()) return bad;
  const Dims& d = c.d;
  if (!E || !mix || !V || G < 1 || r0 < 0 || rows < 1 || rows > 65535 || (long long)r0 + rows > (long long)d.K * G)
    return "k_rescale_project: bad arguments";
  if (x && (d.D < 1 || !c.c_eta)) return "k_rescale_project: 'x' without covariates";
  if (x && d.D > RS_DMAX) return "k_rescale_project: more than 8 covariates";
  const long long CS = (long long)c.nch * n_slots;
  hipLaunchKernelGGL(k_rescale_project, dim3((unsigned)((CS + 255) / 256), (unsigned)rows), dim3(256), 0, st, c.c_nu, c.chain_bytes,
                     x ? c.c_eta : (const double*)nullptr, c.chain_bytes_cov, E, mix, x, d.K, d.P, d.D, x ? d.D : 0, first_slot, n_slots, CS, r0, V);
  if (hipGetLastError() != hipSuccess) return "k_rescale_project: launch failed";
  return "";
}

}  // namespace bfmmm
