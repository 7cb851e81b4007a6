// Contrasts of cluster mean functions and covariate effects from chain slots.  For every chain q, slot t and contrast
// r, with cs = q S + (t - first_slot), A = mix[cs] the draw's K x K label map (a transform of the rescale step, or the permutation
// matrix of its row of perm) and the weights Wnu[r, k], Weta[r, k, d] of the contrast,
//     a_c    = sum_k Wnu[r, k] A[k][c]              a'_cd = sum_k Weta[r, k, d] A[k][c]              (k in order from 0.0)
//     b_r[p] = sum_c ( a_c nu_c,p + sum_d a'_cd eta_c,p,d )                                            (c, then d, in order from 0.0)
//     v_r(g) = sum_p E_gp b_r[p]                                                                       (p in order from 0.0)
// one rounding per product and per sum.  The kernels only form the values, V[cs + N (e - r0)] of result rows e = r G + g of a chunk
// [r0, r0 + rows), N = C S (the layout of k_ccov_values with `diagonal`: launch_ccov_maxdev takes the rows as they are), the size
// of every contrast per draw and counts over rows; mean, sd, quantiles, the seven statistics and crit are the launchers of
// kernels_bands.hip, kernels_diag.hip and kernels_cluster_cov.hip on those rows, as they are.
//
//   k_contrast_coef    Once per call: a thread owns one draw of one contrast.  It reads the draw's A and forms the K (1 + D) mixed
//                      weights a_c, a'_cd into its column of an LDS table (entry-major: the 64 lanes of the wave on 64 consecutive
//                      doubles, no bank conflict, any index), then walks p and writes b_r[p] to tab[(r P + p) N + cs], draw-fastest:
//                      consecutive lanes write consecutive doubles.  The mixing is done here and nowhere else, K (1 + D) products
//                      per (draw, contrast, p), where k_rescale_project redoes it for every grid point.
//   k_contrast_values  A thread owns one draw of one result row: v = sum_p E_gp tab[(r P + p) N + cs], plain multiplies and
//                      additions, p ascending from 0.0.  The loads of a wave are 64 consecutive doubles for every p, the row of E is
//                      uniform over the workgroup.
//   k_contrast_norm    A thread owns one (contrast, draw): acc += w_g (v v) over the chunk's rows of the contrast, g ascending, so
//                      over a call's chunks in ascending order the sum is that of g = 0 .. G - 1 whatever the chunking; the chunk
//                      that holds row G - 1 of the contrast replaces the sum by its square root.
//   k_rows_count       One workgroup per row of N values: how many are > thr[row] (or >=), integers summed over the lanes by a
//                      butterfly and over the four waves in LDS.  Serves prob_positive (thr 0, >) and p_sim (thr t_r, >= on dev).
// A value's bits depend on (draw, contrast, g) alone, and a contrast's coefficients on its own weights alone: the results do not
// depend on the chunk, on repeated calls, or on which other contrasts the call holds.  With A a permutation matrix and Wnu = e_k
// every mixing sum is 1 v + 0 w + .., exact, and the sum over p is k_align_project's: the values are those of
// bfmmm_chain_cluster_mean_bands bit for bit (but for the sign of a zero).  Vector stores only, no atomics, no scratch.
#include "model.hpp"
#include "launchers.hpp"

#include <string>

// one rounding per product and per sum, as the restatement's bound assumes
#pragma clang fp contract(off)

namespace bfmmm {

namespace {

constexpr int CT_DMAX = 8;
constexpr int CT_RMAX = 64;
constexpr int CT_CT = 64;                           // threads of k_contrast_coef: one wave
constexpr int CT_NW = KMAX * (1 + CT_DMAX);         // mixed weights of a (draw, contrast)
constexpr int CT_NT = 256;

// grid (blocks of 64 draws, R)
__global__ __launch_bounds__(CT_CT) void k_contrast_coef(const double* c_nu, size_t chain_bytes, const double* c_eta, size_t chain_bytes_cov,
                                                         const double* mix, const double* w_nu, const double* w_eta, int K, int P, int D,
                                                         int DX, int first_slot, int S, long long N, double* tab) {
  __shared__ double sW[CT_NW][CT_CT];      // [c]: a_c, [K + c DX + d]: a'_cd, of the thread's draw
  const int tid = threadIdx.x, r = (int)blockIdx.y;
  const long long cs = (long long)blockIdx.x * CT_CT + tid;
  if (cs >= N) return;                     // no barrier below: a thread reads only its own column of sW
  const int q = (int)(cs / S), s = (int)(cs - (long long)q * S);
  const double* nu = ptr_shift(c_nu, (size_t)q * chain_bytes) + (size_t)(first_slot + s) * ((size_t)K * P);      // nu: [c + K p]
  const double* eta = DX > 0 ? ptr_shift(c_eta, (size_t)q * chain_bytes_cov) + (size_t)(first_slot + s) * ((size_t)P * D * K) : nullptr;
  const double* A = mix + (size_t)cs * K * K;
  const double* wn = w_nu + (size_t)r * K;
  const double* we = DX > 0 ? w_eta + (size_t)r * K * D : nullptr;
  for (int c = 0; c < K; ++c) {
    double a = 0.0;
    for (int k = 0; k < K; ++k) a += wn[k] * A[k * K + c];
    sW[c][tid] = a;
    for (int d = 0; d < DX; ++d) {
      double ad = 0.0;
      for (int k = 0; k < K; ++k) ad += we[k * D + d] * A[k * K + c];
      sW[K + c * DX + d][tid] = ad;
    }
  }
  double* out = tab + (size_t)r * P * (size_t)N + (size_t)cs;
  for (int p = 0; p < P; ++p) {
    double b = 0.0;
    for (int c = 0; c < K; ++c) {
      b += sW[c][tid] * nu[c + (size_t)K * p];
      for (int d = 0; d < DX; ++d) b += sW[K + c * DX + d][tid] * eta[p + (size_t)P * (d + (size_t)D * c)];      // eta: [p + P (d + D c)]
    }
    out[(size_t)p * (size_t)N] = b;
  }
}

// grid (blocks of 256 draws, rows of the chunk): row e = r0 + blockIdx.y = r G + g
__global__ __launch_bounds__(CT_NT) void k_contrast_values(const double* tab, const double* E, int G, int P, long long N, long long r0, double* V) {
  const long long cs = (long long)blockIdx.x * CT_NT + threadIdx.x;
  if (cs >= N) return;
  const long long e = r0 + (long long)blockIdx.y;
  const int r = (int)(e / G), g = (int)(e - (long long)r * G);
  const double* eg = E + (size_t)g * P;
  const double* b = tab + (size_t)r * P * (size_t)N + (size_t)cs;
  double v = 0.0;
  for (int p = 0; p < P; ++p) v += eg[p] * b[(size_t)p * (size_t)N];
  V[(size_t)cs + (size_t)N * blockIdx.y] = v;
}

// contrasts [rp0, rp0 + npc) of the call, the ones with rows in the chunk [r0, r0 + rows)
__global__ __launch_bounds__(CT_NT) void k_contrast_norm(const double* V, long long N, long long r0, long long rows, int G, long long rp0,
                                                         long long npc, const double* w, double* acc) {
  const long long idx = (long long)blockIdx.x * CT_NT + threadIdx.x;
  if (idx >= npc * N) return;
  const long long pr = idx / N, cs = idx - pr * N, r = rp0 + pr;
  const long long lo = max(r0, r * G), hi = min(r0 + rows, (r + 1) * G);
  double a = acc[(size_t)r * N + cs];
  for (long long e = lo; e < hi; ++e) {
    const double v = V[(size_t)cs + (size_t)N * (size_t)(e - r0)];
    const double t = v * v;
    a += w[e - r * G] * t;
  }
  acc[(size_t)r * N + cs] = hi == (r + 1) * G ? sqrt(a) : a;
}

// one workgroup per row
__global__ __launch_bounds__(CT_NT) void k_rows_count(const double* V, long long N, const double* thr, int ge, int32_t* count) {
  __shared__ int sC[CT_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* row = V + (size_t)blockIdx.x * (size_t)N;
  const double t = thr ? thr[blockIdx.x] : 0.0;
  int n = 0;
  for (long long cs = tid; cs < N; cs += CT_NT) {
    const double v = row[cs];
    n += (ge ? v >= t : v > t) ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if (lane == 0) sC[wave] = n;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < CT_NT / 64; ++w) tot += sC[w];
    count[blockIdx.x] = tot;
  }
}

}  // namespace

std::string contrast_check(const Ctx& c, const ContrastCall& f) {
  const Dims& d = c.d;
  if (d.K < 1 || d.K > KMAX) return "K outside 1 .. 8";
  if (d.P < 1) return "P below 1";
  if (f.G < 1) return "G below 1";
  if (f.R < 1 || f.R > CT_RMAX) return "R outside 1 .. 64";
  if (f.w_eta && (d.D < 1 || d.D > CT_DMAX || !c.c_eta)) return "w_eta without covariates, or more than 8 of them";
  if (f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "range outside the chain storage";
  if ((long long)c.nch * f.n_slots > (1LL << 22)) return "more than 2^22 draws";
  return "";
}

std::string launch_contrast_coef(const Ctx& c, const ContrastCall& f, hipStream_t st) {
  const std::string bad = contrast_check(c, f);
  if (!bad.empty()) return "k_contrast_coef: " + bad;
  if (!f.mix || !f.w_nu || !f.tab) return "k_contrast_coef: bad arguments";
  const Dims& d = c.d;
  const long long N = (long long)c.nch * f.n_slots;
  hipLaunchKernelGGL(k_contrast_coef, dim3((unsigned)((N + CT_CT - 1) / CT_CT), (unsigned)f.R), dim3(CT_CT), 0, st, c.c_nu, c.chain_bytes,
                     f.w_eta ? c.c_eta : (const double*)nullptr, c.chain_bytes_cov, f.mix, f.w_nu, f.w_eta, d.K, d.P, d.D, f.w_eta ? d.D : 0,
                     f.first_slot, f.n_slots, N, f.tab);
  if (hipGetLastError() != hipSuccess) return "k_contrast_coef: launch failed";
  return "";
}

std::string launch_contrast_values(const Ctx& c, const ContrastCall& f, long long r0, long long rows, double* V, hipStream_t st) {
  const std::string bad = contrast_check(c, f);
  if (!bad.empty()) return "k_contrast_values: " + bad;
  if (!f.E || !f.tab || !V || r0 < 0 || rows < 1 || rows > 65535 || r0 + rows > (long long)f.R * f.G) return "k_contrast_values: bad arguments";
  const long long N = (long long)c.nch * f.n_slots;
  hipLaunchKernelGGL(k_contrast_values, dim3((unsigned)((N + CT_NT - 1) / CT_NT), (unsigned)rows), dim3(CT_NT), 0, st, f.tab, f.E, f.G, c.d.P, N,
                     r0, V);
  if (hipGetLastError() != hipSuccess) return "k_contrast_values: launch failed";
  return "";
}

std::string launch_contrast_norm(const Ctx& c, const ContrastCall& f, long long r0, long long rows, const double* V, double* acc, hipStream_t st) {
  const std::string bad = contrast_check(c, f);
  if (!bad.empty()) return "k_contrast_norm: " + bad;
  if (!f.w || !V || !acc || r0 < 0 || rows < 1 || r0 + rows > (long long)f.R * f.G) return "k_contrast_norm: bad arguments";
  const long long N = (long long)c.nch * f.n_slots;
  const long long rp0 = r0 / f.G, npc = (r0 + rows - 1) / f.G - rp0 + 1;
  const long long blocks = (npc * N + CT_NT - 1) / CT_NT;
  if (blocks > 0x7fffffffLL) return "k_contrast_norm: too many workgroups in one chunk";
  hipLaunchKernelGGL(k_contrast_norm, dim3((unsigned)blocks), dim3(CT_NT), 0, st, V, N, r0, rows, f.G, rp0, npc, f.w, acc);
  if (hipGetLastError() != hipSuccess) return "k_contrast_norm: launch failed";
  return "";
}

std::string launch_rows_count(const double* V, long long N, long long rows, const double* thr, int ge, int32_t* count, hipStream_t st) {
  if (!V || !count || N < 1 || N > 0x7fffffffLL || rows < 1 || rows > 0x7fffffffLL) return "k_rows_count: bad arguments";
  hipLaunchKernelGGL(k_rows_count, dim3((unsigned)rows), dim3(CT_NT), 0, st, V, N, thr, ge ? 1 : 0, count);
  if (hipGetLastError() != hipSuccess) return "k_rows_count: launch failed";
  return "";
}

}  // namespace bfmmm
