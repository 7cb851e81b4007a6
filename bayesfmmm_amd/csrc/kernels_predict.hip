// Prediction of held-out curves from the chain slots: for a new curve with record (G, s, yy, n*) and covariates x,
// every chain q and slot t, the integral of the marginal density l(z) of kernels_curve_ll.hip over Z_new ~ Dir(alpha_3 pi) by staged
// importance sampling.  With the draw's directions theta_a, a = (k, mt) (mt = 0: nu_k + eta_k x, mt = m: phi_km + xi_km x), A = K (M + 1):
//     Gamma_ab = theta_a' G theta_b,  tau_a = theta_a' s                                   (once per curve and draw)
//     c'Gc = sum_kk' z_k z_k' Gamma_(k0)(k'0),  c's = sum_k z_k tau_(k0),  rr = yy - 2 c's + c'Gc,
//     u_m = sum_k z_k tau_(km) - sum_kk' z_k z_k' Gamma_(km)(k'0),  W_ml = sum_kk' z_k z_k' Gamma_(km)(k'l),  A = sigma^2 I_M + W,
//     l(z) = -1/2 [ n* log 2 pi + (n* - M) log sigma^2 + log det A + (rr - u'A^-1 u) / sigma^2 ]
// so that a value of l costs about K^2 (M + 1)(M + 2) / 2 multiply-adds on a table in LDS and an M x M Cholesky, whatever n* and P.
//
// Geometry.  One workgroup of 256 threads owns a new curve, a chain and a run of SCH slots; the band of G and s sit in LDS for the
// whole launch.  Per draw (pred_draw of predict_core.hpp, which k_predict_fit of kernels_predict_fit.hip runs too):
//   (1) theta directions-major [a PS + p] with x folded in, rows padded with zeros to AP = A rounded up to 16, columns to 4
//   (2) H = Theta G over the band window, tau_a (p in order)
//   (3) Gamma = Theta H' on v_mfma_f64_16x16x4_f64, the upper-triangle 16 x 16 tiles only, dealt to the four waves; lane l holds
//       A[row l & 15][k = 4 kb + (l >> 4)] and B[k][col l & 15] and receives D[row (l >> 4) + 4 reg][col l & 15] (the mapping of
//       k_ceig_solve); an off-diagonal tile is also stored transposed
//   (4) the R stages: one lane per sample (a loop where J > 256): the gamma variates of rng.hpp, z, l(z) from broadcast reads of
//       Gamma with the lane's M x M system in its own LDS column, then the stage's sums in a fixed tree (the lane's samples in order,
//       the wave by DPP and two shuffles, the four waves in order) and the next proposal by thread 0
// Gamma and tau never leave LDS.  fp64, no atomics; every sum's order depends on (J, R) and the lane count of the workgroup alone: a
// value's bits depend on (curve, chain, slot, seed, J, R), not on the chunk, the grid or a repeated call.
#include "model.hpp"
#include "launchers.hpp"
#include "predict_core.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

// KT: the compile-time bound on K (4 or KMAX), so that a lane's z stays in registers
template <int KT>
__global__ __launch_bounds__(PR_NT) void k_predict(PredArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const PredLds L = pred_lds(a.K, a.P, a.M, a.LG, a.J, KT);
  const int rr = blockIdx.x;                    // the curve's row in the chunk
  const int r = a.r0 + rr;                      // its position in the call
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const PredSlots ch = pred_slots(a, q_chain);
  double yy;
  int ni;
  pred_setup(a, L, sm, r, &yy, &ni);
  for (int s = s_lo; s < s_hi; ++s) pred_draw<KT>(a, L, sm, ch, r, rr, q_chain, s, yy, ni);
}

// One workgroup per row: lpd = log mean exp lpd_t by a max-shifted sum, the means of m, q and ess and the least ess, every sum in the
// order of block_sum (a thread's draws in order first)
__global__ __launch_bounds__(PR_NT) void k_predict_pool(int K, long long N, const double* lpd_t, const double* ess_t, const double* m_t,
                                                        const double* q_t, double* lpd, double* z_mean, double* z_sd, double* ess_mean,
                                                        double* ess_min) {
  __shared__ double sRed[4 * (2 + 2 * KMAX)];
  constexpr int NV = 2 + 2 * KMAX;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const double* lp = lpd_t + r * (size_t)N;
  const double* es = ess_t + r * (size_t)N;
  double mx = -INFINITY, mn = INFINITY;
  for (long long o = tid; o < N; o += PR_NT) { mx = fmax(mx, lp[o]); mn = fmin(mn, es[o]); }
  mx = block_extreme<true>(mx, sRed, lane, wave);
  mn = block_extreme<false>(mn, sRed, lane, wave);
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  for (long long o = tid; o < N; o += PR_NT) {
    v[0] += exp(lp[o] - mx);
    v[1] += es[o];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {          // (k >= K: a copy of k = K - 1 that nobody reads; the loads go out together)
      const size_t e = (r * (size_t)N + (size_t)o) * K + min(k, K - 1);
      v[2 + k] += m_t[e];
      v[2 + KMAX + k] += q_t[e];
    }
  }
  block_sum<NV>(v, sRed, lane, wave);
  if (tid == 0) {
    const double n = (double)N;
    lpd[r] = mx + log(v[0] / n);
    ess_mean[r] = v[1] / n;
    ess_min[r] = mn;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const double m = v[2 + k] / n;
        z_mean[r * K + k] = m;
        z_sd[r * K + k] = sqrt(fmax(v[2 + KMAX + k] / n - m * m, 0.0));
      }
  }
}

}  // namespace

std::string predict_check(const Ctx& c, const PredictCall& f, size_t* lds_bytes) {
  const Dims& d = c.d;
  if (d.P < 1 || d.P > PMAX) return "k_predict: P outside 1 .. 64";
  if (d.M < 1 || d.M > 16) return "k_predict: n_eigen outside 1 .. 16";
  if (d.K < 1 || d.K > KMAX) return "k_predict: K outside 1 .. 8";
  if (d.D < 0 || d.D > 8) return "k_predict: more than 8 covariates";
  if (d.BW < 0 || d.BW > BWWIDE) return "k_predict: band half-width above 31";
  if (c.nch < 1 || c.nch > 65535) return "k_predict: more than 65535 chains";
  if (f.J < 1 || f.R < 1 || f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "k_predict: range outside the chain storage";
  // J (K + 1) doubles of a stage's samples: beyond 2^24 samples nothing fits, whatever the rest
  const PredLds L = pred_lds(d.K, d.P, d.M, d.LG, std::min(f.J, 1 << 24), pred_kt(d.K));
  const size_t bytes = L.total * sizeof(double);
  if (lds_bytes) *lds_bytes = bytes;
  if (bytes > PR_LDS_HARD || f.J > (1 << 24))
    return "k_predict: the tables of a draw (Gamma of " + std::to_string(L.AP) + " x " + std::to_string(L.AP) + " for K (n_eigen + 1) = " +
           std::to_string(L.A) + " directions, the " + std::to_string((long long)f.J) + " x (K + 1) values of a stage's samples) need " +
           (f.J > (1 << 24) ? std::string("more than 1073741824") : std::to_string(bytes)) + " bytes of LDS, above the limit of " +
           std::to_string(PR_LDS_HARD) + " (160 KiB)";
  return "";
}

PredArgs pred_args(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t, double* prop,
                   double* samples, double* a_last) {
  const Dims& d = c.d;
  PredArgs a;
  a.c_nu = c.c_nu; a.c_Phi = c.c_Phi; a.c_sigma = c.c_sigma; a.c_pi = c.c_pi; a.c_alpha3 = c.c_alpha3;
  a.c_eta = d.D > 0 ? c.c_eta : nullptr; a.c_xi = d.D > 0 ? c.c_xi : nullptr;
  a.rec = f.rec; a.X = d.D > 0 ? f.X : nullptr; a.zs = f.zs; a.ni = f.ni; a.perm = f.perm;
  a.lpd_t = lpd_t; a.ess_t = ess_t; a.m_t = m_t; a.q_t = q_t; a.prop = prop; a.samples = samples;
  a.a_last = a_last; a.a_start = nullptr;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.seed = f.seed; a.chain0 = c.chain; a.chain_stride = c.chain_id_stride;
  a.n_new = f.n_new; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.BW = d.BW; a.LG = d.LG; a.LREC = d.LREC;
  a.cadj = (d.D > 0 && c.covariance_adj) ? 1 : 0;
  a.C = c.nch; a.first_slot = f.first_slot; a.S = f.n_slots; a.J = f.J; a.R = f.R; a.r0 = r0; a.rows = rows;
  // slots per workgroup: several workgroups per curve and chain while the grid stays below about eight per CU
  long long sch = ((long long)rows * c.nch * f.n_slots + 2047) / 2048;
  sch = std::max<long long>(1, std::min<long long>(sch, f.n_slots));
  while (((long long)f.n_slots + sch - 1) / sch > 65535) sch *= 2;
  a.SCH = (int)sch;
  return a;
}

std::string launch_predict(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                           double* prop, double* samples, hipStream_t st, double* a_last) {
  size_t lds = 0;
  const std::string bad = predict_check(c, f, &lds);
  if (!bad.empty()) return bad;
  if (rows < 1 || r0 < 0 || (long long)r0 + rows > f.n_new) return "k_predict: curves outside the call";
  if (!m_t != !q_t) return "k_predict: m_t and q_t go together";
  const PredArgs a = pred_args(c, f, r0, rows, lpd_t, ess_t, m_t, q_t, prop, samples, a_last);
  const dim3 grid((unsigned)rows, (unsigned)((f.n_slots + a.SCH - 1) / a.SCH), (unsigned)c.nch);
  void (*fn)(PredArgs) = pred_kt(c.d.K) == 4 ? k_predict<4> : k_predict<KMAX>;
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_predict: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, grid, dim3(PR_NT), lds, st, a);
  if (hipGetLastError() != hipSuccess) return "k_predict: launch failed";
  return "";
}

std::string launch_predict_pool(int K, long long N, int rows, const double* lpd_t, const double* ess_t, const double* m_t, const double* q_t,
                                double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min, hipStream_t st) {
  if (K < 1 || K > KMAX || N < 1 || rows < 1) return "k_predict_pool: bad shape";
  hipLaunchKernelGGL(k_predict_pool, dim3((unsigned)rows), dim3(PR_NT), 0, st, K, N, lpd_t, ess_t, m_t, q_t, lpd, z_mean, z_sd, ess_mean, ess_min);
  if (hipGetLastError() != hipSuccess) return "k_predict_pool: launch failed";
  return "";
}

}  // namespace bfmmm
