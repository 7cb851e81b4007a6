// The fitted function of held-out, partly observed curves from the chain slots: for a new curve, every chain q and
// slot t, after the stages of kernels_predict.hip (pred_draw of predict_core.hpp: the same keys, indices, summation trees and
// proposals, so lpd, ess and the memberships are k_predict's bit for bit), the predictive mean function, its variance and one
// sampled path on the G rows of an evaluation basis E (G x P).  Given a last-stage sample z_j the scores of the new curve are
//     chi | y_new, z_j, draw ~ N(A^-1 u, sigma^2 A^-1),   A = sigma^2 I_M + W = L L',  b = L^-1 u   (what pred_ell leaves in the lane's column)
// so with the table e_g,a = E_g . theta_a, a = (k, mt), of the draw (x folded in, as theta is):
//     c_j(g) = sum_k z_jk e_g,(k0),  v_j(g)_m = sum_k z_jk e_g,(km),  chi^_j = L^-T b,
//     mu_j(g) = c_j(g) + sum_m chi^_jm v_j(g)_m,  s_j(g) = sigma^2 |L^-1 v_j(g)|^2  (+ sigma^2 with noise),
//     mu_t(g) = sum_j w~_j mu_j(g),  v_t(g) = sum_j w~_j [ s_j(g) + (mu_j(g) - mu_t(g))^2 ]   (a second pass over j),  w~_j = w_j / sum w
// and the path: j* the first j with sum_{i <= j} w_i > U sum w (the sum in sample order), xi ~ N(0, I_M),
//     path(g) = c_j*(g) + sum_m (chi^_j* + sigma L^-T xi)_m v_j*(g)_m   (+ sigma eps_g with noise).
// Variates: key make_key(seed, RNG chain id, slot) as in 7m, update id UPD_PREDICT_FIT, index r (1 + M + G) + i with r the curve's
// position in the call: i = 0: U (runif), i = 1 + m: xi_m (rnorm), i = 1 + M + g: eps_g (rnorm).
// The draws are pooled with equal weights (the convention of Z_mean: the new curve does not reweight the parameter draws):
//     mean[r, g] = mean_cs mu_t(g),  sd[r, g] = sqrt( mean_cs v_t(g) + mean_cs (mu_t(g) - mean)^2 )   (two passes; k_predict_fit_pool)
// and the quantiles of the paths, written draw-fastest, come from launch_bands_quantiles.
//
// After the last stage of a draw (step numbers continue kernels_predict.hip's):
//   (5) e = E Theta' on v_mfma_f64_16x16x4_f64 with the operand mapping of step (3), G padded to 16, A operand read from E with zeros
//       beyond (G, P), B operand theta as step (1) left it; thread 0 draws U and finds j*
//   (6) one lane per sample, in blocks of 256 samples: the lane completes the factor (1 / L_cc into the diagonal, chi^ over b); where
//       J > 256 the columns hold the last pass only, so l(z) is evaluated again from the z kept in LDS for every block.  Eight grid
//       rows at a time: mu_j and s_j by a forward substitution (in registers for M <= 8, else in a second LDS column), then the
//       two sums over j in the tree of block_sum (a lane's samples in order, the wave, the four waves in order).  The lane that
//       owns j* leaves its coefficients.
//   (7) the path, one thread a grid row.
// fp64, no atomics.  A value's bits depend on (curve, chain, slot, seed, J, R, E, noise) alone.
#include "model.hpp"
#include "launchers.hpp"
#include "predict_core.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

constexpr int PF_GV = 8;      // grid rows a lane holds at a time
constexpr int PF_MT = 8;      // the largest M whose forward substitution runs in registers (fit_row)
enum { PF_COEF = 0, PF_Z = 16, PF_J = 24, PF_PAR = 32 };      // the scalars of the path behind the tables

struct PredFitArgs {
  PredArgs p;
  const double* E;
  double *mu_t, *var_t, *path_t, *path_u, *path_xi;
  int32_t* path_idx;
  int G, noise;
};

// LDS doubles behind k_predict's: e [g ES + a] of GP rows, the lanes' columns of the forward substitution (M > PF_MT only), the
// path's scalars
struct PredFitLds {
  int GP, ES;
  size_t e, t, fp, total;
};
__host__ __device__ inline PredFitLds pred_fit_lds(const PredLds& L, int G, int M) {
  PredFitLds F;
  F.GP = (G + 15) / 16 * 16;
  F.ES = L.AP + 1;
  size_t o = L.total;
  F.e = o; o += (size_t)F.GP * F.ES;
  F.t = o; o += M > PF_MT ? (size_t)M * PR_NT : 0;
  F.fp = o; o += PF_PAR;
  F.total = o;
  return F;
}

// The lane's column after pred_ell: 1 / L_cc into the diagonal of the triangle and chi^ = L^-T b over b
__device__ inline void fit_finish(double* Q, int M, double sig) {
  double* b = Q;
  double* A = Q + (size_t)M * PR_NT;
#pragma nounroll
  for (int c = 0; c < M; ++c) {
    double dg = A[tri_index(M, c, c) * PR_NT] + sig;
    for (int k2 = 0; k2 < c; ++k2) { const double l2 = A[tri_index(M, k2, c) * PR_NT]; dg -= l2 * l2; }
    A[tri_index(M, c, c) * PR_NT] = 1.0 / sqrt(dg);
  }
#pragma nounroll
  for (int c = M - 1; c >= 0; --c) {
    double x = b[c * PR_NT];
    for (int r3 = c + 1; r3 < M; ++r3) x -= A[tri_index(M, c, r3) * PR_NT] * b[r3 * PR_NT];
    b[c * PR_NT] = x * A[tri_index(M, c, c) * PR_NT];
  }
}

// mu_j(g) and |L^-1 v_j(g)|^2 of the lane's sample on the grid row whose table row is e: v_m, then t = L^-1 v by forward substitution.
// MT > 0 (M <= MT): t stays in registers, so that the lane's loads of its factor do not wait for a store; MT = 0: in the lane's
// second LDS column sT.  The same operations in the same order either way.
template <int KT, int MT>
__device__ inline void fit_row(const double (&z)[KT], const int (&ko)[KT], const double* e, const double* sQ, const double* A, double* sT,
                               int M, double& mu, double& ss) {
  double c = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < KT; ++k) c += z[k] * e[ko[k]];
  if constexpr (MT > 0) {
    double t[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      t[m] = 0.0;
      if (m < M) {
        double vm = 0.0;
#pragma unroll
        for (int k = 0; k < KT; ++k) vm += z[k] * e[ko[k] + m + 1];
        c += sQ[m * PR_NT] * vm;
#pragma unroll
        for (int k2 = 0; k2 < m; ++k2) vm -= A[tri_index(M, k2, m) * PR_NT] * t[k2];
        vm *= A[tri_index(M, m, m) * PR_NT];
        t[m] = vm;
        s2 += vm * vm;
      }
    }
  } else {
#pragma nounroll
    for (int m = 0; m < M; ++m) {
      double vm = 0.0;
#pragma unroll
      for (int k = 0; k < KT; ++k) vm += z[k] * e[ko[k] + m + 1];
      c += sQ[m * PR_NT] * vm;
      for (int k2 = 0; k2 < m; ++k2) vm -= A[tri_index(M, k2, m) * PR_NT] * sT[k2 * PR_NT];
      vm *= A[tri_index(M, m, m) * PR_NT];
      sT[m * PR_NT] = vm;
      s2 += vm * vm;
    }
  }
  mu = c;
  ss = s2;
}

// Steps (5) to (7) of one draw after pred_draw, which returned sw = sum w
template <int KT>
__device__ inline void fit_draw(const PredFitArgs& fa, const PredLds& L, const PredFitLds& F, double* sm, int r, int rr, int q_chain, int s,
                                double yy, int ni, double sw) {
  const PredArgs& a = fa.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, P = a.P, M = a.M, M1 = M + 1, J = a.J, G = fa.G, GP = F.GP, ES = F.ES, PS = L.PS;
  const double* sTh = sm + L.th;
  const double* sTau = sm + L.tau;
  const double* sGam = sm + L.gam;
  double* sQ = sm + L.q + tid;
  const double* sZ = sm + L.z;
  const double* sLw = sm + L.lw;
  double* sRed = sm + L.red;
  const double* sPar = sm + L.par;
  double* sE = sm + F.e;
  double* sT = sm + F.t + tid;
  double* sFp = sm + F.fp;
  const long long N = (long long)a.C * a.S;
  const size_t t = (size_t)(a.first_slot + s);
  const size_t cs = (size_t)q_chain * a.S + s;
  const size_t row = (size_t)rr * (size_t)N + cs;
  const double sig = sPar[PP_SIG];
  const RngKey key = make_key(a.seed, a.chain0 + (uint32_t)q_chain * a.chain_stride, (uint32_t)t);
  const uint32_t i0 = (uint32_t)((unsigned long long)r * (unsigned long long)(1 + M + G));

  // (5) e = E Theta'
  {
    const int lr = lane & 15, lk = lane >> 4, AT = L.AP / 16, ntile = (GP / 16) * AT;
    for (int tile = wave; tile < ntile; tile += PR_NT / 64) {
      const int ti = tile / AT, tj = tile - ti * AT;
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
      const int g = 16 * ti + lr;
      const double* pa = fa.E + (size_t)min(g, G - 1) * P;
      const double* pb = sTh + (16 * tj + lr) * PS + lk;
      for (int kb = 0; kb < L.PP / 4; ++kb) {
        const int p = 4 * kb + lk;
        const double ev = pa[min(p, P - 1)];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(g < G && p < P ? ev : 0.0, pb[4 * kb], acc, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sE[(16 * ti + lk + 4 * reg) * ES + 16 * tj + lr] = acc[reg];
    }
  }
  if (tid == 0) {
    const double U = runif(key, UPD_PREDICT_FIT, i0);
    const double target = U * sw;
    double cum = 0.0;
    int js = J - 1;
    for (int j = 0; j < J; ++j) {
      cum += sLw[j];
      if (cum > target) { js = j; break; }
    }
    sFp[PF_J] = (double)js;
    fa.path_u[row] = U;
    fa.path_idx[row] = js;
  }
  __syncthreads();

  // (6) the lanes' samples
  const int jstar = (int)sFp[PF_J];
  const int nblk = (J + PR_NT - 1) / PR_NT;
  int ko[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) ko[k] = min(k, K - 1) * M1;
  const double* A = sQ + (size_t)M * PR_NT;
#pragma nounroll
  for (int g0 = 0; g0 < G; g0 += PF_GV) {
    double mu[PF_GV], sv[PF_GV], mut[PF_GV], acc[PF_GV];
#pragma unroll
    for (int i = 0; i < PF_GV; ++i) { mu[i] = 0.0; sv[i] = 0.0; mut[i] = 0.0; }
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int i = 0; i < PF_GV; ++i) acc[i] = 0.0;
#pragma nounroll
      for (int blk = 0; blk < nblk; ++blk) {
        const int j = blk * PR_NT + tid;
        if (j < J) {
          double z[KT];
#pragma unroll
          for (int k = 0; k < KT; ++k) { const double zv = sZ[min(k, K - 1) * J + j]; z[k] = k < K ? zv : 0.0; }
          const bool first = g0 == 0 && pass == 0;
          if (nblk > 1 || first) {
            if (nblk > 1) (void)pred_ell<KT>(z, K, M, sGam, L.GS, sTau, sQ, yy, sig, ni);
            fit_finish(sQ, M, sig);
            if (first && j == jstar) {
              // the owner of j*: xi, L^-T xi in place, then chi^ + sigma L^-T xi
              for (int m = 0; m < M; ++m) {
                const double xi = rnorm(key, UPD_PREDICT_FIT, i0 + 1u + (uint32_t)m);
                sFp[PF_COEF + m] = xi;
                fa.path_xi[row * M + m] = xi;
              }
              for (int c = M - 1; c >= 0; --c) {
                double x = sFp[PF_COEF + c];
                for (int r3 = c + 1; r3 < M; ++r3) x -= A[tri_index(M, c, r3) * PR_NT] * sFp[PF_COEF + r3];
                sFp[PF_COEF + c] = x * A[tri_index(M, c, c) * PR_NT];
              }
              const double sd = sqrt(sig);
              for (int m = 0; m < M; ++m) sFp[PF_COEF + m] = sQ[m * PR_NT] + sd * sFp[PF_COEF + m];
              for (int k = 0; k < K; ++k) sFp[PF_Z + k] = sZ[k * J + j];
            }
          }
          if (nblk > 1 || pass == 0) {
            // mu_j and s_j of the eight rows
#pragma unroll
            for (int i = 0; i < PF_GV; ++i) {
              const double* e = sE + (g0 + i) * ES;
              double ss;
              if (M <= PF_MT) fit_row<KT, PF_MT>(z, ko, e, sQ, A, sT, M, mu[i], ss);
              else fit_row<KT, 0>(z, ko, e, sQ, A, sT, M, mu[i], ss);
              sv[i] = fa.noise ? sig * ss + sig : sig * ss;
            }
          }
          const double w = sLw[j];
#pragma unroll
          for (int i = 0; i < PF_GV; ++i) {
            const double dm = mu[i] - mut[i];
            acc[i] += pass == 0 ? w * mu[i] : w * (sv[i] + dm * dm);
          }
        }
      }
      block_sum<PF_GV>(acc, sRed, lane, wave);
      if (pass == 0) {
#pragma unroll
        for (int i = 0; i < PF_GV; ++i) mut[i] = acc[i] / sw;
      }
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < PF_GV; ++i)
        if (g0 + i < G) {
          const size_t o = ((size_t)rr * G + (g0 + i)) * (size_t)N + cs;
          fa.mu_t[o] = mut[i];
          fa.var_t[o] = acc[i] / sw;
        }
    }
  }
  // (7) the path (block_sum's last barrier is behind the owner's stores)
  {
    const double sd = sqrt(sig);
    for (int g = tid; g < G; g += PR_NT) {
      const double* e = sE + g * ES;
      double c = 0.0;
      for (int k = 0; k < K; ++k) c += sFp[PF_Z + k] * e[k * M1];
      for (int m = 0; m < M; ++m) {
        double vm = 0.0;
        for (int k = 0; k < K; ++k) vm += sFp[PF_Z + k] * e[k * M1 + m + 1];
        c += sFp[PF_COEF + m] * vm;
      }
      if (fa.noise) c += sd * rnorm(key, UPD_PREDICT_FIT, i0 + 1u + (uint32_t)M + (uint32_t)g);
      fa.path_t[((size_t)rr * G + g) * (size_t)N + cs] = c;
    }
  }
}

template <int KT>
__global__ __launch_bounds__(PR_NT) void k_predict_fit(PredFitArgs fa) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const PredArgs& a = fa.p;
  const PredLds L = pred_lds(a.K, a.P, a.M, a.LG, a.J, KT);
  const PredFitLds F = pred_fit_lds(L, fa.G, a.M);
  const int rr = blockIdx.x;
  const int r = a.r0 + rr;
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);
  const PredSlots ch = pred_slots(a, q_chain);
  double yy;
  int ni;
  pred_setup(a, L, sm, r, &yy, &ni);
  for (int s = s_lo; s < s_hi; ++s) {
    const double sw = pred_draw<KT>(a, L, sm, ch, r, rr, q_chain, s, yy, ni);
    fit_draw<KT>(fa, L, F, sm, r, rr, q_chain, s, yy, ni, sw);
  }
}

// One workgroup per (curve, grid row): mean = mean_cs mu_t, sd = sqrt(mean_cs v_t + mean_cs (mu_t - mean)^2) in two passes, every sum
// in the order of block_sum
__global__ __launch_bounds__(PR_NT) void k_predict_fit_pool(long long N, const double* mu_t, const double* var_t, double* mean, double* sd) {
  __shared__ double sRed[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t col = blockIdx.x;
  const double* mu = mu_t + col * (size_t)N;
  const double* va = var_t + col * (size_t)N;
  double v[1] = {0.0};
  for (long long o = tid; o < N; o += PR_NT) v[0] += mu[o];
  block_sum<1>(v, sRed, lane, wave);
  const double m = v[0] / (double)N;
  v[0] = 0.0;
  for (long long o = tid; o < N; o += PR_NT) { const double d = mu[o] - m; v[0] += va[o] + d * d; }
  block_sum<1>(v, sRed, lane, wave);
  if (tid == 0) {
    mean[col] = m;
    sd[col] = sqrt(v[0] / (double)N);
  }
}

}  // namespace

std::string predict_fit_check(const Ctx& c, const PredictFitCall& f, size_t* lds_bytes) {
  const std::string bad = predict_check(c, f.p, nullptr);
  if (!bad.empty()) return bad;
  if (f.G < 1) return "k_predict_fit: G below 1";
  const Dims& d = c.d;
  // (1 + M + G) variates a curve: the index is a 32-bit counter word
  if ((long double)f.p.n_new * (long double)(1 + d.M + (long long)f.G) > 4294967296.0L)
    return "k_predict_fit: n_new x (1 + n_eigen + G) = " + std::to_string(f.p.n_new) + " x " + std::to_string(1 + d.M + (long long)f.G) +
           " exceeds the 4294967296 (2^32) indices of the random number counter";
  const PredLds L = pred_lds(d.K, d.P, d.M, d.LG, f.p.J, pred_kt(d.K));
  const int Gc = std::min(f.G, 1 << 24);
  const PredFitLds F = pred_fit_lds(L, Gc, d.M);
  const size_t bytes = F.total * sizeof(double);
  if (lds_bytes) *lds_bytes = bytes;
  if (bytes > PR_LDS_HARD || f.G > (1 << 24))
    return "k_predict_fit: the tables of a draw (those of k_predict, " + std::to_string(L.total * sizeof(double)) + " bytes, e of " +
           std::to_string(f.G > (1 << 24) ? (long long)f.G : (long long)F.GP) + " x " + std::to_string(L.AP) + " for G = " + std::to_string(f.G) +
           " grid rows" + (d.M > PF_MT ? " and the " + std::to_string(d.M) + " x 256 values of the forward substitution" : std::string()) + ") need " +
           (f.G > (1 << 24) ? std::string("more than 1073741824") : std::to_string(bytes)) + " bytes of LDS, above the limit of " +
           std::to_string(PR_LDS_HARD) + " (160 KiB)";
  return "";
}

std::string launch_predict_fit(const Ctx& c, const PredictFitCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                               double* prop, double* samples, double* mu_t, double* var_t, double* path_t, int32_t* path_idx, double* path_u,
                               double* path_xi, hipStream_t st) {
  size_t lds = 0;
  const std::string bad = predict_fit_check(c, f, &lds);
  if (!bad.empty()) return bad;
  if (rows < 1 || r0 < 0 || (long long)r0 + rows > f.p.n_new) return "k_predict_fit: curves outside the call";
  if (!f.E || !mu_t || !var_t || !path_t || !path_idx || !path_u || !path_xi) return "k_predict_fit: null buffer";
  PredFitArgs fa;
  fa.p = pred_args(c, f.p, r0, rows, lpd_t, ess_t, m_t, q_t, prop, samples);
  fa.E = f.E; fa.G = f.G; fa.noise = f.noise ? 1 : 0;
  fa.mu_t = mu_t; fa.var_t = var_t; fa.path_t = path_t; fa.path_idx = path_idx; fa.path_u = path_u; fa.path_xi = path_xi;
  const dim3 grid((unsigned)rows, (unsigned)((f.p.n_slots + fa.p.SCH - 1) / fa.p.SCH), (unsigned)c.nch);
  void (*fn)(PredFitArgs) = pred_kt(c.d.K) == 4 ? k_predict_fit<4> : k_predict_fit<KMAX>;
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_predict_fit: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, grid, dim3(PR_NT), lds, st, fa);
  if (hipGetLastError() != hipSuccess) return "k_predict_fit: launch failed";
  return "";
}

std::string launch_predict_fit_pool(long long N, long long ncol, const double* mu_t, const double* var_t, double* mean, double* sd, hipStream_t st) {
  if (N < 1 || ncol < 1 || ncol > 2147483647LL) return "k_predict_fit_pool: bad shape";
  hipLaunchKernelGGL(k_predict_fit_pool, dim3((unsigned)ncol), dim3(PR_NT), 0, st, N, mu_t, var_t, mean, sd);
  if (hipGetLastError() != hipSuccess) return "k_predict_fit_pool: launch failed";
  return "";
}

}  // namespace bfmmm
