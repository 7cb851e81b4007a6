// The mode search of the Laplace mixture proposal (kernels_predict_laplace.hip) on the tables Gamma and tau of a draw,
// for one thread a start (the host) or one wave a start (the device): the integrand's log density over the log-ratios eta,
//     g(eta) = l(z(eta)) + sum_k alpha_k log z_k - lB(alpha),   z_k = e^eta_k / (1 + sum e^eta) (k < d = K - 1),  z_K = 1 / (1 + sum e^eta),
// its gradient and Hessian from the tables alone, and the Levenberg-damped Newton ascent.  With T(z) = sum_kl z_k z_l Gamma_(k.)(l.),
// t(z) = sum_k z_k tau_(k.), rr = yy - 2 t_0 + T_00, u = t_1: - T_1:,0, A = sigma^2 I + T_1:,1:, b = A^-1 u and
// F = log det A + (rr - u'b) / sigma^2, so that l = -1/2 (n* log 2 pi + (n* - M) log sigma^2 + F):
//     S_k = sum_l z_l Gamma_(k.)(l.),  D_k = S_k + S_k' = dT/dz_k,  D_kl = Gamma_(k.)(l.) + Gamma_(k.)(l.)' = d2T/dz_k dz_l,
//     d_k rr = -2 tau_k0 + D_k[0,0],  d_k u = tau_k,1: - D_k[1:,0],  d_k A = D_k[1:,1:],  r_k = d_k u - d_k A b,
//     d_k F  = tr(A^-1 d_k A) + (d_k rr - 2 b'd_k u + b'd_k A b) / sigma^2,
//     d_kl F = tr(A^-1 D_kl[1:,1:]) - tr(A^-1 d_k A A^-1 d_l A) + (D_kl[0,0] + 2 b'D_kl[1:,0] + b'D_kl[1:,1:] b - 2 r_k'A^-1 r_l) / sigma^2,
// l_k = -1/2 d_k F, l_kl = -1/2 d_kl F, and with J_ik = z_i (delta_ik - z_k), alpha_0 = sum alpha:
//     grad_k = sum_i l_i J_ik + alpha_k - alpha_0 z_k,
//     H_kl   = sum_ij l_ij J_ik J_jl + sum_i l_i z_i [(delta_il - z_l)(delta_ik - z_k) - z_k (delta_kl - z_l)] - alpha_0 z_k (delta_kl - z_l).
// Nothing of size P or n* is touched.  Host and device: the same text runs in a stand-alone program on the CPU.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <math.h>

namespace bfmmm {

constexpr int LAP_ITERS = 40;           // Newton steps of a start at the most
constexpr double LAP_DEC = 1e-6;        // a start has converged where -H is positive definite and grad'(-H)^-1 grad is below this
constexpr double LAP_SAME = 1e-3;       // a mode within this (max norm in eta) of an earlier component is dropped

// the scratch of one start (doubles), carved up by lap_ws
struct LapWs {
  double *S, *Pk, *rk, *wk, *pa, *T, *Ai, *Lc, *u, *b, *tv, *z, *lk, *lkl, *Jm, *H, *Ht, *C, *grad, *gradt, *eta, *etat, *delta;
};
__host__ __device__ inline int lap_scratch(int K, int M) {
  const int M1 = M + 1, d = K - 1;
  return K * (M1 * M1 + M * M + 4 * M) + M1 * M1 + 2 * M * M + 2 * M + M1 + 2 * K + K * K + K * d + 3 * d * d + 5 * d;
}
__host__ __device__ inline LapWs lap_ws(double* p, int K, int M) {
  const int M1 = M + 1, d = K - 1;
  LapWs w;
  w.S = p; p += K * M1 * M1;
  w.Pk = p; p += K * M * M;
  w.rk = p; p += K * M;
  w.wk = p; p += K * M;
  w.pa = p; p += 2 * K * M;
  w.T = p; p += M1 * M1;
  w.Ai = p; p += M * M;
  w.Lc = p; p += M * M;
  w.u = p; p += M;
  w.b = p; p += M;
  w.tv = p; p += M1;
  w.z = p; p += K;
  w.lk = p; p += K;
  w.lkl = p; p += K * K;
  w.Jm = p; p += K * d;
  w.H = p; p += d * d;
  w.Ht = p; p += d * d;
  w.C = p; p += d * d;
  w.grad = p; p += d;
  w.gradt = p; p += d;
  w.eta = p; p += d;
  w.etat = p; p += d;
  w.delta = p; p += d;
  return w;
}

// z of eta, entries clamped below at DBL_MIN
__host__ __device__ inline void lap_z(int K, const double* eta, double* z) {
  const int d = K - 1;
  double mx = 0.0, sum = 0.0;
  for (int k = 0; k < d; ++k) mx = fmax(mx, eta[k]);
  for (int k = 0; k < K; ++k) { z[k] = exp((k < d ? eta[k] : 0.0) - mx); sum += z[k]; }
  for (int k = 0; k < K; ++k) z[k] = fmax(z[k] / sum, DBL_MIN);
}

// C C' = A + lam I (n x n, row-major; C lower, the rest of it untouched); false where a pivot is not positive
__host__ __device__ inline bool lap_chol(int n, const double* A, double lam, double sign, double* C) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = sign * A[i * n + j] + (i == j ? lam : 0.0);
      for (int k = 0; k < j; ++k) v -= C[i * n + k] * C[j * n + k];
      if (i == j) {
        if (!(v > 0.0) || !(v < INFINITY)) return false;
        C[i * n + i] = sqrt(v);
      } else {
        C[i * n + j] = v / C[j * n + j];
      }
    }
  return true;
}
// x = (C C')^-1 y
__host__ __device__ inline void lap_chol_solve(int n, const double* C, const double* y, double* x) {
  for (int i = 0; i < n; ++i) {
    double v = y[i];
    for (int k = 0; k < i; ++k) v -= C[i * n + k] * x[k];
    x[i] = v / C[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = x[i];
    for (int k = i + 1; k < n; ++k) v -= C[k * n + i] * x[k];
    x[i] = v / C[i * n + i];
  }
}

// the draw and the curve as the search sees them
struct LapCase {
  const double *Gam, *tau, *alpha;      // Gamma [(k M1 + a) GS + l M1 + b], tau [k M1 + a], alpha_3 pi
  double lBa, yy, sig;
  int GS, K, M, ni;
};

// Between two phases of lap_eval whose entries are dealt to the lanes of a wave: what the lanes wrote to the scratch is there for all
__host__ __device__ inline void lap_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}

// g at eta; with derivs the gradient (d) and the Hessian (d x d) too.  -inf where A has no Cholesky factor.
// Run by the nl lanes of a wave together (lane of nl; one thread alone: 0 of 1): the tables S_k, T, A^-1, P_k, r_k, A^-1 r_k and
// l_kl are dealt to the lanes entry by entry, each entry summed by one lane in the order a single thread would, and everything
// else is computed by every lane alike, so that the lanes agree on every value and every branch and the bits do not depend on nl.
__host__ __device__ inline double lap_eval(const LapCase& c, const double* eta, const LapWs& w, bool derivs, double* grad, double* H,
                                           int lane = 0, int nl = 1) {
  const int K = c.K, M = c.M, M1 = M + 1, d = K - 1, GS = c.GS;
  const double sig = c.sig;
  double* z = w.z;
  lap_z(K, eta, z);
  for (int e = lane; e < K * M1 * M1; e += nl) {
    const int k = e / (M1 * M1), ab = e - k * M1 * M1, a = ab / M1, b = ab - a * M1;
    const double* g = c.Gam + (k * M1 + a) * GS + b;
    double s = 0.0;
    for (int l = 0; l < K; ++l) s += z[l] * g[l * M1];
    w.S[e] = s;
  }
  lap_sync();
  for (int e = lane; e < M1 * M1 + M1; e += nl) {
    double s = 0.0;
    if (e < M1 * M1) {
      for (int k = 0; k < K; ++k) s += z[k] * w.S[k * M1 * M1 + e];
      w.T[e] = s;
    } else {
      for (int k = 0; k < K; ++k) s += z[k] * c.tau[k * M1 + e - M1 * M1];
      w.tv[e - M1 * M1] = s;
    }
  }
  lap_sync();
  const double rr = c.yy - 2.0 * w.tv[0] + w.T[0];
  for (int m = 0; m < M; ++m) {
    w.u[m] = w.tv[m + 1] - 0.5 * (w.T[(m + 1) * M1] + w.T[m + 1]);
    for (int n = 0; n <= m; ++n) w.Ai[m * M + n] = 0.5 * (w.T[(m + 1) * M1 + n + 1] + w.T[(n + 1) * M1 + m + 1]);      // (A for now)
  }
  if (!lap_chol(M, w.Ai, sig, 1.0, w.Lc)) return -INFINITY;
  double logdet = 0.0, ub = 0.0;
  for (int m = 0; m < M; ++m) logdet += 2.0 * log(w.Lc[m * M + m]);
  lap_chol_solve(M, w.Lc, w.u, w.b);
  for (int m = 0; m < M; ++m) ub += w.u[m] * w.b[m];
  const double F = logdet + (rr - ub) / sig;
  double g = -0.5 * ((double)c.ni * 1.83787706640934548356 + (double)(c.ni - M) * log(sig) + F) - c.lBa;
  double a0 = 0.0;
  for (int k = 0; k < K; ++k) { g += c.alpha[k] * log(z[k]); a0 += c.alpha[k]; }
  if (!derivs) return g;

  // A^-1, a column a lane, solved in place
  lap_sync();
  for (int n = lane; n < M; n += nl) {
    for (int i = 0; i < M; ++i) {
      double v = i == n ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) v -= w.Lc[i * M + k] * w.Ai[k * M + n];
      w.Ai[i * M + n] = v / w.Lc[i * M + i];
    }
    for (int i = M - 1; i >= 0; --i) {
      double v = w.Ai[i * M + n];
      for (int k = i + 1; k < M; ++k) v -= w.Lc[k * M + i] * w.Ai[k * M + n];
      w.Ai[i * M + n] = v / w.Lc[i * M + i];
    }
  }
  lap_sync();
  // row m of d_k u, d_k A b, r_k and P_k = A^-1 d_k A; pa: the terms b_m d_k u_m and b_m (d_k A b)_m
  for (int e = lane; e < K * M; e += nl) {
    const int k = e / M, m = e - k * M;
    const double* Sk = w.S + k * M1 * M1;
    const double du = c.tau[k * M1 + m + 1] - (Sk[(m + 1) * M1] + Sk[m + 1]);
    double Ab = 0.0;
    for (int n = 0; n < M; ++n) Ab += (Sk[(m + 1) * M1 + n + 1] + Sk[(n + 1) * M1 + m + 1]) * w.b[n];
    w.rk[e] = du - Ab;
    w.pa[e] = w.b[m] * du;
    w.pa[K * M + e] = w.b[m] * Ab;
    for (int n = 0; n < M; ++n) {
      double s = 0.0;
      for (int q = 0; q < M; ++q) s += w.Ai[m * M + q] * (Sk[(q + 1) * M1 + n + 1] + Sk[(n + 1) * M1 + q + 1]);
      w.Pk[k * M * M + m * M + n] = s;
    }
  }
  lap_sync();
  for (int e = lane; e < K * M; e += nl) {
    const int k = e / M, m = e - k * M;
    double s = 0.0;
    for (int n = 0; n < M; ++n) s += w.Ai[m * M + n] * w.rk[k * M + n];
    w.wk[e] = s;
  }
  for (int k = lane; k < K; k += nl) {
    double tr = 0.0, bdu = 0.0, bAb = 0.0;
    for (int m = 0; m < M; ++m) { tr += w.Pk[k * M * M + m * M + m]; bdu += w.pa[k * M + m]; bAb += w.pa[K * M + k * M + m]; }
    const double drr = -2.0 * c.tau[k * M1] + 2.0 * w.S[k * M1 * M1];
    w.lk[k] = -0.5 * (tr + (drr - 2.0 * bdu + bAb) / sig);
  }
  lap_sync();
  for (int k = 0, p = 0; k < K; ++k)
    for (int l = k; l < K; ++l, ++p) {
      if (p % nl != lane) continue;
      // D_kl[a][b] = Gamma_(k a)(l b) + Gamma_(k b)(l a)
      const double* gk = c.Gam + (k * M1) * GS + l * M1;
      double t1 = 0.0, t2 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
      for (int m = 0; m < M; ++m) {
        c1 += w.b[m] * (gk[(m + 1) * GS] + gk[m + 1]);
        c3 += w.rk[k * M + m] * w.wk[l * M + m];
        for (int n = 0; n < M; ++n) {
          const double dkl = gk[(m + 1) * GS + n + 1] + gk[(n + 1) * GS + m + 1];
          t1 += w.Ai[n * M + m] * dkl;
          c2 += w.b[m] * dkl * w.b[n];
          t2 += w.Pk[k * M * M + m * M + n] * w.Pk[l * M * M + n * M + m];
        }
      }
      const double v = -0.5 * (t1 - t2 + (2.0 * gk[0] + 2.0 * c1 + c2 - 2.0 * c3) / sig);
      w.lkl[k * K + l] = v;
      w.lkl[l * K + k] = v;
    }
  lap_sync();
  for (int i = 0; i < K; ++i)
    for (int k = 0; k < d; ++k) w.Jm[i * d + k] = z[i] * ((i == k ? 1.0 : 0.0) - z[k]);
  for (int k = 0; k < d; ++k) {
    double s = c.alpha[k] - a0 * z[k];
    for (int i = 0; i < K; ++i) s += w.lk[i] * w.Jm[i * d + k];
    grad[k] = s;
    for (int l = 0; l <= k; ++l) {
      double h = -a0 * z[k] * ((k == l ? 1.0 : 0.0) - z[l]);
      for (int i = 0; i < K; ++i) {
        double t = 0.0;
        for (int j = 0; j < K; ++j) t += w.lkl[i * K + j] * w.Jm[j * d + l];
        const double dil = i == l ? 1.0 : 0.0, dik = i == k ? 1.0 : 0.0, dkl = k == l ? 1.0 : 0.0;
        h += w.Jm[i * d + k] * t + w.lk[i] * z[i] * ((dil - z[l]) * (dik - z[k]) - z[k] * (dkl - z[l]));
      }
      H[k * d + l] = h;
      H[l * d + k] = h;
    }
  }
  return g;
}

// The damped Newton ascent from w.eta, by one thread or by the nl lanes of a wave together (lap_eval), every lane taking every step.  Returns whether the start has converged; then w.eta is the mode, w.H the Hessian there, w.C
// the Cholesky factor of -H and *g the value.  *g0: g at the start; *iters: the steps tried.
__host__ __device__ inline bool lap_search(const LapCase& c, const LapWs& w, double* g_out, double* g0, int* iters, int lane = 0, int nl = 1) {
  const int d = c.K - 1;
  double g = lap_eval(c, w.eta, w, true, w.grad, w.H, lane, nl);
  *g0 = g;
  *g_out = g;
  *iters = 0;
  if (!(fabs(g) < INFINITY)) return false;
  double lam = 0.0;
  for (int it = 0;; ++it) {
    *iters = it;
    double scale = 1.0;
    for (int k = 0; k < d; ++k) scale = fmax(scale, fabs(w.H[k * d + k]));
    const bool pd = lap_chol(d, w.H, 0.0, -1.0, w.C);
    if (pd) {
      lap_chol_solve(d, w.C, w.grad, w.delta);
      double dec = 0.0;
      for (int k = 0; k < d; ++k) dec += w.grad[k] * w.delta[k];
      if (dec < LAP_DEC) { *g_out = g; return true; }
    }
    if (it == LAP_ITERS) return false;
    if (!pd || lam > 0.0) {
      if (!pd && lam == 0.0) lam = 1e-3 * scale;
      int tries = 0;
      while (!lap_chol(d, w.H, lam, -1.0, w.C)) {
        lam = fmax(10.0 * lam, 1e-3 * scale);
        if (++tries > 60) return false;
      }
      lap_chol_solve(d, w.C, w.grad, w.delta);
    }
    for (int k = 0; k < d; ++k) w.etat[k] = w.eta[k] + w.delta[k];
    const double gt = lap_eval(c, w.etat, w, true, w.gradt, w.Ht, lane, nl);
    if (fabs(gt) < INFINITY && gt >= g - 1e-13 * fabs(g)) {
      for (int k = 0; k < d; ++k) { w.eta[k] = w.etat[k]; w.grad[k] = w.gradt[k]; }
      for (int k = 0; k < d * d; ++k) w.H[k] = w.Ht[k];
      g = gt;
      lam *= 0.1;
      if (lam < 1e-6 * scale) lam = 0.0;
    } else {
      lam = fmax(10.0 * lam, 1e-3 * scale);
    }
  }
}

// Sigma = (C C')^-1 = L L': L packed by rows ([i (i + 1) / 2 + j], j <= i) into Lp; tmp: 2 d d doubles.  Returns sum log L_ii, or
// NaN where Sigma has no factor in floating point.
__host__ __device__ inline double lap_scale_factor(int d, const double* C, double* tmp, double* Lp) {
  double* Ci = tmp;            // C^-1, lower
  double* Sg = tmp + d * d;
  for (int j = 0; j < d; ++j)
    for (int i = 0; i < d; ++i) {
      if (i < j) { Ci[i * d + j] = 0.0; continue; }
      double v = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) v -= C[i * d + k] * Ci[k * d + j];
      Ci[i * d + j] = v / C[i * d + i];
    }
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = i; k < d; ++k) s += Ci[k * d + i] * Ci[k * d + j];
      Sg[i * d + j] = s;
      Sg[j * d + i] = s;
    }
  if (!lap_chol(d, Sg, 0.0, 1.0, Ci)) return NAN;
  double sl = 0.0;
  for (int i = 0; i < d; ++i) {
    for (int j = 0; j <= i; ++j) Lp[i * (i + 1) / 2 + j] = Ci[i * d + j];
    sl += log(Ci[i * d + i]);
  }
  return sl;
}

}  // namespace bfmmm
