// What k_loo_pointwise (kernels_loo_pointwise.hip) and k_loo_blocks (kernels_loo_blocks.hip) do alike for a
// batch of staged draws of one curve: steps (1) to (4) of the former's header comment and the MFMA loop of its step (5), written
// once.  A workgroup of LC_NT threads calls each step with all its threads and puts its own __syncthreads() between them.  `Args`
// is the kernel's argument record; read here: c_nu, c_Phi, c_eta, c_xi of the chain (passed shifted), K, P, M, D, BW, cadj,
// first_slot.  The LDS strides are the caller's: row p of a draw's [c | V] has CVS doubles and a draw CVN, [e | G V] of a draw GVN,
// a draw's A / u / beta record AS (A: lower triangle, row-major, M x M; u at M M; beta at M M + M).
// fp64; every sum has a fixed order.
#pragma once
#include "model.hpp"

namespace bfmmm {

constexpr int LC_NT = 256;

typedef double lc_v4 __attribute__((ext_vector_type(4)));

// (1) c and V_m at p, draws sb .. sb + gn of the slot range: sCV[g CVN + p CVS + mt]
template <class Args>
__device__ __forceinline__ void lc_coefficients(const Args& a, const double* c_nu, const double* c_Phi, const double* c_eta,
                                                const double* c_xi, const double* sZ, const double* sX, double* sCV, int sb, int gn,
                                                int CVS, int CVN, int GVN, int tid) {
  const int K = a.K, P = a.P, M = a.M, D = a.D;
  for (int e = tid; e < gn * GVN; e += LC_NT) {
    const int g = e / GVN, r = e - g * GVN, mt = r / P, p = r - mt * P;
    const size_t t = (size_t)(a.first_slot + sb + g);
    const bool cov = D > 0 && (mt == 0 || a.cadj);
    const double* z = sZ + g * K;
    double v = 0.0;
    for (int k = 0; k < K; ++k) {
      double x = mt == 0 ? c_nu[t * K * P + (size_t)p * K + k] : c_Phi[t * K * P * M + k + (size_t)K * (p + P * (mt - 1))];
      if (cov) {
        const double* tx = mt == 0 ? c_eta + t * P * D * K + p + (size_t)P * D * k
                                   : c_xi + t * K * P * D * M + p + (size_t)P * D * ((mt - 1) + M * k);
        for (int d = 0; d < D; ++d) x += sX[d] * tx[(size_t)P * d];
      }
      v += z[k] * x;
    }
    sCV[g * CVN + p * CVS + mt] = v;
  }
}

// (2) G times each of them at p, over the band window: sGV[g GVN + mt P + p] = e = s - G c (mt = 0) or G V_mt
template <class Args>
__device__ __forceinline__ void lc_gram_times(const Args& a, const double* sRec, const double* sS, const double* sCV, double* sGV, int gn,
                                              int CVS, int CVN, int GVN, int tid) {
  const int P = a.P, BW = a.BW;
  for (int e = tid; e < gn * GVN; e += LC_NT) {
    const int g = e / GVN, r = e - g * GVN, mt = r / P, p = r - mt * P;
    const double* cv = sCV + g * CVN + mt;
    double hv = 0.0;
    for (int d = -BW; d <= BW; ++d) {
      const int p2 = p + d;
      if (p2 >= 0 && p2 < P) hv += sRec[(d < 0 ? -d : d) * P + min(p, p2)] * cv[p2 * CVS];
    }
    sGV[g * GVN + r] = mt == 0 ? sS[p] - hv : hv;
  }
}

// (3) u_m = V_m'e, A_lm = V_m'(G V_l) for l >= m, sigma^2 on the diagonal
template <class Args>
__device__ __forceinline__ void lc_u_and_a(const Args& a, const double* sCV, const double* sGV, const double* sSig, double* sA, int gn,
                                           int CVS, int CVN, int GVN, int AS, int tid) {
  const int P = a.P, M = a.M, M1 = M + 1;
  for (int e = tid; e < gn * M * M1; e += LC_NT) {
    const int g = e / (M * M1), r = e - g * M * M1, m = r / M1, j = r - m * M1;      // j = 0: u_m, else l = j - 1
    if (j > 0 && j - 1 < m) continue;
    const double* vm = sCV + g * CVN + 1 + m;
    const double* gv = sGV + g * GVN + j * P;
    double s_ = 0.0;
    for (int p = 0; p < P; ++p) s_ += vm[p * CVS] * gv[p];
    double* A = sA + g * AS;
    if (j == 0) A[M * M + m] = s_;
    else A[(j - 1) * M + m] = (j - 1 == m) ? s_ + sSig[g] : s_;
  }
}

// (4) one lane: A = L L' in place, beta = A^-1 u
__device__ __forceinline__ void lc_factor_beta(double* A, int M) {
  const double* u = A + M * M;
  double* beta = A + M * M + M;
  for (int c = 0; c < M; ++c) {
    double dg = A[c * M + c];
    for (int k2 = 0; k2 < c; ++k2) { const double l2 = A[c * M + k2]; dg -= l2 * l2; }
    const double l = sqrt(dg);
    A[c * M + c] = l;
    for (int r3 = c + 1; r3 < M; ++r3) {
      double v = A[r3 * M + c];
      for (int k2 = 0; k2 < c; ++k2) v -= A[r3 * M + k2] * A[c * M + k2];
      A[r3 * M + c] = v / l;
    }
  }
  for (int c = 0; c < M; ++c) {
    double x = u[c];
    for (int k2 = 0; k2 < c; ++k2) x -= A[c * M + k2] * beta[k2];
    beta[c] = x / A[c * M + c];
  }
  for (int c = M - 1; c >= 0; --c) {
    double x = beta[c];
    for (int r3 = c + 1; r3 < M; ++r3) x -= A[r3 * M + c] * beta[r3];
    beta[c] = x / A[c * M + c];
  }
}

// (5), first half, one wave: [mu | W] = B_tile [c | V] of one draw on v_mfma_f64_16x16x4_f64 into the wave's rows sMW (row j: MWS
// doubles); sB: the tile's nr basis rows of BS doubles (zero rows up to the next multiple of 16), cv: the draw's [c | V]
__device__ __forceinline__ void lc_mfma_rows(const double* sB, const double* cv, double* sMW, int nr, int P, int M1, int BS, int CVS,
                                             int MWS, int lane) {
  const int lr = lane & 15, lk = lane >> 4;
  for (int ti = 0; 16 * ti < nr; ++ti) {
    const double* pa = sB + (16 * ti + lr) * BS;
    for (int tj = 0; 16 * tj < M1; ++tj) {
      const int col = 16 * tj + lr;
      lc_v4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int kb = 0; 4 * kb < P; ++kb) {
        const int p = 4 * kb + lk;
        const bool in = p < P;
        const double av = in ? pa[p] : 0.0;
        const double bv = in && col < M1 ? cv[p * CVS + col] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
      if (col < M1) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sMW[(16 * ti + lk + 4 * reg) * MWS + col] = acc[reg];
      }
    }
  }
}

}  // namespace bfmmm
