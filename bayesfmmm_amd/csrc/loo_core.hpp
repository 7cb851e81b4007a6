// What k_loo_pointwise (kernels_loo_pointwise.hip) and k_loo_blocks (kernels_loo_blocks.hip) do alike for a
// batch of staged draws of one curve: steps (1) to (4) of the former's header comment and the MFMA loop of its step (5), written
// once.  A workgroup of LC_NT threads calls each step with all its threads and puts its own __syncthreads() between them.  `Args`
// is the kernel's argument record; read here: c_nu, c_Phi, c_eta, c_xi of the chain (passed shifted), K, P, M, D, BW, cadj,
// first_slot.  The LDS strides are the caller's: row p of a draw's [c | V] has CVS doubles and a draw CVN, [e | G V] of a draw GVN,
// a draw's A / u / beta record AS (A: lower triangle, row-major, M x M; u at M M; beta at M M + M).
// fp64; every sum has a fixed order.
// Behind the device steps, the host half of the two kernels, written once as well: the argument record, the choice of TB, the
// shape check, the filling of the record and the launch.
#pragma once
#include "model.hpp"

#include <string>

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

// ---- the host half of the two kernels ----------------------------------------------------------------------------------------------
constexpr int LC_TB_MAX = 8;
constexpr size_t LC_LDS_SOFT = 64 * 1024;      // two workgroups per CU where the shape allows
constexpr size_t LC_LDS_HARD = 160 * 1024;

// What both kernels take, in two parts that keep the order of the kernels' argument records: k_loo_blocks has its row table between
// them (kernels_loo_blocks.hip).
template <class Tile>
struct LcArgsHead {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Z, *c_nu, *c_Phi, *c_sigma, *c_eta, *c_xi;
  const double *rec, *X, *y, *B;
  const Tile* tiles;
};
struct LcArgsTail {
  double* out;                                  // matrix v at out + v * out_stride
  size_t out_stride, chain_bytes, chain_bytes_cov;
  int n, K, P, M, D, BW, LG, LREC, cadj, mv;
  int C, first_slot, S;
  int TB, SCH;                                  // draws per staged batch, slots per workgroup (a multiple of TB)
};
template <class Tile>
struct LcArgs : LcArgsHead<Tile>, LcArgsTail {};

// draws per staged batch and the LDS bytes of the layout lds(K, P, M, LG, TB) with them: what fits LC_LDS_SOFT down to 4, then LC_LDS_HARD
template <class Layout>
int lc_pick_tb(const Dims& d, Layout lds, size_t* bytes_out) {
  auto bytes = [&](int tb) { return lds(d.K, d.P, d.M, d.LG, tb).total * sizeof(double); };
  int TB = LC_TB_MAX;
  while (TB > 4 && bytes(TB) > LC_LDS_SOFT) TB >>= 1;
  while (TB > 1 && bytes(TB) > LC_LDS_HARD) TB >>= 1;
  *bytes_out = bytes(TB);
  return TB;
}

// "" or what kernel `k` cannot take of the sampler's shape; `holds`: what its LDS holds, for a shape whose layout needs `bytes`
inline std::string lc_shape_check(const Ctx& c, const std::string& k, const char* holds, size_t bytes) {
  const Dims& d = c.d;
  if (d.P < 1 || d.P > PMAX) return k + ": P outside 1 .. 64";
  if (d.M < 1 || d.M > 16) return k + ": n_eigen outside 1 .. 16";
  if (d.K < 1 || d.K > KMAX) return k + ": K outside 1 .. 8";
  if (d.D < 0 || d.D > 8) return k + ": more than 8 covariates";
  if (d.BW < 0 || d.BW > BWWIDE) return k + ": band half-width above 31";
  if (c.nch < 1 || c.nch > 65535) return k + ": more than 65535 chains";
  if (bytes > LC_LDS_HARD)
    return k + ": " + holds + " (P = " + std::to_string(d.P) + ", n_eigen = " + std::to_string(d.M) + ", band " + std::to_string(d.BW) +
           ") need " + std::to_string(bytes) + " bytes of LDS, above the kernel's 163840";
  return "";
}

// all of LcArgs but TB and SCH; "" or what kernel `k` cannot take: `bad` of its shape check, or the arguments (`tables`: all given)
template <class Args, class Tile>
std::string lc_fill(Args& a, const std::string& bad, const std::string& k, const Ctx& c, bool tables, const Tile* tiles, long long n_tiles,
                    const double* B, const double* y, int first_slot, int n_slots, double* out, size_t out_stride) {
  const Dims& d = c.d;
  if (!bad.empty()) return bad;
  if (n_tiles < 1 || n_tiles > 2147483647LL || !tables || !y || !out || (!d.mv && !B)) return k + ": bad arguments";
  if (n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return k + ": range outside the chain storage";
  a.c_Z = c.c_Z; a.c_nu = c.c_nu; a.c_Phi = c.c_Phi; a.c_sigma = c.c_sigma;
  a.c_eta = d.D > 0 ? c.c_eta : nullptr; a.c_xi = d.D > 0 ? c.c_xi : nullptr;
  a.rec = c.rec; a.X = d.D > 0 ? c.X : nullptr; a.y = y; a.B = B; a.tiles = tiles; a.out = out; a.out_stride = out_stride;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.n = d.n; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.BW = d.BW; a.LG = d.LG; a.LREC = d.LREC;
  a.cadj = (d.D > 0 && c.covariance_adj) ? 1 : 0;
  a.mv = d.mv ? 1 : 0;
  a.C = c.nch; a.first_slot = first_slot; a.S = n_slots;
  return "";
}

// kernel `k` (named `name`, LDS layout `layout`) over n_tiles tiles, runs of a.SCH slots and the chains
template <class Args, class Layout>
std::string lc_launch(void (*k)(Args), const std::string& name, Args& a, const Dims& d, Layout layout, long long n_tiles, hipStream_t st) {
  size_t lds = 0;
  a.TB = lc_pick_tb(d, layout, &lds);
  // slots per workgroup: eight batches, more where the grid's y extent would pass 65535
  long long sch = (long long)a.TB * 8;
  while (((long long)a.S + sch - 1) / sch > 65535) sch *= 2;
  a.SCH = (int)sch;
  const dim3 grid((unsigned)n_tiles, (unsigned)((a.S + a.SCH - 1) / a.SCH), (unsigned)a.C);
  if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return name + ": cannot set the LDS size";
  }
  hipLaunchKernelGGL(k, grid, dim3(LC_NT), lds, st, a);
  if (hipGetLastError() != hipSuccess) return name + ": launch failed";
  return "";
}

}  // namespace bfmmm
