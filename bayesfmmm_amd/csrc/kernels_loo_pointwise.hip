// Observation-level leave-one-out quantities of chain slots: for every chain q, slot t and observation j of
// curve i, the law of y_ij given the REST of the curve and the draw, the scores chi_i integrated out.  With c and V_m as in
// kernels_curve_ll.hip, b_j the j-th basis row of the curve (the unit vectors for the multivariate model):
//     mu_j = b_j'c,  w_j = (b_j'V_1 .. b_j'V_M)',  r_j = y_ij - mu_j,
//     A = sigma^2 I_M + V'G_i V = L L',  u = V'(s_i - G_i c),  beta = A^-1 u            (from the resident record, not from the rows)
//     h_j = |L^-1 w_j|^2,  omega_j = 1 - h_j,  e_j = r_j - w_j'beta,
//     l = -1/2 [ log 2 pi + log sigma^2 - log omega_j + e_j^2 / (sigma^2 omega_j) ],  z = e_j / (sigma sqrt omega_j),
//     m = y_ij - e_j / omega_j,  v = sigma^2 / omega_j.
// Four values per (observation, draw) go to four matrices of rows x (C S), draw fastest, then chain, then observation: l,
// Phi(z) = erfc(-z / sqrt 2) / 2, m and m^2 + v: the log-likelihood matrix and the three auxiliary matrices of
// post_psis_expect_device.
//
// Geometry.  A workgroup of 256 threads takes one row tile (up to 64 consecutive observations of one curve, from the host's tile
// list), one chain and a run of slots.  The tile's dense basis rows, the curve's record and covariates are staged once; then
// TB draws at a time:
//   (1) every (draw, mt, p): c[p] (mt = 0) or V_mt[p] from the slot's nu, Phi (eta, xi), the k sum in order -> LDS, P x (M + 1) a draw
//   (2) every (draw, mt, p): (G V_mt)[p] over the band window -> e = s - G c, G V_m
//   (3) every (draw, m, l >= m): u_m = V_m'e and A_lm = V_m'(G V_l) (+ sigma^2 on the diagonal), p in order
//   (4) lane g of the first wave: Cholesky of draw g's A in place, beta by the two triangular solves
//   (5) wave w takes draws w, w + 4, ..: [mu | W] = B_tile [c | V] on v_mfma_f64_16x16x4_f64 (row tiles of 16, ceil((M + 1) / 16)
//       column tiles, ceil(P / 4) k-steps; C/D: col = lane & 15, row = (lane >> 4) + 4 reg) into the wave's own LDS rows; then
//       lane j owns observation j: w_j'beta, the forward solve L^-1 w_j in place in its row (L broadcast from LDS), the four
//       values -> the staging table
//   (6) the table -> the four matrices, one draw-contiguous segment per (matrix, observation)
// Steps (1) to (4) and the MFMA loop of (5) are loo_core.hpp's, shared with k_loo_blocks (kernels_loo_blocks.hip).
// L and beta of a (curve, draw) are recomputed by every tile of the curve, from the same record in the same order, so the tiles of
// a curve agree bit for bit and there is neither a pre-pass nor a workspace.  fp64, vector stores only, no atomics; every sum has
// a fixed order that depends on (observation, chain, slot) alone: the bits do not depend on the chunk, the grid or TB.
#include "model.hpp"
#include "launchers.hpp"
#include "loo_core.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

constexpr int LP_NT = LC_NT;
constexpr int LP_TB_MAX = LC_TB_MAX;

using LpArgs = LcArgs<LpTile>;

// LDS doubles of k_loo_pointwise
struct LpLds {
  int BS, CVS, CVN, GVN, AS, MWS, TBS;
  size_t b, rec, x, z, sig, cv, gv, a, mw, out, total;
};
__host__ __device__ inline LpLds lp_lds(int K, int P, int M, int LG, int TB) {
  LpLds L;
  L.BS = P | 1;                                 // a basis row
  L.CVS = (M + 1) | 1;                          // row p of [c | V]
  L.CVN = P * L.CVS;
  L.GVN = (M + 1) * P;
  L.AS = M * M + 2 * M;                         // A (lower triangle, row-major), u, beta
  L.MWS = (M + 1) | 1;                          // row j of [mu | W]
  L.TBS = TB | 1;
  size_t o = 0;
  L.b = o; o += (size_t)LP_ROWS * L.BS;
  L.rec = o; o += (size_t)LG + P;
  L.x = o; o += 8;
  L.z = o; o += (size_t)TB * K;
  L.sig = o; o += LP_TB_MAX;
  L.cv = o; o += (size_t)TB * L.CVN;
  L.gv = o; o += (size_t)TB * L.GVN;
  L.a = o; o += (size_t)TB * L.AS;
  L.mw = o; o += (size_t)(LP_NT / 64) * LP_ROWS * L.MWS;
  L.out = o; o += (size_t)4 * LP_ROWS * L.TBS;
  L.total = o;
  return L;
}

__global__ __launch_bounds__(LP_NT) void k_loo_pointwise(LpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, P = a.P, M = a.M, D = a.D, M1 = M + 1, TB = a.TB, n = a.n;
  const LpLds L = lp_lds(K, P, M, a.LG, TB);
  const int BS = L.BS, CVS = L.CVS, CVN = L.CVN, GVN = L.GVN, AS = L.AS, MWS = L.MWS, TBS = L.TBS;
  double* sB = sm + L.b;
  double* sRec = sm + L.rec;
  double* sX = sm + L.x;
  double* sZ = sm + L.z;
  double* sSig = sm + L.sig;
  double* sCV = sm + L.cv;
  double* sGV = sm + L.gv;
  double* sA = sm + L.a;
  double* sMW = sm + L.mw + (size_t)wave * LP_ROWS * MWS;
  double* sOut = sm + L.out;

  const LpTile tl = a.tiles[blockIdx.x];
  const int i = tl.curve, nr = tl.rows;
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const double* c_Z = ptr_shift(a.c_Z, (size_t)q_chain * a.chain_bytes);
  const double* c_nu = ptr_shift(a.c_nu, (size_t)q_chain * a.chain_bytes);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q_chain * a.chain_bytes);
  const double* c_sigma = ptr_shift(a.c_sigma, (size_t)q_chain * a.chain_bytes);
  const double* c_eta = D > 0 ? ptr_shift(a.c_eta, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  const double* c_xi = D > 0 ? ptr_shift(a.c_xi, (size_t)q_chain * a.chain_bytes_cov) : nullptr;

  // ---- once per workgroup: the tile's basis rows (zero rows beyond the tile), the curve's record and covariates ----
  for (int e = tid; e < LP_ROWS * P; e += LP_NT) {
    const int r = e / P, p = e - r * P;
    double v = 0.0;
    if (r < nr) v = a.mv ? (p == r ? 1.0 : 0.0) : a.B[(size_t)(tl.b0 + r) * P + p];
    sB[r * BS + p] = v;
  }
  const double* rec = a.rec + (size_t)i * a.LREC;
  for (int e = tid; e < a.LG + P; e += LP_NT) sRec[e] = rec[e];      // G(p, p + d) at [d P + p], then s
  if (tid < D) sX[tid] = a.X[i + (size_t)n * tid];
  double yv = 0.0;                                                    // lane j: y of observation j of the tile
  if (lane < nr) yv = a.mv ? a.y[i + (size_t)n * lane] : a.y[tl.y0 + lane];
  const double* sS = sRec + a.LG;

  for (int sb = s_lo; sb < s_hi; sb += TB) {
    const int gn = min(TB, s_hi - sb);
    __syncthreads();                                                  // the previous batch's readers are done (and the set-up above)
    for (int e = tid; e < gn * K; e += LP_NT) {
      const int g = e / K, k = e - g * K;
      sZ[g * K + k] = c_Z[(size_t)(a.first_slot + sb + g) * n * K + i + (size_t)n * k];
    }
    if (tid < gn) sSig[tid] = c_sigma[a.first_slot + sb + tid];
    __syncthreads();
    lc_coefficients(a, c_nu, c_Phi, c_eta, c_xi, sZ, sX, sCV, sb, gn, CVS, CVN, GVN, tid);      // (1) c and V_m at p
    __syncthreads();
    lc_gram_times(a, sRec, sS, sCV, sGV, gn, CVS, CVN, GVN, tid);      // (2) G times each of them at p, over the band window
    __syncthreads();
    lc_u_and_a(a, sCV, sGV, sSig, sA, gn, CVS, CVN, GVN, AS, tid);      // (3) u_m = V_m'e, A_lm = V_m'(G V_l) for l >= m, sigma^2 on the diagonal
    __syncthreads();
    if (tid < gn) lc_factor_beta(sA + tid * AS, M);      // (4) lane g: A = L L' in place, beta = A^-1 u
    __syncthreads();
    // (5) wave w: draws w, w + 4, ..
    for (int g = wave; g < gn; g += LP_NT / 64) {
      lc_mfma_rows(sB, sCV + g * CVN, sMW, nr, P, M1, BS, CVS, MWS, lane);
      __builtin_amdgcn_wave_barrier();
      if (lane < nr) {
        double* w = sMW + lane * MWS;
        const double* Lc = sA + g * AS;
        const double* beta = Lc + M * M + M;
        const double sig = sSig[g];
        double dot = 0.0;
        for (int m = 0; m < M; ++m) dot += w[1 + m] * beta[m];
        const double ej = (yv - w[0]) - dot;
        double hj = 0.0;
        for (int c = 0; c < M; ++c) {
          double x = w[1 + c];
          for (int k2 = 0; k2 < c; ++k2) x -= Lc[c * M + k2] * w[1 + k2];
          x /= Lc[c * M + c];
          w[1 + c] = x;
          hj += x * x;
        }
        const double om = 1.0 - hj;
        const double zj = ej / sqrt(sig * om);
        const double mj = yv - ej / om;
        double* so = sOut + lane * TBS + g;
        so[0] = -0.5 * (1.83787706640934548356 + log(sig) - log(om) + ej * ej / (sig * om));
        so[LP_ROWS * TBS] = 0.5 * erfc(-zj * 0.70710678118654752440);
        so[2 * LP_ROWS * TBS] = mj;
        so[3 * LP_ROWS * TBS] = mj * mj + sig / om;
      }
      __builtin_amdgcn_wave_barrier();                               // the wave's rows are rewritten by its next draw
    }
    __syncthreads();
    // (6) draw-contiguous segments
    for (int e = tid; e < 4 * nr * gn; e += LP_NT) {
      const int g = e % gn, r2 = e / gn, row = r2 % nr, v = r2 / nr;
      a.out[(size_t)v * a.out_stride + (size_t)(tl.out_row + row) * a.C * a.S + (size_t)q_chain * a.S + (size_t)(sb + g)] =
          sOut[(v * LP_ROWS + row) * TBS + g];
    }
  }
}

// x4 <- max(0, x4 - x3^2): the conditional variance from the fourth matrix and the third, for the host's var_trace
__global__ __launch_bounds__(256) void k_loo_pointwise_var(const double* m, double* q, size_t count) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) q[e] = fmax(0.0, q[e] - m[e] * m[e]);
}

}  // namespace

// "" or what k_loo_pointwise cannot take of the sampler's shape: asked before a call allocates anything
std::string loo_pointwise_check(const Ctx& c) {
  size_t bytes = 0;
  (void)lc_pick_tb(c.d, lp_lds, &bytes);
  return lc_shape_check(c, "k_loo_pointwise", "the tile's basis rows, the record and one draw's [c | V]", bytes);
}

// The four matrices of the n_tiles row tiles at `tiles` (device), every chain, slots [first_slot, first_slot + n_slots): matrix v
// at out + v * out_stride, row tl.out_row + j of observation j of a tile, draw fastest, then chain.  B: the dense basis rows the
// tiles index (null for the multivariate model), y: the sampler's observations.  Returns "" or what the kernel cannot take.
std::string launch_loo_pointwise(const Ctx& c, const LpTile* tiles, long long n_tiles, const double* B, const double* y, int first_slot,
                                 int n_slots, double* out, size_t out_stride, hipStream_t st) {
  LpArgs a;
  const std::string bad = lc_fill(a, loo_pointwise_check(c), "k_loo_pointwise", c, tiles != nullptr, tiles, n_tiles, B, y, first_slot, n_slots, out, out_stride);
  if (!bad.empty()) return bad;
  return lc_launch(k_loo_pointwise, "k_loo_pointwise", a, c.d, lp_lds, n_tiles, st);
}

// var[e] = max(0, second[e] - mean[e]^2) in place of second, `count` entries
std::string launch_loo_pointwise_var(const double* mean, double* second, size_t count, hipStream_t st) {
  if (!count) return "";
  const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 65535);
  hipLaunchKernelGGL(k_loo_pointwise_var, dim3(blocks), dim3(256), 0, st, mean, second, count);
  if (hipGetLastError() != hipSuccess) return "k_loo_pointwise_var: launch failed";
  return "";
}

}  // namespace bfmmm
