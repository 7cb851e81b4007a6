// Leave-block-out quantities of chain slots within curves: for every chain q, slot t and listed block b of
// observations of curve i, the joint law of y_b given the REST of the curve and the draw, the scores chi_i integrated out.  With c,
// V, G_i, s_i, A = sigma^2 I_M + V'G_i V = L L' and u = V'(s_i - G_i c) as in kernels_loo_pointwise.hip, W_b the rows
// w_j = (b_j'V_1 .. b_j'V_M) of the block and r_b = y_b - B_b c:
//     A_-b = A - W_b'W_b = L_b L_b',   beta_b = A_-b^-1 (u - W_b'r_b),
//     rt_j = r_j - w_j'beta_b,   m_j = y_j - rt_j,   v_j = sigma^2 (1 + |L_b^-1 w_j|^2),   z_j = rt_j / sqrt v_j        (j in b)
//     l_b = -1/2 [ |b| (log 2 pi + log sigma^2) + log det A - log det A_-b + ( |rt_b|^2 - |L^-1 W_b'rt_b|^2 ) / sigma^2 ].
// Four values per (listed observation, draw) go to the four matrices of k_loo_pointwise, rows x (C S), draw fastest: l_b (the
// same in every row of a block), Phi(z_j), m_j and m_j^2 + v_j.
//
// Geometry: k_loo_pointwise's.  A workgroup of 256 threads takes one row tile, one chain and a run of slots, TB draws at a time.
// A tile's rows are GATHERED: up to LP_ROWS listed observations of one curve, whole blocks only, each row with its observation's
// index in the curve, its basis row in the launch's B and the position and length of its block within the tile (the host's row
// table).  Steps (1) to (4) and the MFMA product [mu | W] = B_tile [c | V] are loo_core.hpp's, with A copied aside before it is
// factorised.  Then the wave of a draw turns mu_j into r_j and goes through the tile's blocks LB_NG at a time, a group of LB_GL
// lanes a block, with wave-level synchronisation between the steps:
//   (a) lane e of the group: entry e of the lower triangle of A_-b = A - sum_j w_j w_j', or of u - sum_j w_j r_j, j in the order the
//       block lists its rows
//   (b) the group's first lane: A_-b = L_b L_b' in place and beta_b by the two triangular solves (lc_factor_beta)
//   (c) a lane a row: rt_j in place of r_j
//   (d) lane e: (W_b'rt_b)_e, e < M, and |rt_b|^2 (e = M), j in order
//   (e) the first lane: x = L^-1 W_b'rt_b and l_b
//   (f) a lane a row: L_b^-1 w_j in place in its row, the four values -> the staging table
// The scratch of a wave is LB_NG records of M M + 3 M + 2 doubles, whatever the number of blocks.  fp64, vector stores only, no
// atomics; every sum has a fixed order that depends on (block, chain, slot) alone: the bits of a block do not depend on the blocks
// that share its tile, the chunk, the grid, TB or its place in the list.
#include "model.hpp"
#include "launchers.hpp"
#include "loo_core.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

constexpr int LB_NT = LC_NT;
constexpr int LB_TB_MAX = LC_TB_MAX;
constexpr int LB_GL = 16;                      // lanes of a block's group
constexpr int LB_NG = 64 / LB_GL;              // blocks in flight in a wave

// loo_core.hpp's record with the row table behind the tile list, where it always was: with `rows` at the end of the record the
// compiler schedules k_loo_blocks differently and its device time grows by 1% (measured at blocks of 50)
struct LbRows { const LbRow* rows; };
struct LbArgs : LcArgsHead<LbTile>, LbRows, LcArgsTail {};

// LDS doubles of k_loo_blocks
struct LbLds {
  int BS, CVS, CVN, GVN, AS, MWS, TBS, GS;
  size_t b, rec, x, z, sig, cv, gv, a, ak, mw, y, blk, scr, out, total;
};
__host__ __device__ inline LbLds lb_lds(int K, int P, int M, int LG, int TB) {
  LbLds L;
  L.BS = P | 1;                                 // a basis row
  L.CVS = (M + 1) | 1;                          // row p of [c | V]
  L.CVN = P * L.CVS;
  L.GVN = (M + 1) * P;
  L.AS = M * M + 2 * M;                         // A (lower triangle, row-major), u, beta
  L.MWS = (M + 1) | 1;                          // row j of [r | W]
  L.TBS = TB | 1;
  L.GS = M * M + 3 * M + 2;                     // a group: A_-b, u - W_b'r_b, beta_b, W_b'rt_b with |rt_b|^2, l_b
  size_t o = 0;
  L.b = o; o += (size_t)LP_ROWS * L.BS;
  L.rec = o; o += (size_t)LG + P;
  L.x = o; o += 8;
  L.z = o; o += (size_t)TB * K;
  L.sig = o; o += LB_TB_MAX;
  L.cv = o; o += (size_t)TB * L.CVN;
  L.gv = o; o += (size_t)TB * L.GVN;
  L.a = o; o += (size_t)TB * L.AS;
  L.ak = o; o += (size_t)TB * M * M;            // A before its factorisation
  L.mw = o; o += (size_t)(LB_NT / 64) * LP_ROWS * L.MWS;
  L.y = o; o += LP_ROWS;
  L.blk = o; o += LP_ROWS + 1;                  // as ints: (first row, length) of the tile's blocks, then their number
  L.scr = o; o += (size_t)(LB_NT / 64) * LB_NG * L.GS;
  L.out = o; o += (size_t)4 * LP_ROWS * L.TBS;
  L.total = o;
  return L;
}

// the lanes of a wave have written LDS that other lanes of it read next
__device__ __forceinline__ void lb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(LB_NT) void k_loo_blocks(LbArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, P = a.P, M = a.M, D = a.D, M1 = M + 1, TB = a.TB, n = a.n;
  const LbLds L = lb_lds(K, P, M, a.LG, TB);
  const int BS = L.BS, CVS = L.CVS, CVN = L.CVN, GVN = L.GVN, AS = L.AS, MWS = L.MWS, TBS = L.TBS, GS = L.GS;
  double* sB = sm + L.b;
  double* sRec = sm + L.rec;
  double* sX = sm + L.x;
  double* sZ = sm + L.z;
  double* sSig = sm + L.sig;
  double* sCV = sm + L.cv;
  double* sGV = sm + L.gv;
  double* sA = sm + L.a;
  double* sAk = sm + L.ak;
  double* sMW = sm + L.mw + (size_t)wave * LP_ROWS * MWS;
  double* sY = sm + L.y;
  int* sBlk = (int*)(sm + L.blk);
  double* sOut = sm + L.out;

  const LbTile tl = a.tiles[blockIdx.x];
  const LbRow* rt = a.rows + tl.row0;
  const int i = tl.curve, nr = min(tl.rows, LP_ROWS);
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const double* c_Z = ptr_shift(a.c_Z, (size_t)q_chain * a.chain_bytes);
  const double* c_nu = ptr_shift(a.c_nu, (size_t)q_chain * a.chain_bytes);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q_chain * a.chain_bytes);
  const double* c_sigma = ptr_shift(a.c_sigma, (size_t)q_chain * a.chain_bytes);
  const double* c_eta = D > 0 ? ptr_shift(a.c_eta, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  const double* c_xi = D > 0 ? ptr_shift(a.c_xi, (size_t)q_chain * a.chain_bytes_cov) : nullptr;

  // ---- once per workgroup: the tile's gathered basis rows (zero rows beyond the tile), y, the block table, the curve's record ----
  for (int e = tid; e < LP_ROWS * P; e += LB_NT) {
    const int r = e / P, p = e - r * P;
    double v = 0.0;
    if (r < nr) v = a.mv ? (p == rt[r].obs ? 1.0 : 0.0) : a.B[(size_t)rt[r].b * P + p];
    sB[r * BS + p] = v;
  }
  const double* rec = a.rec + (size_t)i * a.LREC;
  for (int e = tid; e < a.LG + P; e += LB_NT) sRec[e] = rec[e];      // G(p, p + d) at [d P + p], then s
  if (tid < D) sX[tid] = a.X[i + (size_t)n * tid];
  if (wave == 0) {
    int bpos = -1, blen = 0;
    double yv = 0.0;
    if (lane < nr) {
      const LbRow rw = rt[lane];
      bpos = rw.bpos; blen = rw.blen;
      yv = a.mv ? a.y[i + (size_t)n * rw.obs] : a.y[tl.y0 + rw.obs];
    }
    sY[lane] = yv;
    const bool first = bpos == lane;                                  // the first row of its block
    const unsigned long long mask = __ballot(first);
    if (first) {
      const int k = __popcll(mask & ((1ull << lane) - 1ull));
      sBlk[2 * k] = lane;
      sBlk[2 * k + 1] = max(0, min(blen, nr - lane));
    }
    if (lane == 0) sBlk[2 * LP_ROWS] = __popcll(mask);
  }
  const double* sS = sRec + a.LG;
  const int grp = lane / LB_GL, gl = lane % LB_GL;
  double* scr = sm + L.scr + (size_t)(wave * LB_NG + grp) * GS;       // the group's record
  double* beta_b = scr + M * M + M;
  double* tb = scr + M * M + 2 * M;
  const int NTRI = M * (M + 1) / 2;

  for (int sb = s_lo; sb < s_hi; sb += TB) {
    const int gn = min(TB, s_hi - sb);
    __syncthreads();                                                  // the previous batch's readers are done (and the set-up above)
    for (int e = tid; e < gn * K; e += LB_NT) {
      const int g = e / K, k = e - g * K;
      sZ[g * K + k] = c_Z[(size_t)(a.first_slot + sb + g) * n * K + i + (size_t)n * k];
    }
    if (tid < gn) sSig[tid] = c_sigma[a.first_slot + sb + tid];
    __syncthreads();
    lc_coefficients(a, c_nu, c_Phi, c_eta, c_xi, sZ, sX, sCV, sb, gn, CVS, CVN, GVN, tid);      // (1)
    __syncthreads();
    lc_gram_times(a, sRec, sS, sCV, sGV, gn, CVS, CVN, GVN, tid);                               // (2)
    __syncthreads();
    lc_u_and_a(a, sCV, sGV, sSig, sA, gn, CVS, CVN, GVN, AS, tid);                              // (3)
    __syncthreads();
    for (int e = tid; e < gn * NTRI; e += LB_NT) {                    // A aside: its lower triangle
      const int g = e / NTRI, r = e - g * NTRI;
      int c = 0;
      while ((c + 1) * (c + 2) / 2 <= r) ++c;
      const int k = r - c * (c + 1) / 2;
      sAk[g * M * M + c * M + k] = sA[g * AS + c * M + k];
    }
    __syncthreads();
    if (tid < gn) lc_factor_beta(sA + tid * AS, M);                   // (4)
    __syncthreads();
    const int nblk = __builtin_amdgcn_readfirstlane(sBlk[2 * LP_ROWS]);
    // (5) wave w: draws w, w + 4, ..
    for (int g = wave; g < gn; g += LB_NT / 64) {
      lc_mfma_rows(sB, sCV + g * CVN, sMW, nr, P, M1, BS, CVS, MWS, lane);
      lb_wave_sync();
      const double* Lc = sA + g * AS;
      const double* Ak = sAk + g * M * M;
      const double* u = Lc + M * M;
      const double sig = sSig[g];
      if (lane < nr) sMW[lane * MWS] = sY[lane] - sMW[lane * MWS];    // r_j
      double ldL = 0.0;
      for (int c = 0; c < M; ++c) ldL += log(Lc[c * M + c]);
      lb_wave_sync();
      for (int b0 = 0; b0 < nblk; b0 += LB_NG) {
        const bool act = b0 + grp < nblk;
        const int st = act ? sBlk[2 * (b0 + grp)] : 0, len = act ? sBlk[2 * (b0 + grp) + 1] : 0;
        const double* wb = sMW + st * MWS;                            // the block's rows [r | w]
        // (a) A_-b and u - W_b'r_b
        if (act) {
          for (int e = gl; e < NTRI + M; e += LB_GL) {
            double s_ = 0.0;
            if (e < NTRI) {
              int c = 0;
              while ((c + 1) * (c + 2) / 2 <= e) ++c;
              const int k = e - c * (c + 1) / 2;
              for (int j = 0; j < len; ++j) s_ += wb[j * MWS + 1 + c] * wb[j * MWS + 1 + k];
              scr[c * M + k] = Ak[c * M + k] - s_;
            } else {
              const int m = e - NTRI;
              for (int j = 0; j < len; ++j) s_ += wb[j * MWS + 1 + m] * wb[j * MWS];
              scr[M * M + m] = u[m] - s_;
            }
          }
        }
        lb_wave_sync();
        // (b) L_b and beta_b
        if (act && gl == 0) lc_factor_beta(scr, M);
        lb_wave_sync();
        // (c) rt_j
        if (act) {
          for (int j = gl; j < len; j += LB_GL) {
            double* w = sMW + (st + j) * MWS;
            double dot = 0.0;
            for (int m = 0; m < M; ++m) dot += w[1 + m] * beta_b[m];
            w[0] = w[0] - dot;
          }
        }
        lb_wave_sync();
        // (d) W_b'rt_b and |rt_b|^2
        if (act) {
          for (int e = gl; e <= M; e += LB_GL) {
            double s_ = 0.0;
            if (e < M) { for (int j = 0; j < len; ++j) s_ += wb[j * MWS + 1 + e] * wb[j * MWS]; }
            else { for (int j = 0; j < len; ++j) s_ += wb[j * MWS] * wb[j * MWS]; }
            tb[e] = s_;
          }
        }
        lb_wave_sync();
        // (e) l_b
        if (act && gl == 0) {
          double ss = 0.0, ldb = 0.0;
          for (int c = 0; c < M; ++c) {
            double x = tb[c];
            for (int k2 = 0; k2 < c; ++k2) x -= Lc[c * M + k2] * tb[k2];
            x /= Lc[c * M + c];
            tb[c] = x;
            ss += x * x;
            ldb += log(scr[c * M + c]);
          }
          tb[M + 1] = -0.5 * ((double)len * (1.83787706640934548356 + log(sig)) + 2.0 * (ldL - ldb) + (tb[M] - ss) / sig);
        }
        lb_wave_sync();
        // (f) the rows' values
        if (act) {
          const double lb = tb[M + 1];
          for (int j = gl; j < len; j += LB_GL) {
            const int row = st + j;
            double* w = sMW + row * MWS;
            double hj = 0.0;
            for (int c = 0; c < M; ++c) {
              double x = w[1 + c];
              for (int k2 = 0; k2 < c; ++k2) x -= scr[c * M + k2] * w[1 + k2];
              x /= scr[c * M + c];
              w[1 + c] = x;
              hj += x * x;
            }
            const double vj = sig * (1.0 + hj);
            const double rj = w[0];
            const double zj = rj / sqrt(vj);
            const double mj = sY[row] - rj;
            double* so = sOut + row * TBS + g;
            so[0] = lb;
            so[LP_ROWS * TBS] = 0.5 * erfc(-zj * 0.70710678118654752440);
            so[2 * LP_ROWS * TBS] = mj;
            so[3 * LP_ROWS * TBS] = mj * mj + vj;
          }
        }
        lb_wave_sync();                                               // the groups' records are rewritten by the next blocks
      }
    }
    __syncthreads();
    // (6) draw-contiguous segments
    for (int e = tid; e < 4 * nr * gn; e += LB_NT) {
      const int g = e % gn, r2 = e / gn, row = r2 % nr, v = r2 / nr;
      a.out[(size_t)v * a.out_stride + (size_t)(tl.row0 + row) * a.C * a.S + (size_t)q_chain * a.S + (size_t)(sb + g)] =
          sOut[(v * LP_ROWS + row) * TBS + g];
    }
  }
}

}  // namespace

// "" or what k_loo_blocks cannot take of the sampler's shape: asked before a call allocates anything
std::string loo_blocks_check(const Ctx& c) {
  size_t bytes = 0;
  (void)lc_pick_tb(c.d, lb_lds, &bytes);
  return lc_shape_check(c, "k_loo_blocks", "the tile's basis rows, the record, one draw's [c | V] and the blocks' records", bytes);
}

// The four matrices of the n_tiles row tiles at `tiles` with their rows at `rows` (device), every chain, slots [first_slot,
// first_slot + n_slots): matrix v at out + v * out_stride, row tl.row0 + j of row j of a tile, draw fastest, then chain.  B: the
// dense basis rows the row table indexes (null for the multivariate model), y: the sampler's observations.  The tables are the
// host's: every row's block lies within its tile.  Returns "" or what the kernel cannot take.
std::string launch_loo_blocks(const Ctx& c, const LbTile* tiles, long long n_tiles, const LbRow* rows, const double* B, const double* y,
                              int first_slot, int n_slots, double* out, size_t out_stride, hipStream_t st) {
  LbArgs a;
  const std::string bad = lc_fill(a, loo_blocks_check(c), "k_loo_blocks", c, tiles && rows, tiles, n_tiles, B, y, first_slot, n_slots, out, out_stride);
  if (!bad.empty()) return bad;
  a.rows = rows;
  return lc_launch(k_loo_blocks, "k_loo_blocks", a, c.d, lb_lds, n_tiles, st);
}

}  // namespace bfmmm
