// Pooled per-curve covariance surfaces from chain slots: for every chain q, slot t, curve i and rows E1_g, E2_h of
// two evaluation bases (G1 x P and G2 x P, row-major; E2 = E1 where only one is given)
//     V_im      = sum_k Z_ik (phi_km + sum_d x_id xi_kmd)                    (xi: covariance-adjusted only; the V_im of 7d / 7e)
//     W1[g][m]  = E1_g . V_im,   W2[h][m] = E2_h . V_im
//     C_i(g, h) = sum_m W1[g][m] W2[h][m]                                    (= sum_k sum_k' Z_ik Z_ik' C^(k,k')(g, h))
// a sum over k and k' (label-invariant) of products of two factors that change sign together (sign-invariant): the chains pool as
// they are.  Of the N = C S draws of slots [first_slot, first_slot + S):
//     mean[(r G1 + g) G2 + h]             the mean of C_i(g, h) over the N draws (result row r is curve curves[r], or r),
//     sd[(r G1 + g) G2 + h]               the sample sd (N - 1; NaN for one draw), in a second pass over the draws,
//     chain_mean[((r C + q) G1 + g) G2 + h]   the mean over the S slots of chain q;
// diagonal: only g = h, at [r G1 + g] and [(r C + q) G1 + g].
//
//   k_cov_project   T[((cs KP + k) GP + g) RS + dd MP + m] = E_g . phi_km (dd = 0) or E_g . xi_km,dd-1 of draw cs = q S + (t -
//                   first_slot): everything one draw contributes lies together, a (k, tile of 16 g) piece is 16 RS consecutive
//                   doubles (a multiple of 128 bytes from a 128-byte boundary), so staging reads whole 64-byte segments.  g is
//                   padded to the tile (GP), m to the MFMA's four (MP = 4 MB), k to the k-slices (KP), all with zeros; RS = D1 MP
//                   + 2 doubles between rows makes the LDS image of a piece, a plain copy, free of bank conflicts for the
//                   operand reads below (16 rows x 2 values of m per half wave: 16 RS mod 32 distinct even numbers).
//   k_curve_cov     A workgroup of four waves owns a tile of 16 rows g, up to four tiles of 16 columns h and four curves, one
//                   per wave.  The tables' pieces of a draw (of a slice of KS values of k where a whole draw does not fit) are
//                   staged in LDS once for the four curves, the next stage's loads in flight while this one is consumed.  Lane
//                   l of a wave forms its own MFMA operands on the VALU, W[row l & 15][m = 4 mb + (l >> 4)] = sum_k Z_ik (T +
//                   sum_d x_id Tx), k in order, d in order inside; a draw's d of a tile is v_mfma_f64_16x16x4_f64 over m in
//                   blocks of four from a zero accumulator (lane l feeds A[row l & 15][m l >> 4] and B[m l >> 4][col l & 15] and
//                   receives D[row (l >> 4) + 4 reg][col l & 15]).  diagonal: the tile (gt, gt) only, both operands the same
//                   registers, only g = h stored.
// Summation order, fixed per entry whatever the tile grouping, the grid, the chunk or the call: s_q = sum_t d(q, t) in slot order
// from 0, the pooled sum sum_q s_q in chain order from 0, mean = that / N, chain_mean = s_q / S; the sd pass forms d by the same
// instructions and sums (d - mean)^2 in the same order, sd = sqrt(that / (N - 1)).  No atomics, no split over the draws, no
// scratch.  Every copy of W[g][m] is formed by the same instructions from the same staged values, so with E2 = E1 d(g, h) and
// d(h, g) are the same M products accumulated in the same order: the surface is symmetric bit for bit.
#include "model.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <string>

// the MFMA fuses internally; W and the accumulation over the draws must round as the restatement's do
#pragma clang fp contract(off)

namespace bfmmm {

namespace {

constexpr int COV_NT = 256;
constexpr int COV_NW = COV_NT / 64;      // waves = curves of a workgroup
constexpr int COV_MMAX = 16;             // n_eigen: four chained MFMAs
constexpr int COV_DMAX = 8;
constexpr int COV_NE = 20;               // staged values per thread and stage at most
constexpr int COV_STAGE_MAX = COV_NT * COV_NE;
constexpr int COV_CT = 4;                // column tiles of a wave at most

struct CovArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Z, *c_Phi, *c_xi, *X;
  size_t chain_bytes, chain_bytes_cov;
  const double *tab1, *tab2;      // the projection tables of E1 and E2 (tab2 == tab1: E2 = E1)
  size_t ds1, ds2;                // doubles of a draw in either
  const int* curves;              // the curve of result row r of the call, or null: curve r
  int r0, rows;                   // the chunk's result rows
  int n, K, P, M, D, DX;          // DX: covariates that enter V (D where covariance-adjusted, else 0)
  int C, first_slot, S;
  int G1, G2, GP1, GP2, RS, KS, NKS, KP, stage, diagonal;
  double *mean, *sd, *chain_mean; // of the chunk
};

// one workgroup per draw; consecutive threads write consecutive doubles
__global__ __launch_bounds__(COV_NT) void k_cov_project(CovArgs a, const double* E, int G, int GP, int MP, double* tab) {
  const int cs = (int)blockIdx.x, tid = threadIdx.x;
  const int K = a.K, P = a.P, M = a.M, D = a.D, D1 = a.DX + 1, RS = a.RS;
  const int q = cs / a.S;
  const size_t t = (size_t)(a.first_slot + cs - q * a.S);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q * a.chain_bytes) + t * K * P * M;
  const double* c_xi = a.DX > 0 ? ptr_shift(a.c_xi, (size_t)q * a.chain_bytes_cov) + t * K * P * D * M : nullptr;
  const int perk = GP * RS, total = a.KP * perk;
  double* out = tab + (size_t)cs * total;
  for (int e = tid; e < total; e += COV_NT) {
    const int k = e / perk, r = e - k * perk, g = r / RS, c = r - g * RS, dd = c / MP, m = c - dd * MP;
    double s = 0.0;
    if (k < K && g < G && dd < D1 && m < M) {
      const double* th;                                          // theta[p] = th[p * st]
      int st;
      if (dd == 0) { th = c_Phi + k + (size_t)K * P * m; st = K; }                 // Phi: [k + K (p + P m)]
      else { th = c_xi + (size_t)P * ((dd - 1) + D * (m + M * k)); st = 1; }       // xi: [p + P (d + D (m + M k))]
      const double* eg = E + (size_t)g * P;
      for (int p = 0; p < P; ++p) s += eg[p] * th[(size_t)p * st];
    }
    out[e] = s;
  }
}

// w[mb] += z (T + sum_d x_d Tx_d) for this lane's m of every block of four; t: the lane's entry of direction 0 of its row
template <int MB>
__device__ __forceinline__ void cov_w(const double* t, double z, const double* sx, int DX, double (&w)[MB]) {
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    double b = t[4 * mb];
    for (int d = 0; d < DX; ++d) b += sx[d] * t[(1 + d) * 4 * MB + 4 * mb];
    w[mb] += z * b;
  }
}

struct CovBlock {
  int gt, ct0, nct, perk, row, live;      // row tile, first column tile and their number, doubles of a staged k, result row of the wave
};

// One pass over the draws for the tiles of a wave: tot[ct] = sum_q sum_t f(d), f(d) = d (PASS 0) or (d - mu)^2 (PASS 1).
template <int MB, int CT, int PASS>
__device__ __forceinline__ void cov_pass(const CovArgs& a, const CovBlock& b, double* sT, double (*sZ)[COV_NW][KMAX], const double* sx,
                                         const int* sIdx, const int (&soff)[COV_NE], unsigned bmask, int tid, double4_t (&tot)[CT],
                                         const double4_t (&mu)[CT]) {
  const int lane = tid & 63, wave = tid >> 6;
  const int K = a.K, KS = a.KS, NKS = a.NKS, RS = a.RS, perk = b.perk;
  const int NS = a.C * a.S * NKS;                                 // stages: (draw, k-slice)
  const size_t slot = (size_t)a.n * K;
  const double4_t zero = {0.0, 0.0, 0.0, 0.0};
  const int zc = tid < COV_NW * KMAX ? sIdx[tid >> 3] : -1, zk = tid & 7;
  double v[COV_NE], zv = 0.0;
  auto fetch = [&](int g) {
    const int cs = g / NKS, ks = g - cs * NKS;
    const double* bA = a.tab1 + (size_t)cs * a.ds1 + (size_t)ks * KS * a.GP1 * RS;
    const double* bB = a.tab2 + (size_t)cs * a.ds2 + (size_t)ks * KS * a.GP2 * RS;
#pragma unroll
    for (int u = 0; u < COV_NE; ++u) v[u] = soff[u] >= 0 ? (((bmask >> u) & 1u) ? bB : bA)[soff[u]] : 0.0;
    if (zc >= 0 && zk < K) {
      const int q = cs / a.S;
      zv = (ptr_shift(a.c_Z, (size_t)q * a.chain_bytes) + (size_t)(a.first_slot + cs - q * a.S) * slot)[(size_t)zk * a.n + zc];
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int u = 0; u < COV_NE; ++u)
      if (soff[u] >= 0) sT[buf * a.stage + tid + COV_NT * u] = v[u];
    if (tid < COV_NW * KMAX) sZ[buf][tid >> 3][zk] = zv;          // zeros for k >= K and for rows past the chunk
  };
  double4_t s[CT];
  double wa[MB], wb[CT][MB];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    s[ct] = zero; tot[ct] = zero;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) wb[ct][mb] = 0.0;
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) wa[mb] = 0.0;
  const int loff = (lane & 15) * RS + (lane >> 4);
  fetch(0);
  put(0);
  __syncthreads();
  for (int g = 0; g < NS; ++g) {
    if (g + 1 < NS) fetch(g + 1);
    const int cs = g / NKS, ks = g - cs * NKS;
    if (b.live) {
      const double* tb = sT + (g & 1) * a.stage + loff;
      const double* zb = sZ[g & 1][wave] + ks * KS;
      const int klen = min(KS, K - ks * KS);
      for (int kk = 0; kk < klen; ++kk) {
        const double z = zb[kk];
        const double* tk = tb + kk * perk;
        cov_w<MB>(tk, z, sx, a.DX, wa);
        if (!a.diagonal) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            if (ct < b.nct) cov_w<MB>(tk + (16 + 16 * ct) * RS, z, sx, a.DX, wb[ct]);
        }
      }
      if (ks == NKS - 1) {                                        // W of the draw is complete
        const int q = cs / a.S;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (ct < b.nct) {
            double4_t d = zero;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              d = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[mb], a.diagonal ? wa[mb] : wb[ct][mb], d, 0, 0, 0);
              wb[ct][mb] = 0.0;
            }
            if (PASS == 0) s[ct] += d;
            else { const double4_t e = d - mu[ct]; s[ct] += e * e; }
          }
        }
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) wa[mb] = 0.0;
        if (cs - q * a.S == a.S - 1) {                            // the chain's last draw: s_q is complete
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            tot[ct] += s[ct];
            if (PASS == 0 && a.chain_mean && ct < b.nct) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int gl = (lane >> 4) + 4 * r, gg = b.gt * 16 + gl, hh = (b.ct0 + ct) * 16 + (lane & 15);
                const size_t rb = (size_t)b.row * a.C + q;
                if (a.diagonal) { if (gl == (lane & 15) && gg < a.G1) a.chain_mean[rb * a.G1 + gg] = s[ct][r] / (double)a.S; }
                else if (gg < a.G1 && hh < a.G2) a.chain_mean[(rb * a.G1 + gg) * a.G2 + hh] = s[ct][r] / (double)a.S;
              }
            }
            s[ct] = zero;
          }
        }
      }
    }
    if (g + 1 < NS) put((g + 1) & 1);      // the buffer stage g - 1 was read from, before the barrier that ended stage g - 1's turn
    __syncthreads();
  }
}

// two waves per SIMD wherever the instance's registers allow it without scratch (all but three and four MFMAs on four tiles)
template <int MB, int CT>
__global__ __launch_bounds__(COV_NT, (MB <= 2 || CT == 1) ? 2 : 1) void k_curve_cov(CovArgs a, int tiles1, int ncg) {
  extern __shared__ __attribute__((aligned(16))) double sT[];     // two stages
  __shared__ double sZ[2][COV_NW][KMAX];
  __shared__ double sX[COV_NW][COV_DMAX];
  __shared__ int sIdx[COV_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned bx = blockIdx.x;
  const int cgp = (int)(bx % (unsigned)ncg), gt = (int)((bx / (unsigned)ncg) % (unsigned)tiles1), grp = (int)(bx / ((unsigned)ncg * (unsigned)tiles1));
  CovBlock b;
  b.gt = gt;
  b.ct0 = a.diagonal ? gt : cgp * CT;
  b.nct = a.diagonal ? 1 : min(CT, a.GP2 / 16 - b.ct0);
  b.perk = (16 + (a.diagonal ? 0 : 16 * b.nct)) * a.RS;
  b.row = grp * COV_NW + wave;
  b.live = b.row < a.rows;
  if (tid < COV_NW) {
    const int row = grp * COV_NW + tid;
    sIdx[tid] = row < a.rows ? (a.curves ? a.curves[a.r0 + row] : a.r0 + row) : -1;
  }
  __syncthreads();
  if (tid < COV_NW * COV_DMAX) {
    const int w = tid >> 3, d = tid & 7;
    sX[w][d] = (d < a.DX && sIdx[w] >= 0) ? a.X[sIdx[w] + (size_t)a.n * d] : 0.0;
  }
  // what this thread stages of every stage: element e of [kk][16 rows of the row tile | 16 nct rows of the column tiles][RS]
  int soff[COV_NE];
  unsigned bmask = 0;
  const int cnt = a.KS * b.perk;
#pragma unroll
  for (int u = 0; u < COV_NE; ++u) {
    const int e = tid + COV_NT * u;
    soff[u] = -1;
    if (e < cnt) {
      const int kk = e / b.perk, r = e - kk * b.perk;
      if (r < 16 * a.RS) soff[u] = (kk * a.GP1 + gt * 16) * a.RS + r;
      else { soff[u] = (kk * a.GP2 + b.ct0 * 16) * a.RS + r - 16 * a.RS; bmask |= 1u << u; }
    }
  }
  __syncthreads();
  const double N = (double)a.C * (double)a.S;
  double4_t tot[CT], mu[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) mu[ct] = double4_t{0.0, 0.0, 0.0, 0.0};
  auto store = [&](double* out, const double4_t (&val)[CT]) {
    if (!b.live) return;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (ct < b.nct) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gl = (lane >> 4) + 4 * r, gg = gt * 16 + gl, hh = (b.ct0 + ct) * 16 + (lane & 15);
          if (a.diagonal) { if (gl == (lane & 15) && gg < a.G1) out[(size_t)b.row * a.G1 + gg] = val[ct][r]; }
          else if (gg < a.G1 && hh < a.G2) out[((size_t)b.row * a.G1 + gg) * a.G2 + hh] = val[ct][r];
        }
      }
    }
  };
  cov_pass<MB, CT, 0>(a, b, sT, sZ, sX[wave], sIdx, soff, bmask, tid, tot, mu);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) mu[ct] = tot[ct] / N;
  store(a.mean, mu);
  if (!a.sd) return;
  cov_pass<MB, CT, 1>(a, b, sT, sZ, sX[wave], sIdx, soff, bmask, tid, tot, mu);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[ct][r] = sqrt(tot[ct][r] / (N - 1.0));      // one draw: 0 / 0
  }
  store(a.sd, tot);
}

// what the model and the call's grids fix: MFMAs per draw and tile, covariates in V, row stride, k-slices, column tiles per wave
struct CovGeom {
  int MB = 0, DX = 0, RS = 0, KS = 0, NKS = 0, KP = 0, GP1 = 0, GP2 = 0, CT = 0, stage = 0;
};

std::string cov_geom(const Ctx& c, const CovCall& f, CovGeom& g) {
  const Dims& d = c.d;
  if (d.K < 1 || d.K > KMAX) return "K outside 1 .. 8";
  if (d.M < 1 || d.M > COV_MMAX) return "n_eigen outside 1 .. 16";
  if (d.D < 0 || d.D > COV_DMAX) return "more than 8 covariates";
  if (d.P < 1) return "P below 1";
  if (f.G1 < 1 || f.G2 < 1 || f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "range outside the chain storage";
  if ((long long)c.nch * f.n_slots > (1LL << 22)) return "more than 2^22 draws";
  if ((long long)d.n * KMAX > 0x7fffffffLL) return "n K above 2^31 - 1";
  g.MB = (d.M + 3) / 4;
  g.DX = (d.D > 0 && c.covariance_adj) ? d.D : 0;
  g.RS = (g.DX + 1) * 4 * g.MB + 2;
  const long long gp1 = ((long long)f.G1 + 15) / 16 * 16, gp2 = ((long long)f.G2 + 15) / 16 * 16;
  if (KMAX * std::max(gp1, gp2) * g.RS > 0x7fffffffLL) return "G K (n_eigen + 2) (1 + D) above 2^31 - 1";
  g.GP1 = (int)gp1; g.GP2 = (int)gp2;
  g.CT = (!f.diagonal && g.GP2 > 16 && (16 + 16 * COV_CT) * g.RS <= COV_STAGE_MAX) ? COV_CT : 1;
  const int perk = (16 + (f.diagonal ? 0 : 16 * g.CT)) * g.RS;
  g.KS = std::max(1, std::min(d.K, COV_STAGE_MAX / perk));
  g.NKS = (d.K + g.KS - 1) / g.KS;
  g.KP = g.NKS * g.KS;
  g.stage = g.KS * perk;
  return "";
}

CovArgs cov_args(const Ctx& c, const CovCall& f, const CovGeom& g) {
  const Dims& d = c.d;
  CovArgs a;
  a.c_Z = c.c_Z; a.c_Phi = c.c_Phi; a.c_xi = g.DX > 0 ? c.c_xi : nullptr; a.X = g.DX > 0 ? c.X : nullptr;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.tab1 = f.tab1; a.tab2 = f.tab2 ? f.tab2 : f.tab1;
  a.ds1 = (size_t)g.KP * g.GP1 * g.RS; a.ds2 = (size_t)g.KP * g.GP2 * g.RS;
  a.curves = f.curves; a.r0 = 0; a.rows = 0;
  a.n = d.n; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.DX = g.DX;
  a.C = c.nch; a.first_slot = f.first_slot; a.S = f.n_slots;
  a.G1 = f.G1; a.G2 = f.G2; a.GP1 = g.GP1; a.GP2 = g.GP2; a.RS = g.RS; a.KS = g.KS; a.NKS = g.NKS; a.KP = g.KP; a.stage = g.stage;
  a.diagonal = f.diagonal ? 1 : 0;
  a.mean = a.sd = a.chain_mean = nullptr;
  return a;
}

template <int MB, int CT>
std::string cov_launch(const CovArgs& a, hipStream_t st) {
  const long long tiles1 = a.GP1 / 16, ncg = a.diagonal ? 1 : (a.GP2 / 16 + CT - 1) / CT;
  const long long blocks = ((long long)a.rows + COV_NW - 1) / COV_NW * tiles1 * ncg;
  if (blocks > 0x7fffffffLL) return "k_curve_cov: too many workgroups in one chunk";
  const size_t lds = sizeof(double) * 2 * (size_t)a.stage;
  if (hipFuncSetAttribute((const void*)k_curve_cov<MB, CT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 2 * COV_STAGE_MAX)) !=
      hipSuccess) {
    (void)hipGetLastError();
    return "k_curve_cov: cannot set the LDS size";
  }
  hipLaunchKernelGGL((k_curve_cov<MB, CT>), dim3((unsigned)blocks), dim3(COV_NT), lds, st, a, (int)tiles1, (int)ncg);
  if (hipGetLastError() != hipSuccess) return "k_curve_cov: launch failed";
  return "";
}

template <int CT>
std::string cov_launch_mb(int MB, const CovArgs& a, hipStream_t st) {
  switch (MB) {
    case 1: return cov_launch<1, CT>(a, st);
    case 2: return cov_launch<2, CT>(a, st);
    case 3: return cov_launch<3, CT>(a, st);
    default: return cov_launch<4, CT>(a, st);
  }
}

}  // namespace

std::string cov_check(const Ctx& c, const CovCall& f) {
  CovGeom g;
  return cov_geom(c, f, g);
}

size_t cov_table_doubles(const Ctx& c, const CovCall& f, int which) {
  CovGeom g;
  if (!cov_geom(c, f, g).empty()) return 0;
  return (size_t)c.nch * f.n_slots * g.KP * (which ? g.GP2 : g.GP1) * g.RS;
}

// the projection tables of the call: f.tab1 of E1 and, where E2 is given, f.tab2 of E2
std::string launch_cov_project(const Ctx& c, const CovCall& f, hipStream_t st) {
  CovGeom g;
  const std::string err = cov_geom(c, f, g);
  if (!err.empty()) return "k_cov_project: " + err;
  if (!f.E1 || !f.tab1 || (f.E2 && !f.tab2)) return "k_cov_project: bad arguments";
  const CovArgs a = cov_args(c, f, g);
  const dim3 grid((unsigned)(a.C * a.S));
  hipLaunchKernelGGL(k_cov_project, grid, dim3(COV_NT), 0, st, a, f.E1, f.G1, g.GP1, 4 * g.MB, f.tab1);
  if (f.E2) hipLaunchKernelGGL(k_cov_project, grid, dim3(COV_NT), 0, st, a, f.E2, f.G2, g.GP2, 4 * g.MB, f.tab2);
  if (hipGetLastError() != hipSuccess) return "k_cov_project: launch failed";
  return "";
}

// mean, sd (or null) and chain_mean (or null) of result rows [r0, r0 + rows) of the call into the chunk's buffers (row r0 first)
std::string launch_curve_cov(const Ctx& c, const CovCall& f, int r0, int rows, double* mean, double* sd, double* chain_mean, hipStream_t st) {
  CovGeom g;
  const std::string err = cov_geom(c, f, g);
  if (!err.empty()) return "k_curve_cov: " + err;
  if (rows < 1 || r0 < 0 || !mean || !f.tab1 || (!f.curves && r0 + rows > c.d.n) || (f.diagonal && (f.tab2 || f.G2 != f.G1)))
    return "k_curve_cov: bad arguments";
  CovArgs a = cov_args(c, f, g);
  a.r0 = r0; a.rows = rows; a.mean = mean; a.sd = sd; a.chain_mean = chain_mean;
  return g.CT == 1 ? cov_launch_mb<1>(g.MB, a, st) : cov_launch_mb<COV_CT>(g.MB, a, st);
}

}  // namespace bfmmm
