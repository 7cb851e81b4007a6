// Cluster covariance surfaces with the labels aligned, from chain slots (the reference's FCovCI over a chain batch):
// for every chain q, slot t, pair r = (k, l) of aligned components and rows E1_g, E2_h of two evaluation bases (G1 x P and G2 x P,
// row-major; E2 = E1 where only one is given), with cs = q S + (t - first_slot) and perm[cs K + .] the draw's permutation row
//     theta_km   = phi_{perm[k], m} + sum_d x_d xi_{perm[k], m, d}          (d in order from 0; no x: phi alone)
//     W1_k[g][m] = sum_p E1_gp theta_km,p                                    (p in order from 0), W2 likewise with E2
//     c_r(g, h)  = sum_m W1_k[g][m] W2_l[h][m]
// a sum over m of products of two factors that change sign, or are rotated, together: once the labels are aligned the chains pool
// as they are.  The kernels only form the values, V[cs + N (e - r0)] of result rows e = (r G1 + g) G2 + h (diagonal: e = r G1 + g,
// only g = h) of a chunk [r0, r0 + rows), N = C S; mean, sd and quantiles are launch_bands_moments and launch_bands_quantiles
// (kernels_bands.hip) on those rows, as they are.
//
//   k_ccov_project  One workgroup per draw: T[((cs K + k) GP + g) MP + m] = W_k[g][m] of the ALIGNED component k, perm and x folded
//                   in.  g is padded to tiles of 16 (GP), m to the MFMA's four (MP = 4 MB), both with zeros, and the row stride is
//                   MP itself: the 16 rows of a (k, tile) piece are 16 MP consecutive doubles from a 128-byte boundary, so the 64
//                   operand reads of one MFMA below (16 rows x 4 values of m, 32 bytes a row) cover whole 64-byte segments, every
//                   byte fetched is used, and with MB = 1 they are one run of 512 bytes.  Filled once per call for E1 and once
//                   more for E2 where given.
//   k_ccov_mix      Only where the call takes a transform A per draw in place of perm: k_ccov_project fills the
//                   tables of the raw components and this pass mixes them in place, W~_k = sum_c A[k][c] W_c.
//   k_ccov_values   A workgroup of four waves owns one 16 x 16 tile (g-tile, h-tile) of one pair and a block of 16 consecutive
//                   draws, four per wave.  For a draw lane l reads its operands straight from the two tables, A[row l & 15][m =
//                   4 mb + (l >> 4)] of W1_k and B[m][col l & 15] of W2_l (all eight loads of a wave's four draws are issued before
//                   the first MFMA); the tile is MB chained v_mfma_f64_16x16x4_f64 from a zero accumulator (lane l receives
//                   D[row (l >> 4) + 4 reg][col l & 15], the mapping of k_curve_cov).  The 256 x 16 results are staged in LDS at
//                   [entry][draw] with 17 doubles between entries (ds_write_b64 serves 16 consecutive lanes at a time on 16
//                   8-byte banks: an odd stride puts them on 16 different ones) and written draw-fastest: consecutive threads
//                   write consecutive draws of an entry, runs of 128 bytes where the block is full.  A tile that straddles the
//                   chunk or the edge of the surface stores only its live entries; one that has none leaves at once.  diagonal:
//                   tiles (gt, gt) only, both operands from the table of E1, only g = h stored.
//   k_ccov_maxdev   One thread per (pair, draw): dev[r N + cs] = max(dev, |(v - mean) / sd|) over the chunk's entries of pair r,
//                   entries with sd = 0 skipped, a NaN kept (DESIGN.md 7h's rule).  dev persists over the call's chunks; a maximum
//                   is exact and order-free, so the chunking cannot change it.  One-wave workgroups, sixteen loads ahead: a
//                   thread's values lie N doubles apart, consecutive threads' side by side.
//   k_ccov_crit     One workgroup per pair, rows of up to 8192 draws: dev's row sorted in LDS and crit read off it by the quantile
//                   rule of row_stats.hpp, here without an fma, as the restatement and k_fit_sim interpolate (longer rows: the
//                   unchanged k_bands_quantiles_big and k_fit_quantiles).
// A value's bits depend on (draw, pair, g, h) alone: it is the same table entries through the same instructions, whatever the tile
// grouping, the grid, the chunk or the call, and a table entry is one thread's sum in a fixed order.  So the results do not depend
// on the chunk, repeated calls agree, a selected pair equals its rows of the full result, the diagonal is the surface's diagonal,
// and with E2 = E1 pair (l, k) is the transpose of pair (k, l) (the same M products accumulated in the same order), all bit for
// bit.  No atomics, no scratch.
#include "model.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <string>

// the MFMA fuses internally; the tables, the standardised deviations and the interpolation of crit must round as the
// restatement's do
#pragma clang fp contract(off)

#include "row_stats.hpp"

namespace bfmmm {

namespace {

constexpr int CC_NT = 256;
constexpr int CC_MMAX = 16;             // n_eigen: four chained MFMAs
constexpr int CC_DMAX = 8;
constexpr int CC_DB = 16;               // draws of a workgroup of k_ccov_values
constexpr int CC_DW = CC_DB / (CC_NT / 64);      // draws of a wave
constexpr int CC_LD = CC_DB + 1;        // doubles between the entries of the LDS stage
constexpr int CC_MD = 16;               // values a thread of k_ccov_maxdev loads ahead
constexpr int CC_MT = 64;               // its workgroup: one wave, so that a few thousand draws already cover the CUs

struct CcovArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Phi, *c_xi;
  size_t chain_bytes, chain_bytes_cov;
  const int32_t* perm;            // [cs K + k]; null: the identity (the tables of the raw components, for k_ccov_mix)
  const double* mix;              // [(cs K + k) K + c]: the transform of every draw in place of perm, or null
  const int32_t* pairs;           // [2 r], [2 r + 1]
  const double* x;                // the covariate setting, or null
  const double *tab1, *tab2;      // the projection tables of E1 and E2 (tab2 == tab1: E2 = E1)
  size_t ds1, ds2;                // doubles of a draw in either
  int K, P, M, D, DX;             // DX: covariates that enter theta (D where x is given, else 0)
  int C, first_slot, S;
  int G1, G2, GP1, GP2, MP, diagonal;
  long long N;
};

// one workgroup per draw; consecutive threads write consecutive doubles
__global__ __launch_bounds__(CC_NT) void k_ccov_project(CcovArgs a, const double* E, int G, int GP, double* tab) {
  __shared__ double sx[CC_DMAX];
  __shared__ int sp[KMAX];
  const int cs = (int)blockIdx.x, tid = threadIdx.x;
  const int K = a.K, P = a.P, M = a.M, D = a.D, DX = a.DX, MP = a.MP;
  const int q = cs / a.S;
  const size_t t = (size_t)(a.first_slot + cs - q * a.S);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q * a.chain_bytes) + t * K * P * M;
  const double* c_xi = DX > 0 ? ptr_shift(a.c_xi, (size_t)q * a.chain_bytes_cov) + t * K * P * D * M : nullptr;
  if (tid < CC_DMAX) sx[tid] = tid < DX ? a.x[tid] : 0.0;
  if (tid < KMAX) sp[tid] = tid < K ? (a.perm ? a.perm[(size_t)cs * K + tid] : tid) : 0;
  __syncthreads();
  const int perk = GP * MP, total = K * perk;
  double* out = tab + (size_t)cs * total;
  for (int e = tid; e < total; e += CC_NT) {
    const int k = e / perk, r = e - k * perk, g = r / MP, m = r - g * MP;
    double s = 0.0;
    if (g < G && m < M) {
      const int kk = sp[k];
      const double* phi = c_Phi + kk + (size_t)K * P * m;                                     // Phi: [k + K (p + P m)]
      const double* xi = DX > 0 ? c_xi + (size_t)P * D * (m + (size_t)M * kk) : nullptr;      // xi: [p + P (d + D (m + M k))]
      const double* eg = E + (size_t)g * P;
      for (int p = 0; p < P; ++p) {
        double th = phi[(size_t)K * p];
        for (int d = 0; d < DX; ++d) th += sx[d] * xi[p + (size_t)P * d];
        s += eg[p] * th;
      }
    }
    out[e] = s;
  }
}

// The second pass of a call that takes a transform per draw: the table holds W_c of the raw components c, and
// every entry (g, m) becomes W~_k = sum_c A[k][c] W_c, c in order from 0.0, for all k at once, in place: a thread reads the K values
// of its entry before it writes them, and no other thread touches them.  A permutation matrix leaves 1 W + 0 W' + .., the entries
// k_ccov_project writes under that permutation (the padding stays zero).
__global__ __launch_bounds__(CC_NT) void k_ccov_mix(CcovArgs a, int GP, double* tab) {
  __shared__ double sA[KMAX * KMAX];
  const int cs = (int)blockIdx.x, tid = threadIdx.x, K = a.K;
  if (tid < K * K) sA[tid] = a.mix[(size_t)cs * K * K + tid];
  __syncthreads();
  const int perk = GP * a.MP;
  double* t = tab + (size_t)cs * K * perk;
  for (int e = tid; e < perk; e += CC_NT) {
    double w[KMAX];
#pragma unroll
    for (int c = 0; c < KMAX; ++c) w[c] = c < K ? t[(size_t)c * perk + e] : 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < KMAX; ++c)
          if (c < K) s += sA[k * K + c] * w[c];
        t[(size_t)k * perk + e] = s;
      }
  }
}

// tiles [t0, ..) of the call's tiles, numbered (r TG1 + gt) TG2 + ht (diagonal: r TG1 + gt), times nb blocks of draws
template <int MB>
__global__ __launch_bounds__(CC_NT) void k_ccov_values(CcovArgs a, long long t0, int nb, long long r0, long long rows, double* V) {
  __shared__ double sV[256 * CC_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int db = (int)(blockIdx.x % (unsigned)nb);
  const long long tile = t0 + (long long)(blockIdx.x / (unsigned)nb);
  const int TG1 = a.GP1 / 16, TG2 = a.GP2 / 16;
  int gt, ht;
  long long r;
  if (a.diagonal) { r = tile / TG1; gt = (int)(tile - r * TG1); ht = gt; }
  else { const long long rg = tile / TG2; ht = (int)(tile - rg * TG2); r = rg / TG1; gt = (int)(rg - r * TG1); }
  const int G1 = a.G1, G2 = a.G2;
  // the tile's first and last entry: nothing of it in the chunk, nothing to do
  const int gl = min(gt * 16 + 15, G1 - 1), hl = min(ht * 16 + 15, G2 - 1);
  const long long efirst = a.diagonal ? r * G1 + gt * 16 : (r * G1 + gt * 16) * G2 + ht * 16;
  const long long elast = a.diagonal ? r * G1 + gl : (r * G1 + gl) * G2 + hl;
  if (elast < r0 || efirst >= r0 + rows) return;
  const int k = a.pairs[2 * r], l = a.pairs[2 * r + 1];
  const double* tb = a.diagonal ? a.tab1 : a.tab2;
  const size_t dsb = a.diagonal ? a.ds1 : a.ds2;
  const int GPB = a.diagonal ? a.GP1 : a.GP2;
  const size_t offA = ((size_t)k * a.GP1 + gt * 16 + (lane & 15)) * a.MP + (lane >> 4);
  const size_t offB = ((size_t)l * GPB + ht * 16 + (lane & 15)) * a.MP + (lane >> 4);
  const long long cs0 = (long long)db * CC_DB;
  double av[CC_DW][MB], bv[CC_DW][MB];
#pragma unroll
  for (int j = 0; j < CC_DW; ++j) {
    const long long cs = cs0 + wave * CC_DW + j;
    const bool on = cs < a.N;                     // uniform over the wave
    const double* pa = a.tab1 + (size_t)(on ? cs : 0) * a.ds1 + offA;
    const double* pb = tb + (size_t)(on ? cs : 0) * dsb + offB;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      av[j][mb] = pa[4 * mb];
      bv[j][mb] = pb[4 * mb];
    }
  }
#pragma unroll
  for (int j = 0; j < CC_DW; ++j) {
    double4_t d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j][mb], bv[j][mb], d, 0, 0, 0);
    // entry (row (lane >> 4) + 4 reg, col lane & 15) of the tile is 64 reg + lane
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sV[(64 * reg + lane) * CC_LD + wave * CC_DW + j] = d[reg];
  }
  __syncthreads();
  if (a.diagonal) {
    const int gi = tid >> 4, d = tid & 15, g = gt * 16 + gi;
    const long long cs = cs0 + d, e = r * G1 + g - r0;
    if (g < G1 && cs < a.N && e >= 0 && e < rows) V[(size_t)cs + (size_t)a.N * (size_t)e] = sV[(17 * gi) * CC_LD + d];
    return;
  }
  for (int i = tid; i < 256 * CC_DB; i += CC_NT) {
    const int el = i >> 4, d = i & 15, g = gt * 16 + (el >> 4), h = ht * 16 + (el & 15);
    const long long cs = cs0 + d, e = (r * G1 + g) * G2 + h - r0;
    if (g < G1 && h < G2 && cs < a.N && e >= 0 && e < rows) V[(size_t)cs + (size_t)a.N * (size_t)e] = sV[el * CC_LD + d];
  }
}

// pairs [rp0, rp0 + npc) of the call, the ones with entries in the chunk [r0, r0 + rows); cells: entries of a pair
__global__ __launch_bounds__(CC_MT) void k_ccov_maxdev(const double* V, long long N, long long r0, long long rows, long long cells,
                                                       long long rp0, long long npc, const double* mean, const double* sd, double* dev) {
  const long long idx = (long long)blockIdx.x * CC_MT + threadIdx.x;
  if (idx >= npc * N) return;
  const long long pr = idx / N, cs = idx - pr * N, r = rp0 + pr;
  const long long lo = max(r0, r * cells), hi = min(r0 + rows, (r + 1) * cells);
  double mx = dev[(size_t)r * N + cs];
  auto take = [&](double v, long long o) {
    const double sg = sd[o];
    if (sg != 0.0) {
      const double dv = fabs((v - mean[o]) / sg);
      if (dv > mx || dv != dv) mx = dv;
    }
  };
  // a thread's loads are N doubles apart: CC_MD of them are in flight before the first is used
  long long e = lo;
  for (; e + CC_MD <= hi; e += CC_MD) {
    double v[CC_MD];
#pragma unroll
    for (int u = 0; u < CC_MD; ++u) v[u] = V[(size_t)cs + (size_t)N * (size_t)(e + u - r0)];
#pragma unroll
    for (int u = 0; u < CC_MD; ++u) take(v[u], e + u - r0);
  }
  for (; e < hi; ++e) take(V[(size_t)cs + (size_t)N * (size_t)(e - r0)], e - r0);
  dev[(size_t)r * N + cs] = mx;
}

// crit[r] = quantile p of dev[r N + .], N <= CC_SORT_MAX: one workgroup per pair sorts the row in LDS (padded with +inf to a power
// of two) and reads the rule off it
constexpr int CC_SORT_MAX = 8192;
__global__ __launch_bounds__(CC_NT) void k_ccov_crit(const double* dev, int N, double p, double* crit) {
  extern __shared__ double s[];
  const int tid = threadIdx.x;
  const int NP = rs::pow2_ceil(N);
  const double* row = dev + (size_t)blockIdx.x * N;
  for (int e = tid; e < NP; e += CC_NT) s[e] = e < N ? row[e] : INFINITY;
  __syncthreads();
  rs::bitonic_sort<CC_NT>(rs::Plain<double>{s}, 1, NP);
  if (tid == 0) crit[blockIdx.x] = rs::quantile5(rs::Plain<double>{s}, N, p);
}

// what the model and the call's grids fix: MFMAs per draw and tile, covariates in theta, padded grids
struct CcovGeom {
  int MB = 0, DX = 0, GP1 = 0, GP2 = 0;
};

std::string ccov_geom(const Ctx& c, const CcovCall& f, CcovGeom& g) {
  const Dims& d = c.d;
  if (d.K < 1 || d.K > KMAX) return "K outside 1 .. 8";
  if (d.M < 1 || d.M > CC_MMAX) return "n_eigen outside 1 .. 16";
  if (d.D < 0 || d.D > CC_DMAX) return "more than 8 covariates";
  if (d.P < 1) return "P below 1";
  if (f.G1 < 1 || f.G2 < 1 || f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "range outside the chain storage";
  if ((long long)c.nch * f.n_slots > (1LL << 22)) return "more than 2^22 draws";
  g.MB = (d.M + 3) / 4;
  g.DX = f.x ? d.D : 0;
  const long long gp1 = ((long long)f.G1 + 15) / 16 * 16, gp2 = ((long long)f.G2 + 15) / 16 * 16;
  if (KMAX * std::max(gp1, gp2) * 4 * g.MB > 0x7fffffffLL) return "G K n_eigen above 2^31 - 1";
  g.GP1 = (int)gp1; g.GP2 = (int)gp2;
  return "";
}

CcovArgs ccov_args(const Ctx& c, const CcovCall& f, const CcovGeom& g) {
  const Dims& d = c.d;
  CcovArgs a;
  a.c_Phi = c.c_Phi; a.c_xi = g.DX > 0 ? c.c_xi : nullptr;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.perm = f.mix ? nullptr : f.perm; a.mix = f.mix; a.pairs = f.pairs; a.x = g.DX > 0 ? f.x : nullptr;
  a.MP = 4 * g.MB;
  a.tab1 = f.tab1; a.tab2 = f.tab2 ? f.tab2 : f.tab1;
  a.GP1 = g.GP1; a.GP2 = f.tab2 ? g.GP2 : g.GP1;
  a.ds1 = (size_t)d.K * a.GP1 * a.MP; a.ds2 = (size_t)d.K * a.GP2 * a.MP;
  a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.DX = g.DX;
  a.C = c.nch; a.first_slot = f.first_slot; a.S = f.n_slots;
  a.G1 = f.G1; a.G2 = f.G2; a.diagonal = f.diagonal ? 1 : 0;
  a.N = (long long)c.nch * f.n_slots;
  return a;
}

template <int MB>
std::string ccov_launch(const CcovArgs& a, long long t0, long long tiles, long long r0, long long rows, double* V, hipStream_t st) {
  const long long nb = (a.N + CC_DB - 1) / CC_DB;
  if (tiles * nb > 0x7fffffffLL) return "k_ccov_values: too many workgroups in one chunk";
  hipLaunchKernelGGL((k_ccov_values<MB>), dim3((unsigned)(tiles * nb)), dim3(CC_NT), 0, st, a, t0, (int)nb, r0, rows, V);
  if (hipGetLastError() != hipSuccess) return "k_ccov_values: launch failed";
  return "";
}

}  // namespace

std::string ccov_check(const Ctx& c, const CcovCall& f) {
  CcovGeom g;
  return ccov_geom(c, f, g);
}

size_t ccov_table_doubles(const Ctx& c, const CcovCall& f, int which) {
  CcovGeom g;
  if (!ccov_geom(c, f, g).empty()) return 0;
  return (size_t)c.nch * f.n_slots * c.d.K * (which ? g.GP2 : g.GP1) * 4 * g.MB;
}

// the projection tables of the call: f.tab1 of E1 and, where E2 is given, f.tab2 of E2
std::string launch_ccov_project(const Ctx& c, const CcovCall& f, hipStream_t st) {
  CcovGeom g;
  const std::string err = ccov_geom(c, f, g);
  if (!err.empty()) return "k_ccov_project: " + err;
  if (!f.E1 || !f.tab1 || (!f.perm && !f.mix) || (f.E2 && !f.tab2) || (f.x && (!c.covariance_adj || c.d.D < 1))) return "k_ccov_project: bad arguments";
  const CcovArgs a = ccov_args(c, f, g);
  const dim3 grid((unsigned)a.N);
  hipLaunchKernelGGL(k_ccov_project, grid, dim3(CC_NT), 0, st, a, f.E1, f.G1, g.GP1, f.tab1);
  if (f.E2) hipLaunchKernelGGL(k_ccov_project, grid, dim3(CC_NT), 0, st, a, f.E2, f.G2, g.GP2, f.tab2);
  if (f.mix) {
    hipLaunchKernelGGL(k_ccov_mix, grid, dim3(CC_NT), 0, st, a, g.GP1, f.tab1);
    if (f.E2) hipLaunchKernelGGL(k_ccov_mix, grid, dim3(CC_NT), 0, st, a, g.GP2, f.tab2);
  }
  if (hipGetLastError() != hipSuccess) return "k_ccov_project: launch failed";
  return "";
}

// the values of result rows [r0, r0 + rows) of the call: V[cs + N (e - r0)]
std::string launch_ccov_values(const Ctx& c, const CcovCall& f, long long r0, long long rows, double* V, hipStream_t st) {
  CcovGeom g;
  const std::string err = ccov_geom(c, f, g);
  if (!err.empty()) return "k_ccov_values: " + err;
  const long long cells = f.diagonal ? (long long)f.G1 : (long long)f.G1 * f.G2;
  if (rows < 1 || r0 < 0 || r0 + rows > cells * f.n_pairs || !V || !f.tab1 || !f.pairs || (f.diagonal && (f.tab2 || f.G2 != f.G1)))
    return "k_ccov_values: bad arguments";
  const CcovArgs a = ccov_args(c, f, g);
  // the tiles between the one of the chunk's first entry and the one of its last
  const long long TG1 = a.GP1 / 16, TG2 = a.diagonal ? 1 : a.GP2 / 16;
  auto row_tile = [&](long long e) {
    const long long r = e / cells, gg = (e - r * cells) / (f.diagonal ? 1 : f.G2);
    return r * TG1 + gg / 16;
  };
  const long long t0 = row_tile(r0) * TG2, t1 = (row_tile(r0 + rows - 1) + 1) * TG2;
  switch (g.MB) {
    case 1: return ccov_launch<1>(a, t0, t1 - t0, r0, rows, V, st);
    case 2: return ccov_launch<2>(a, t0, t1 - t0, r0, rows, V, st);
    case 3: return ccov_launch<3>(a, t0, t1 - t0, r0, rows, V, st);
    default: return ccov_launch<4>(a, t0, t1 - t0, r0, rows, V, st);
  }
}

// dev[r N + cs] = max(dev, |(v - mean) / sd|) over the entries of pair r in the chunk [r0, r0 + rows), whose values, mean and sd
// are V, mean and sd (entry r0 first)
std::string launch_ccov_maxdev(const CcovCall& f, long long N, long long r0, long long rows, const double* V, const double* mean,
                               const double* sd, double* dev, hipStream_t st) {
  const long long cells = f.diagonal ? (long long)f.G1 : (long long)f.G1 * f.G2;
  if (N < 1 || rows < 1 || r0 < 0 || cells < 1 || r0 + rows > cells * f.n_pairs || !V || !mean || !sd || !dev) return "k_ccov_maxdev: bad arguments";
  const long long rp0 = r0 / cells, npc = (r0 + rows - 1) / cells - rp0 + 1;
  const long long blocks = (npc * N + CC_MT - 1) / CC_MT;
  if (blocks > 0x7fffffffLL) return "k_ccov_maxdev: too many workgroups in one chunk";
  hipLaunchKernelGGL(k_ccov_maxdev, dim3((unsigned)blocks), dim3(CC_MT), 0, st, V, N, r0, rows, cells, rp0, npc, mean, sd, dev);
  if (hipGetLastError() != hipSuccess) return "k_ccov_maxdev: launch failed";
  return "";
}

// crit[r] = quantile p of dev[r N + .] of pairs [0, m), rows of at most ccov_sort_rows() draws (longer ones: launch_bands_quantiles
// into a workspace and launch_fit_quantiles, as the simultaneous bands of DESIGN.md 7h do)
int ccov_sort_rows() { return CC_SORT_MAX; }
std::string launch_ccov_crit(const double* dev, long long N, long long m, double p, double* crit, hipStream_t st) {
  if (!dev || !crit || N < 1 || N > CC_SORT_MAX || m < 1 || m > 0x7fffffffLL) return "k_ccov_crit: bad arguments";
  if (hipFuncSetAttribute((const void*)k_ccov_crit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * CC_SORT_MAX)) != hipSuccess) {
    (void)hipGetLastError();
    return "k_ccov_crit: cannot set the LDS size";
  }
  hipLaunchKernelGGL(k_ccov_crit, dim3((unsigned)m), dim3(CC_NT), sizeof(double) * (size_t)rs::pow2_ceil((int)N), st, dev, (int)N, p, crit);
  if (hipGetLastError() != hipSuccess) return "k_ccov_crit: launch failed";
  return "";
}

}  // namespace bfmmm
