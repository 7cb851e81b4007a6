// Pooled per-curve fitted functions of chain slots and their credible bands: for every chain q, slot t, curve i
// and row E_g of an evaluation basis (G x P, row-major)
//     mean_i(g) = E_g . c_i,                         c_i  = sum_k Z_ik (nu_k + sum_d x_id eta_kd),
//     fit_i(g)  = E_g . (c_i + sum_m chi_im V_im),   V_im = sum_k Z_ik (phi_km + sum_d x_id xi_kmd)   (xi: covariance-adjusted only).
// Both are sums over k (label-invariant); fit is a product of chi_im and V_im (sign-invariant): they pool over chains as
// they are.  A row is one (curve, grid point): its C S values over chains and slots, chain-major and draw-fastest.
//
//   k_fit_project   T[(g NJ + j) CS + cs] = E_g . theta_j of draw cs = q S + (t - first_slot), for the NJ = K M1 (1 + D)
//                   directions j = (k M1 + mt)(1 + D) + dd of a draw (mt = 0: nu_k, mt > 0: phi_k,mt-1; dd = 0 the direction
//                   itself, dd > 0 its covariate part eta / xi; M1 = 1 for `mean`, M + 1 for `fit`).  Shared by all curves:
//                   a value is then K M1 (1 + D) multiply-adds, not P K M1 (1 + D).  Draw-fastest, so that the lanes of the
//                   kernels below (one draw each) read it coalesced.
//   k_fit_rows      C S <= 8192.  A workgroup takes one curve and a tile of GT grid points: lane cs reads Z_i. and chi_i. of
//                   its draw once, forms the draw's value of each of the tile's rows into LDS (fit_value), then mean and sd
//                   of every row (row_mean_sd), one bitonic sort of all the tile's rows at once (padded with +inf) and the
//                   quantiles (quantile5).  (2 + nq) numbers per row leave.
//   k_fit_values    the same fit_value into a workspace out[((r G + g) CS) + cs]: the long rows (k_bands_quantiles_big and
//                   k_bands_moments reduce them) and the host copy of bfmmm_chain_curve_fit.
//   k_fit_quantiles quantile5 read off rows that are already sorted (k_bands_quantiles_big leaves them so in its workspace):
//                   kernels_bands.hip is compiled with contraction on, this file is not, and both tiers must round alike.
//   k_fit_sim       simultaneous band of a curve: one workgroup owns one result row and never stores a value.
//                   Three passes form every value again with the same fit_value: per-lane sums of tiles of FIT_SIM_GT grid
//                   points in registers and the block tree -> mean(g) in LDS; the squares likewise -> sd(g); then per draw
//                   C(cs) = max_g |(v - mean(g)) / sd(g)| over the grid points with sd != 0.  C S <= 8192: C is sorted in LDS
//                   and crit, lower, upper leave; longer rows: C goes to a workspace row that k_bands_quantiles_big sorts,
//                   k_fit_quantiles reads crit off it and k_fit_sim_band writes the band ends.
// fp64, every sum in a fixed order that depends on (curve, grid point, chain, slot) only, no atomics, no scratch: the bits
// do not depend on the chunk, the tile or the grid.
#include "model.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <cmath>
#include <string>

// the interpolation of a quantile must round as the restatement does
#pragma clang fp contract(off)

#include "row_stats.hpp"

namespace bfmmm {

namespace {

constexpr int FIT_NT = 256;
constexpr int FIT_MMAX = 16;                   // n_eigen supported by the unrolled value
constexpr int FIT_GT_MAX = 16;                 // grid points per tile (FIT_GT_MAX x 16 quantile lanes = one workgroup)
constexpr int FIT_LDS_ROWS = 8192;             // C S of the last row sorted in LDS
constexpr size_t FIT_LDS_SOFT = 64 * 1024;     // a tile's rows: two workgroups per CU

struct FitArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Z, *c_chi, *c_nu, *c_Phi, *c_eta, *c_xi;
  const double *X, *E;
  const int* curves;                           // the curve of result row r, or null: curve r
  double* tab;
  size_t chain_bytes, chain_bytes_cov;
  int n, K, P, M, D, cadj;
  int C, first_slot, S, CS, G, NJ, M1;
};

template <int WHICH>
__global__ __launch_bounds__(FIT_NT) void k_fit_project(FitArgs a) {
  const int tid = threadIdx.x, dd8 = tid & 7;
  const int cs = (int)blockIdx.x * 8 + dd8;                    // eight consecutive draws per workgroup: 64-byte stores
  if (cs >= a.CS) return;
  const int K = a.K, P = a.P, M = a.M, D = a.D, D1 = D + 1, M1 = a.M1;
  const int q = cs / a.S;
  const size_t t = (size_t)(a.first_slot + cs - q * a.S);
  const double* c_nu = ptr_shift(a.c_nu, (size_t)q * a.chain_bytes) + t * K * P;
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q * a.chain_bytes) + t * K * P * M;
  const double* c_eta = D > 0 ? ptr_shift(a.c_eta, (size_t)q * a.chain_bytes_cov) + t * P * D * K : nullptr;
  const double* c_xi = D > 0 ? ptr_shift(a.c_xi, (size_t)q * a.chain_bytes_cov) + t * K * P * D * M : nullptr;
  for (int e = tid >> 3; e < a.G * a.NJ; e += FIT_NT / 8) {
    const int g = e / a.NJ, j = e - g * a.NJ;
    const int k = j / (M1 * D1), r = j - k * M1 * D1, mt = r / D1, dd = r - mt * D1;
    const double* th = nullptr;                                // theta_j[p] = th[p * st]
    int st = 1;
    if (dd == 0) {
      if (mt == 0) { th = c_nu + k; st = K; }                  // nu: [k + K p]
      else if (WHICH) { th = c_Phi + k + (size_t)K * P * (mt - 1); st = K; }       // Phi: [k + K (p + P m)]
    } else {
      if (mt == 0) th = c_eta + (size_t)P * ((dd - 1) + D * k);                    // eta: [p + P (d + D k)]
      else if (WHICH && a.cadj) th = c_xi + (size_t)P * ((dd - 1) + D * ((mt - 1) + M * k));   // xi: [p + P (d + D (m + M k))]
    }
    double s = 0.0;
    if (th) {
      const double* eg = a.E + (size_t)g * P;
      for (int p = 0; p < P; ++p) s += eg[p] * th[(size_t)p * st];
    }
    a.tab[(size_t)e * a.CS + cs] = s;
  }
}

// the value of one (curve, grid point, draw): tg = the draw's entry of direction 0 of the grid point, directions CS apart
template <int WHICH>
__device__ __forceinline__ double fit_value(const double* __restrict__ tg, size_t CS, const double (&z)[KMAX],
                                            const double (&ch)[FIT_MMAX], const double* sx, int K, int M, int D, int cadj) {
  const int M1 = WHICH ? M + 1 : 1, D1 = D + 1;
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const double* tk = tg + (size_t)(k * M1) * D1 * CS;
      double c = tk[0];
      for (int d = 0; d < D; ++d) c += sx[d] * tk[(size_t)(1 + d) * CS];
      if (WHICH) {
#pragma unroll
        for (int m = 0; m < FIT_MMAX; ++m) {
          if (m < M) {
            const double* tm = tk + (size_t)(m + 1) * D1 * CS;
            double b = tm[0];
            if (cadj)
              for (int d = 0; d < D; ++d) b += sx[d] * tm[(size_t)(1 + d) * CS];
            c += ch[m] * b;
          }
        }
      }
      v += z[k] * c;
    }
  }
  return v;
}

// Z_i. and chi_i. of draw cs (chi: fit only), zero beyond K and M
template <int WHICH>
__device__ __forceinline__ void fit_draw(const FitArgs& a, int i, int cs, double (&z)[KMAX], double (&ch)[FIT_MMAX]) {
  const int K = a.K, M = a.M, n = a.n;
  const int q = cs / a.S;
  const size_t t = (size_t)(a.first_slot + cs - q * a.S);
  const double* zq = ptr_shift(a.c_Z, (size_t)q * a.chain_bytes) + t * n * K + i;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) z[k] = k < K ? zq[(size_t)n * k] : 0.0;
  if (WHICH) {
    const double* cq = ptr_shift(a.c_chi, (size_t)q * a.chain_bytes) + t * n * M + i;
#pragma unroll
    for (int m = 0; m < FIT_MMAX; ++m) ch[m] = m < M ? cq[(size_t)n * m] : 0.0;
  } else {
#pragma unroll
    for (int m = 0; m < FIT_MMAX; ++m) ch[m] = 0.0;
  }
}

// every draw's value of grid points [g0, g0 + gn) of curve i, lane cs: Z_i. and chi_i. of a draw are read once
template <int WHICH, typename Sink>
__device__ __forceinline__ void fit_form(const FitArgs& a, int i, int g0, int gn, const double* sx, int tid, Sink sink) {
  for (int cs = tid; cs < a.CS; cs += FIT_NT) {
    double z[KMAX], ch[FIT_MMAX];
    fit_draw<WHICH>(a, i, cs, z, ch);
    for (int gl = 0; gl < gn; ++gl)
      sink(gl, cs, fit_value<WHICH>(a.tab + (size_t)(g0 + gl) * a.NJ * a.CS + cs, (size_t)a.CS, z, ch, sx, a.K, a.M, a.D, a.cadj));
  }
}

struct FitRowArgs {
  int r0, GT, NP, tiles, nq;                                   // first result row of the chunk, tile, padded row, tiles per curve
  const double* probs;
  double *mean, *sd, *quant;                                   // of the chunk: [r G + g], [(r G + g) nq + q]
};

template <int WHICH>
__global__ __launch_bounds__(FIT_NT) void k_fit_rows(FitArgs a, FitRowArgs w) {
  extern __shared__ __attribute__((aligned(16))) double s[];   // GT rows of NP
  __shared__ double red[FIT_NT];
  __shared__ double sx[8];
  const int tid = threadIdx.x;
  const int r = (int)(blockIdx.x / (unsigned)w.tiles), tile = (int)(blockIdx.x - (unsigned)r * w.tiles);
  const int g0 = tile * w.GT, gn = min(w.GT, a.G - g0);
  const int i = a.curves ? a.curves[w.r0 + r] : w.r0 + r;
  const int NP = w.NP, T = a.CS;
  if (tid < a.D) sx[tid] = a.X[i + (size_t)a.n * tid];
  for (int e = tid; e < gn * NP; e += FIT_NT)
    if ((e & (NP - 1)) >= T) s[e] = INFINITY;
  __syncthreads();
  fit_form<WHICH>(a, i, g0, gn, sx, tid, [&](int gl, int cs, double v) { s[gl * NP + cs] = v; });
  __syncthreads();
  // mean and sd of every row before it is sorted
  for (int gl = 0; gl < gn; ++gl) {
    double m, sdv;
    rs::row_mean_sd<FIT_NT>(s + gl * NP, T, red, m, sdv);
    if (tid == 0) {
      const size_t o = (size_t)r * a.G + g0 + gl;
      w.mean[o] = m;
      w.sd[o] = sdv;
    }
  }
  rs::bitonic_sort<FIT_NT>(rs::Plain<double>{s}, gn, NP);
  if (tid < gn * w.nq) {
    const int gl = tid / w.nq, qi = tid - gl * w.nq;
    w.quant[((size_t)r * a.G + g0 + gl) * w.nq + qi] = rs::quantile5(rs::Plain<double>{s + gl * NP}, T, w.probs[qi]);
  }
}

// out[((r G + g) CS) + cs] of the chunk's result rows r0 ..; GT grid points per workgroup
template <int WHICH>
__global__ __launch_bounds__(FIT_NT) void k_fit_values(FitArgs a, int r0, int GT, int tiles, double* out) {
  __shared__ double sx[8];
  const int tid = threadIdx.x;
  const int r = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)r * tiles);
  const int g0 = tile * GT, gn = min(GT, a.G - g0);
  const int i = a.curves ? a.curves[r0 + r] : r0 + r;
  if (tid < a.D) sx[tid] = a.X[i + (size_t)a.n * tid];
  __syncthreads();
  double* o = out + ((size_t)r * a.G + g0) * a.CS;
  const size_t CS = (size_t)a.CS;
  fit_form<WHICH>(a, i, g0, gn, sx, tid, [&](int gl, int cs, double v) { o[(size_t)gl * CS + cs] = v; });
}

// quant[col nq + q] from sorted rows W[col NP + .] of T values
__global__ __launch_bounds__(FIT_NT) void k_fit_quantiles(const double* W, int NP, int T, long long ncol, const double* probs, int nq,
                                                          double* quant) {
  const long long e = (long long)blockIdx.x * FIT_NT + threadIdx.x;
  if (e >= ncol * nq) return;
  const long long col = e / nq;
  quant[e] = rs::quantile5(rs::Plain<const double>{W + (size_t)col * NP}, T, probs[(int)(e - col * nq)]);
}

// ---- simultaneous bands ----
constexpr int FIT_SIM_GT = 8;                  // grid points whose per-lane sums are kept in registers at once
constexpr int FIT_SIM_GMAX = 4096;             // 16 G bytes of mean and sd beside the 64 KiB sort row and red[]: 130 of 160 KiB

// The loops over grid points below are long and regular: left alone the compiler carries the address of every direction of a
// value from one grid point to the next in a register pair of its own (8 x 17 pairs for `fit`) and spills.  Hiding the grid
// point's base address from it makes the directions' addresses base + uniform offset again, as in k_fit_values.
#define FIT_SIM_OPAQUE(ptr) asm volatile("" : "+v"(ptr))

struct FitSimArgs {
  int r0, NP, fused;                           // first result row of the chunk; padded sort row, 0: C goes to cw; squares by fma
  double p;                                    // 1 - alpha
  double *mean, *sd, *crit, *lower, *upper;    // of the chunk: [r G + g], crit [r]
  double* cw;                                  // long rows: [r CS + cs]
};

template <int WHICH>
__global__ __launch_bounds__(FIT_NT) void k_fit_sim(FitArgs a, FitSimArgs w) {
  extern __shared__ __attribute__((aligned(16))) double s[];   // mean[G], sd[G], the sort row of NP
  __shared__ double red[FIT_NT];
  __shared__ double sx[8];
  const int tid = threadIdx.x, r = (int)blockIdx.x;
  const int i = a.curves ? a.curves[w.r0 + r] : w.r0 + r;
  const int G = a.G, T = a.CS, NP = w.NP;
  const size_t CS = (size_t)a.CS, gstride = (size_t)a.NJ * CS;
  double *s_mean = s, *s_sd = s + G, *row = s + 2 * (size_t)G;
  if (tid < a.D) sx[tid] = a.X[i + (size_t)a.n * tid];
  for (int e = T + tid; e < NP; e += FIT_NT) row[e] = INFINITY;
  __syncthreads();
  // passes 0 and 1: sum of v, then of (v - mean)^2, per grid point: the lane's draws in order, then the block tree
  for (int pass = 0; pass < 2; ++pass)
    for (int g0 = 0; g0 < G; g0 += FIT_SIM_GT) {
      const int gn = min(FIT_SIM_GT, G - g0);
      // one copy of fit_value: gl is uniform, so picking its accumulator is a uniform test per register pair, not an index
      double acc[FIT_SIM_GT];
#pragma unroll
      for (int j = 0; j < FIT_SIM_GT; ++j) acc[j] = 0.0;
      // k_bands_moments, which gives the long rows' sd in bfmmm_chain_curve_bands, is compiled with contraction on
      const bool fz = pass && w.fused;
      for (int cs = tid; cs < T; cs += FIT_NT) {
        double z[KMAX], ch[FIT_MMAX];
        fit_draw<WHICH>(a, i, cs, z, ch);
#pragma nounroll
        for (int gl = 0; gl < gn; ++gl) {
          const double* tg = a.tab + (size_t)(g0 + gl) * gstride + cs;
          FIT_SIM_OPAQUE(tg);
          const double v = fit_value<WHICH>(tg, CS, z, ch, sx, a.K, a.M, a.D, a.cadj);
          const double dlt = pass ? v - s_mean[g0 + gl] : 0.0;
          const double term = pass ? dlt * dlt : v;
#pragma unroll
          for (int j = 0; j < FIT_SIM_GT; ++j)
            if (j == gl) acc[j] = fz ? __builtin_fma(dlt, dlt, acc[j]) : acc[j] + term;
        }
      }
#pragma unroll
      for (int gl = 0; gl < FIT_SIM_GT; ++gl)
        if (gl < gn) {
          const double tot = rs::block_tree<FIT_NT>(acc[gl], red, rs::OpSum());
          if (tid == 0) {
            if (!pass) s_mean[g0 + gl] = tot / (double)T;
            else s_sd[g0 + gl] = sqrt(tot / (double)(T - 1));
          }
          __syncthreads();
        }
    }
  // pass 2: C(cs) = max over the grid points with sd != 0 of |(v - mean) / sd|, from 0; a NaN (one draw: sd is NaN) stays
  for (int cs = tid; cs < T; cs += FIT_NT) {
    double z[KMAX], ch[FIT_MMAX];
    fit_draw<WHICH>(a, i, cs, z, ch);
    double mx = 0.0;
#pragma nounroll
    for (int g = 0; g < G; ++g) {
      const double* tg = a.tab + (size_t)g * gstride + cs;
      FIT_SIM_OPAQUE(tg);
      const double v = fit_value<WHICH>(tg, CS, z, ch, sx, a.K, a.M, a.D, a.cadj);
      const double sg = s_sd[g];
      if (sg != 0.0) {
        const double dv = fabs((v - s_mean[g]) / sg);
        if (dv > mx || dv != dv) mx = dv;
      }
    }
    if (NP) row[cs] = mx;
    else w.cw[(size_t)r * CS + cs] = mx;
  }
  const size_t o = (size_t)r * G;
  if (!NP) {                                   // long rows: the sort, crit and the band ends follow in launches of their own
    for (int g = tid; g < G; g += FIT_NT) { w.mean[o + g] = s_mean[g]; w.sd[o + g] = s_sd[g]; }
    return;
  }
  __syncthreads();
  rs::bitonic_sort<FIT_NT>(rs::Plain<double>{row}, 1, NP);
  const double crit = rs::quantile5(rs::Plain<double>{row}, T, w.p);
  if (tid == 0) w.crit[r] = crit;
  for (int g = tid; g < G; g += FIT_NT) {
    const double m = s_mean[g], sg = s_sd[g];
    w.mean[o + g] = m;
    w.sd[o + g] = sg;
    w.lower[o + g] = m - crit * sg;
    w.upper[o + g] = m + crit * sg;
  }
}

// the band ends of long rows, once crit[r] has been read off the sorted workspace: e = r G + g
__global__ __launch_bounds__(FIT_NT) void k_fit_sim_band(const double* mean, const double* sd, const double* crit, int G, long long tot,
                                                         double* lower, double* upper) {
  const long long e = (long long)blockIdx.x * FIT_NT + threadIdx.x;
  if (e >= tot) return;
  const double c = crit[e / G], m = mean[e], sg = sd[e];
  lower[e] = m - c * sg;
  upper[e] = m + c * sg;
}

FitArgs fit_args(const Ctx& c, const FitCall& f) {
  const Dims& d = c.d;
  FitArgs a;
  a.c_Z = c.c_Z; a.c_chi = c.c_chi; a.c_nu = c.c_nu; a.c_Phi = c.c_Phi;
  a.c_eta = d.D > 0 ? c.c_eta : nullptr; a.c_xi = d.D > 0 ? c.c_xi : nullptr;
  a.X = d.D > 0 ? c.X : nullptr; a.E = f.E; a.curves = f.curves; a.tab = f.tab;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.n = d.n; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.cadj = (d.D > 0 && c.covariance_adj) ? 1 : 0;
  a.C = c.nch; a.first_slot = f.first_slot; a.S = f.n_slots; a.CS = c.nch * f.n_slots; a.G = f.G;
  a.M1 = f.which ? d.M + 1 : 1;
  a.NJ = d.K * a.M1 * (1 + d.D);
  return a;
}

}  // namespace

long long fit_directions(const Dims& d, int which) { return (long long)d.K * (which ? d.M + 1 : 1) * (1 + d.D); }
int fit_lds_rows() { return FIT_LDS_ROWS; }
int fit_sim_gmax() { return FIT_SIM_GMAX; }

std::string fit_check(const Ctx& c, const FitCall& f) {
  const Dims& d = c.d;
  if (d.K < 1 || d.K > KMAX) return "K outside 1 .. 8";
  if (d.M < 1 || d.M > FIT_MMAX) return "n_eigen outside 1 .. 16";
  if (d.D < 0 || d.D > 8) return "more than 8 covariates";
  if (d.P < 1) return "P below 1";
  if (f.which != 0 && f.which != 1) return "'which' outside {0, 1}";
  if (f.G < 1 || f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "range outside the chain storage";
  if ((long long)c.nch * f.n_slots > (1LL << 22)) return "more than 2^22 draws per row";
  if ((long long)f.G * fit_directions(d, f.which) > 0x7fffffffLL) return "G K (n_eigen + 1) (1 + D) above 2^31 - 1";
  return "";
}

// the projection table of the call: f.tab[(g NJ + j) CS + cs]
std::string launch_fit_project(const Ctx& c, const FitCall& f, hipStream_t st) {
  const std::string err = fit_check(c, f);
  if (!err.empty()) return "k_fit_project: " + err;
  const FitArgs a = fit_args(c, f);
  const dim3 grid((unsigned)((a.CS + 7) / 8));
  if (f.which) hipLaunchKernelGGL(k_fit_project<1>, grid, dim3(FIT_NT), 0, st, a);
  else hipLaunchKernelGGL(k_fit_project<0>, grid, dim3(FIT_NT), 0, st, a);
  if (hipGetLastError() != hipSuccess) return "k_fit_project: launch failed";
  return "";
}

// mean, sd and quantiles of result rows [r0, r0 + rows) x G, rows of C S <= 8192 draws, into the chunk's outputs
std::string launch_fit_rows(const Ctx& c, const FitCall& f, int r0, int rows, const double* probs, int nq, double* mean, double* sd,
                            double* quant, hipStream_t st) {
  const std::string err = fit_check(c, f);
  if (!err.empty()) return "k_fit_rows: " + err;
  const FitArgs a = fit_args(c, f);
  if (a.CS > FIT_LDS_ROWS) return "k_fit_rows: rows above 8192 draws";
  if (nq < 1 || nq > 16 || rows < 1) return "k_fit_rows: bad arguments";
  FitRowArgs w;
  w.NP = rs::pow2_ceil(a.CS);
  const int fit = (int)(FIT_LDS_SOFT / (sizeof(double) * (size_t)w.NP));
  w.GT = std::max(1, std::min(std::min(fit, FIT_GT_MAX), a.G));
  w.tiles = (a.G + w.GT - 1) / w.GT;
  if ((long long)rows * w.tiles > 0x7fffffffLL) return "k_fit_rows: too many workgroups in one chunk";
  w.r0 = r0; w.nq = nq; w.probs = probs; w.mean = mean; w.sd = sd; w.quant = quant;
  const size_t lds = sizeof(double) * (size_t)w.GT * w.NP;
  const void* fn = f.which ? (const void*)k_fit_rows<1> : (const void*)k_fit_rows<0>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIT_LDS_SOFT) != hipSuccess) {
    (void)hipGetLastError();
    return "k_fit_rows: cannot set the LDS size";
  }
  const dim3 grid((unsigned)((long long)rows * w.tiles));
  if (f.which) hipLaunchKernelGGL(k_fit_rows<1>, grid, dim3(FIT_NT), lds, st, a, w);
  else hipLaunchKernelGGL(k_fit_rows<0>, grid, dim3(FIT_NT), lds, st, a, w);
  if (hipGetLastError() != hipSuccess) return "k_fit_rows: launch failed";
  return "";
}

// the values of result rows [r0, r0 + rows) x G into out (rows G CS doubles)
std::string launch_fit_values(const Ctx& c, const FitCall& f, int r0, int rows, double* out, hipStream_t st) {
  const std::string err = fit_check(c, f);
  if (!err.empty()) return "k_fit_values: " + err;
  const FitArgs a = fit_args(c, f);
  if (rows < 1) return "k_fit_values: bad arguments";
  const int GT = std::min(FIT_GT_MAX, a.G), tiles = (a.G + GT - 1) / GT;
  if ((long long)rows * tiles > 0x7fffffffLL) return "k_fit_values: too many workgroups in one chunk";
  const dim3 grid((unsigned)((long long)rows * tiles));
  if (f.which) hipLaunchKernelGGL(k_fit_values<1>, grid, dim3(FIT_NT), 0, st, a, r0, GT, tiles, out);
  else hipLaunchKernelGGL(k_fit_values<0>, grid, dim3(FIT_NT), 0, st, a, r0, GT, tiles, out);
  if (hipGetLastError() != hipSuccess) return "k_fit_values: launch failed";
  return "";
}

// Simultaneous bands of result rows [r0, r0 + rows): mean, sd [r G + g] of the chunk always; rows of C S <= 8192 draws also crit [r],
// lower, upper [r G + g] (cw unused); longer rows C [r CS + cs] into cw instead, for the sort that launch_fit_sim_band follows
std::string launch_fit_sim(const Ctx& c, const FitCall& f, int r0, int rows, double p, double* mean, double* sd, double* crit, double* lower,
                           double* upper, double* cw, hipStream_t st) {
  const std::string err = fit_check(c, f);
  if (!err.empty()) return "k_fit_sim: " + err;
  const FitArgs a = fit_args(c, f);
  if (a.G > FIT_SIM_GMAX) return "k_fit_sim: G above 4096";
  if (rows < 1 || !mean || !sd || !crit || !lower || !upper) return "k_fit_sim: bad arguments";
  const bool lds_row = a.CS <= FIT_LDS_ROWS;
  if (!lds_row && !cw) return "k_fit_sim: no workspace";
  FitSimArgs w;
  w.r0 = r0; w.NP = lds_row ? rs::pow2_ceil(a.CS) : 0; w.fused = lds_row ? 0 : 1; w.p = p;
  w.mean = mean; w.sd = sd; w.crit = crit; w.lower = lower; w.upper = upper; w.cw = cw;
  const size_t lds = sizeof(double) * (2 * (size_t)a.G + (size_t)w.NP);
  const void* fn = f.which ? (const void*)k_fit_sim<1> : (const void*)k_fit_sim<0>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * (2 * FIT_SIM_GMAX + FIT_LDS_ROWS))) != hipSuccess) {
    (void)hipGetLastError();
    return "k_fit_sim: cannot set the LDS size";
  }
  if (f.which) hipLaunchKernelGGL(k_fit_sim<1>, dim3((unsigned)rows), dim3(FIT_NT), lds, st, a, w);
  else hipLaunchKernelGGL(k_fit_sim<0>, dim3((unsigned)rows), dim3(FIT_NT), lds, st, a, w);
  if (hipGetLastError() != hipSuccess) return "k_fit_sim: launch failed";
  return "";
}

std::string launch_fit_sim_band(const double* mean, const double* sd, const double* crit, int G, int rows, double* lower, double* upper,
                                hipStream_t st) {
  const long long tot = (long long)rows * G;
  if (tot < 1 || (tot + FIT_NT - 1) / FIT_NT > 0x7fffffffLL) return "k_fit_sim_band: bad arguments";
  hipLaunchKernelGGL(k_fit_sim_band, dim3((unsigned)((tot + FIT_NT - 1) / FIT_NT)), dim3(FIT_NT), 0, st, mean, sd, crit, G, tot, lower, upper);
  if (hipGetLastError() != hipSuccess) return "k_fit_sim_band: launch failed";
  return "";
}

std::string launch_fit_quantiles(const double* W, int NP, int T, long long ncol, const double* probs, int nq, double* quant, hipStream_t st) {
  const long long tot = ncol * nq;
  if (tot < 1 || (tot + FIT_NT - 1) / FIT_NT > 0x7fffffffLL) return "k_fit_quantiles: bad arguments";
  hipLaunchKernelGGL(k_fit_quantiles, dim3((unsigned)((tot + FIT_NT - 1) / FIT_NT)), dim3(FIT_NT), 0, st, W, NP, T, ncol, probs, nq, quant);
  if (hipGetLastError() != hipSuccess) return "k_fit_quantiles: launch failed";
  return "";
}

}  // namespace bfmmm
