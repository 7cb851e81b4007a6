// Cluster eigenvalues and eigenfunctions with the labels aligned, from chain slots: for every chain q, slot t and
// aligned component k, with cs = q S + (t - first_slot), perm[cs K + .] the draw's permutation row, a grid basis E (G x P,
// row-major), weights w_g >= 0 (null: 1) and reference functions ref (K x J x G; null: the largest-entry rule)
//     theta_km = phi_{perm[k], m} + sum_d x_d xi_{perm[k], m, d}             (d in order from 0; no x: phi alone; k_ccov_project's)
//     Q        = E' diag(w) E,   Q[p][p2] = sum_g (E_gp w_g) E_gp2           (g in order from 0)
//     R_kj     = E' diag(w) ref_kj,   R_kj[p] = sum_g (E_gp w_g) ref_kj[g]
//     S_k      = Theta_k' Q Theta_k = V diag(lambda) V'                      (M x M; lambda descending, ties in index order, >= 0)
//     total_k  = sum_i S_k[i][i]                                              (i in order from 0, before the rotations)
//     pve_kj   = lambda_kj / total_k                                          (0 where total_k == 0)
//     b_kj     = Theta_k v_j / sqrt(lambda_kj)                                (0 where lambda_kj <= M 2^-53 lambda_k1)
//     psi_kj(g)= sgn_kj E_g . b_kj,   sgn_kj = +1 if b_kj . R_kj >= 0 else -1
//                (ref null: the sign of the E_g . b_kj of largest sqrt(w_g) |E_g . b_kj|, lowest g first on ties)
// lambda_kj and psi_kj are the eigenpairs of the w-discretised covariance operator of cluster k: they do not change when the
// columns of Theta_k change sign or are rotated jointly, so once the labels are aligned the chains pool.
//
//   k_ceig_gram    One thread per entry of Q and of R, g in order from 0.  Once per call.
//   k_ceig_solve   One wave per problem (draw, component), NW problems per workgroup; Q (row stride P | 1) is staged once per
//                  workgroup and shared.  A wave keeps Theta_k (P x M, row stride TS = 4 MB + 1, MB = ceil(M / 4), zero-padded),
//                  S_k, V (row stride TS) and a P x 4 stage in LDS.  Lane p forms row p of Y = Q Theta_k in registers (p2 in
//                  order from 0: one read of Q, 4 MB broadcast reads of Theta per step); four columns of Y at a time go through
//                  the stage and lane (i, jj) sums S[i][j] = sum_p Theta[p][i] Y[p][j], p in order from 0.  That is the
//                  plain form; the MFMA form (MF) pads Theta to 16 columns and Q and Theta with zeros to whole tiles, forms a
//                  16-row tile of Y at a time by ceil(P / 4) chained v_mfma_f64_16x16x4_f64, stages it and takes it into S by four
//                  more, with the operand mapping of k_curve_cov.  The launcher takes the form that measured faster (DESIGN.md
//                  7l; bfmmm_set_cluster_eig_form overrides).  The lower triangle is then copied from the upper, so that only the upper one is ever read from the
//                  sums.  Cyclic Jacobi in round-robin order: with n = M rounded up to even, round r of the n - 1 rounds of a
//                  sweep pairs (r, n - 1) and ((r + i) mod (n - 1), (r - i) mod (n - 1)), i = 1 .. n / 2 - 1; a pair with the
//                  index M (odd M) is a bye.  The pairs of a round are disjoint: lane i computes the rotation of pair i from
//                  s_pp, s_qq and the upper s_pq, all lanes apply the round's rotations to the columns of S and V, then to the
//                  rows of S, and the pair's lane writes s_pp - t s_pq, s_qq + t s_pq and the two exact zeros.  A pair is
//                  skipped when |s_pq| <= u max(sqrt(|s_pp s_qq|), u ||S||_F of the start), u = 2^-53; the iteration stops
//                  after a sweep without a rotation, or after 40 sweeps with status bit 0x100 set (the call then fails naming
//                  the draw and the component).  Then the diagonal is ranked, lane p forms its entries of the J leading b in
//                  registers and writes them over its own row of Theta, lane j takes the sign of b_j, and the signed b go out
//                  p-fastest.  lambda, pve and total are written draw-fastest, as rows for launch_bands_moments,
//                  launch_bands_quantiles and diag_launch.
//   k_ceig_values  Row e = (k J + j) G + g of a chunk [r0, r0 + rows): V[cs + N (e - r0)] = E_g . b_kj(cs), p in order from 0.
//                  A workgroup stages the b of 64 consecutive draws (row stride P | 1) and 16 rows of E in LDS; lane d of a
//                  wave owns draw d and the waves share the 16 rows, so consecutive lanes write consecutive draws.
// A value's bits depend on (draw, component) alone (k_ceig_values: and on j, g): one wave's or one thread's sums in a fixed
// order, whatever the grouping into workgroups, the grid, the chunk or the call.  No atomics, no scratch.
#include "model.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <string>

// the restatement rounds every product and every sum once
#pragma clang fp contract(off)

namespace bfmmm {

namespace {

constexpr int CE_MMAX = 16;
constexpr int CE_PMAX = 64;
constexpr int CE_DMAX = 8;
constexpr int CE_CAP = 40;                 // sweeps
constexpr int CE_YS = 5;                   // doubles between the rows of the P x 4 stage
constexpr int CE_DB = 64;                  // draws of a workgroup of k_ceig_values
constexpr int CE_GT = 16;                  // rows of E of a workgroup of k_ceig_values
constexpr int CE_NT = 256;
constexpr size_t CE_LDS_MAX = 65536;       // dynamic LDS a workgroup of k_ceig_solve may take
constexpr double CE_U = 1.1102230246251565e-16;      // 2^-53

struct CeigArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Phi, *c_xi;
  size_t chain_bytes, chain_bytes_cov;
  const int32_t* perm;            // [cs K + k]
  const double *x, *E, *w, *Q, *R;
  double *lam, *pve, *tot, *b;
  int32_t* status;
  int K, P, M, D, DX, S, first_slot, G, J;
  long long N;
};

__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// pair i of round r among n (even) indices, p < q
__device__ __forceinline__ void rr_pair(int r, int i, int n, int& p, int& q) {
  const int a = i == 0 ? r : (r + i) % (n - 1);
  const int b = i == 0 ? n - 1 : (r - i + (n - 1)) % (n - 1);
  p = min(a, b); q = max(a, b);
}

// entries [0, P P) of Q, then [0, KJ P) of R
__global__ __launch_bounds__(CE_NT) void k_ceig_gram(const double* E, const double* w, const double* ref, int G, int P, int KJ, double* Q,
                                                     double* R) {
  const long long idx = (long long)blockIdx.x * CE_NT + threadIdx.x;
  const long long nq = (long long)P * P;
  if (idx >= nq + (long long)KJ * P) return;
  double s = 0.0;
  if (idx < nq) {
    const int p = (int)(idx / P), p2 = (int)(idx - (long long)p * P);
    for (int g = 0; g < G; ++g) {
      const double a = w ? E[(size_t)g * P + p] * w[g] : E[(size_t)g * P + p];
      s += a * E[(size_t)g * P + p2];
    }
    Q[idx] = s;
  } else {
    const long long o = idx - nq;
    const int kj = (int)(o / P), p = (int)(o - (long long)kj * P);
    for (int g = 0; g < G; ++g) {
      const double a = w ? E[(size_t)g * P + p] * w[g] : E[(size_t)g * P + p];
      s += a * ref[(size_t)kj * G + g];
    }
    R[o] = s;
  }
}

// MF: S by v_mfma_f64_16x16x4_f64 (the instance MB = 4: Theta padded to 16 columns; Q and Theta padded with zeros to PR = P rounded
// up to 16 rows and, Q, to P rounded up to 4 columns); else by plain multiplies and additions (PR = P)
template <int MB, bool MF>
__global__ __launch_bounds__(CE_NT) void k_ceig_solve(CeigArgs a, int ws_doubles, int PR, int QS) {
  extern __shared__ double lds[];
  constexpr int MP = 4 * MB, TS = MP + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)blockDim.x >> 6;
  const int K = a.K, P = a.P, M = a.M, D = a.D, DX = a.DX, J = a.J;
  double* sQ = lds;
  if (MF)
    for (int i = tid; i < PR * QS; i += (int)blockDim.x) sQ[i] = 0.0;
  __syncthreads();
  for (int i = tid; i < P * P; i += (int)blockDim.x) {
    const int p = i / P, p2 = i - p * P;
    sQ[p * QS + p2] = a.Q[i];
  }
  __syncthreads();
  const long long prob = (long long)blockIdx.x * nw + wave;
  if (prob >= a.N * K) return;                    // the whole wave; no workgroup barrier follows
  const long long cs = prob / K;
  const int k = (int)(prob - cs * K);
  double* sT = lds + (size_t)PR * QS + (size_t)wave * ws_doubles;     // Theta [p TS + m], later b [p TS + j]
  double* sS = sT + PR * TS;                      // [i TS + j]
  double* sV = sS + M * TS;
  double* sY = sV + M * TS;                       // [p CE_YS + jj]; MF: a 16 x 16 tile of Y, [row 17 + col]
  double* sL = sY + (MF ? 16 * 17 : P * CE_YS);   // lambda by rank (16), then the signs (16)
  double* sG = sL + CE_MMAX;
  int* sO = (int*)(sG + CE_MMAX);                 // the column of V of every rank (16)

  const int q = (int)(cs / a.S);
  const size_t t = (size_t)(a.first_slot + (cs - (long long)q * a.S));
  const int kk = a.perm[(size_t)cs * K + k];
  const double* phi = ptr_shift(a.c_Phi, (size_t)q * a.chain_bytes) + t * K * P * M + kk;                 // Phi: [k + K (p + P m)]
  const double* xi = DX > 0 ? ptr_shift(a.c_xi, (size_t)q * a.chain_bytes_cov) + t * K * P * D * M + (size_t)P * D * M * kk
                            : nullptr;                                                                    // xi: [p + P (d + D (m + M k))]
  for (int e = lane; e < PR * TS; e += 64) sT[e] = 0.0;
  wsync();
  for (int e = lane; e < P * M; e += 64) {
    const int m = e / P, p = e - m * P;
    double th = phi[(size_t)K * (p + (size_t)P * m)];
    for (int d = 0; d < DX; ++d) th += a.x[d] * xi[p + (size_t)P * (d + (size_t)D * m)];
    sT[p * TS + m] = th;
  }
  wsync();

  double y[MP];
#pragma unroll
  for (int m = 0; m < MP; ++m) y[m] = 0.0;
  if constexpr (MF) {
    // a 16-row tile of Y = Q Theta at a time (PR / 4 chained MFMAs: lane l holds A[row l & 15][k = 4 kb + (l >> 4)] of Q and
    // B[k][col l & 15] of Theta and receives D[row (l >> 4) + 4 reg][col l & 15], the mapping of k_curve_cov), staged in LDS and
    // taken into S = Theta' Y by four more, chained over the tiles in order
    const int lr = lane & 15, lk = lane >> 4;
    double4_t sacc = {0.0, 0.0, 0.0, 0.0};
    for (int pt = 0; pt < PR / 16; ++pt) {
      double4_t yacc = {0.0, 0.0, 0.0, 0.0};
      for (int kb = 0; kb < (P + 3) / 4; ++kb)
        yacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sQ[(16 * pt + lr) * QS + 4 * kb + lk], sT[(4 * kb + lk) * TS + lr], yacc, 0, 0, 0);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sY[(lk + 4 * reg) * 17 + lr] = yacc[reg];
      wsync();
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        sacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sT[(16 * pt + 4 * kb + lk) * TS + lr], sY[(4 * kb + lk) * 17 + lr], sacc, 0, 0, 0);
      wsync();
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = lk + 4 * reg;
      if (i < M && lr < M) sS[i * TS + lr] = sacc[reg];
    }
    wsync();
  } else {
  // Y = Q Theta, row `lane`
  if (lane < P)
    for (int p2 = 0; p2 < P; ++p2) {
      const double qv = sQ[lane * QS + p2];
#pragma unroll
      for (int m = 0; m < MP; ++m) y[m] += qv * sT[p2 * TS + m];
    }
  // S = Theta' Y, four columns at a time
#pragma unroll
  for (int jb = 0; jb < MB; ++jb) {
    if (lane < P) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) sY[lane * CE_YS + jj] = y[4 * jb + jj];
    }
    wsync();
    const int i = lane >> 2, j = 4 * jb + (lane & 3);
    if (i < M && j < M) {
      double s = 0.0;
      for (int p = 0; p < P; ++p) s += sT[p * TS + i] * sY[p * CE_YS + (lane & 3)];
      sS[i * TS + j] = s;
    }
    wsync();
  }
  }
  for (int e = lane; e < M * M; e += 64) {
    const int i = e / M, j = e - i * M;
    if (i > j) sS[i * TS + j] = sS[j * TS + i];
    sV[i * TS + j] = i == j ? 1.0 : 0.0;
  }
  wsync();
  double total = 0.0, fro2 = 0.0;
  if (lane == 0) {
    for (int i = 0; i < M; ++i) total += sS[i * TS + i];
    for (int i = 0; i < M; ++i)
      for (int j = i; j < M; ++j) {
        const double v = sS[i * TS + j];
        fro2 += i == j ? v * v : 2.0 * (v * v);
      }
  }
  total = __shfl(total, 0, 64);
  const double ufro = CE_U * sqrt(__shfl(fro2, 0, 64));

  // cyclic Jacobi, round-robin
  const int n = (M + 1) & ~1, nh = n >> 1;
  int sweeps = 0, capped = 0;
  for (;;) {
    int rot = 0;
    for (int r = 0; r < n - 1; ++r) {
      double c = 1.0, s = 0.0, npp = 0.0, nqq = 0.0;
      int p = 0, qd = 0, act = 0;
      if (lane < nh) {
        rr_pair(r, lane, n, p, qd);
        if (qd < M) {
          const double app = sS[p * TS + p], aqq = sS[qd * TS + qd], apq = sS[p * TS + qd];
          if (fabs(apq) > CE_U * fmax(sqrt(fabs(app * aqq)), ufro)) {
            act = 1;
            const double tau = (aqq - app) / (2.0 * apq);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            s = tt * c;
            npp = app - tt * apq;
            nqq = aqq + tt * apq;
          }
        }
      }
      rot |= act;
      if (!__any(act)) continue;                  // uniform over the wave
      wsync();
      // the columns of S and V
      int ip[2], iq[2], ii[2], on[2];
      double ic[2], is[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int it = lane + 64 * u, pi = it / M;
        ii[u] = it - pi * M;
        ic[u] = __shfl(c, pi & 63, 64);
        is[u] = __shfl(s, pi & 63, 64);
        on[u] = __shfl(act, pi & 63, 64) && pi < nh;
        rr_pair(r, min(pi, nh - 1), n, ip[u], iq[u]);
        if (on[u]) {
          const int i = ii[u];
          const double x0 = sS[i * TS + ip[u]], x1 = sS[i * TS + iq[u]];
          sS[i * TS + ip[u]] = ic[u] * x0 - is[u] * x1;
          sS[i * TS + iq[u]] = is[u] * x0 + ic[u] * x1;
          const double v0 = sV[i * TS + ip[u]], v1 = sV[i * TS + iq[u]];
          sV[i * TS + ip[u]] = ic[u] * v0 - is[u] * v1;
          sV[i * TS + iq[u]] = is[u] * v0 + ic[u] * v1;
        }
      }
      wsync();
      // the rows of S
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (on[u]) {
          const int i = ii[u];
          const double x0 = sS[ip[u] * TS + i], x1 = sS[iq[u] * TS + i];
          sS[ip[u] * TS + i] = ic[u] * x0 - is[u] * x1;
          sS[iq[u] * TS + i] = is[u] * x0 + ic[u] * x1;
        }
      wsync();
      if (act) {
        sS[p * TS + p] = npp;
        sS[qd * TS + qd] = nqq;
        sS[p * TS + qd] = 0.0;
        sS[qd * TS + p] = 0.0;
      }
      wsync();
    }
    ++sweeps;
    if (!__any(rot)) break;
    if (sweeps == CE_CAP) { capped = 1; break; }
  }

  // lambda by rank: descending, ties in index order, negative rounding noise clamped
  if (lane < M) {
    const double dj = sS[lane * TS + lane];
    int rank = 0;
    for (int i = 0; i < M; ++i) {
      const double di = sS[i * TS + i];
      rank += (di > dj || (di == dj && i < lane)) ? 1 : 0;
    }
    const double lj = dj > 0.0 ? dj : 0.0;
    sL[rank] = lj;
    sO[rank] = lane;
    const size_t row = (size_t)k * M + rank;
    a.lam[(size_t)cs + (size_t)a.N * row] = lj;
    a.pve[(size_t)cs + (size_t)a.N * row] = total == 0.0 ? 0.0 : lj / total;
  }
  if (lane == 0) {
    a.tot[(size_t)cs + (size_t)a.N * k] = total;
    a.status[(size_t)cs * K + k] = sweeps | (capped ? 0x100 : 0);
  }
  if (J < 1) return;
  wsync();
  // b_j = Theta v_j / sqrt(lambda_j): lane p's entries, then over its own row of Theta
  const double lzero = (double)M * CE_U * sL[0];
#pragma unroll
  for (int j = 0; j < MP; ++j) {
    y[j] = 0.0;
    if (j < J && lane < P) {
      const double lj = sL[j];
      if (lj > lzero) {
        const int col = sO[j];
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += sT[lane * TS + m] * sV[m * TS + col];
        y[j] = s / sqrt(lj);
      }
    }
  }
  wsync();
  if (lane < P) {
#pragma unroll
    for (int j = 0; j < MP; ++j) sT[lane * TS + j] = y[j];
  }
  wsync();
  if (a.R) {
    if (lane < J) {
      const double* rk = a.R + ((size_t)k * J + lane) * P;
      double s = 0.0;
      for (int p = 0; p < P; ++p) s += sT[p * TS + lane] * rk[p];
      sG[lane] = s >= 0.0 ? 1.0 : -1.0;
    }
  } else {
    for (int j = 0; j < J; ++j) {
      double best = -1.0, bv = 0.0;
      int bg = 0x7fffffff;
      for (int g = lane; g < a.G; g += 64) {
        const double* eg = a.E + (size_t)g * P;
        double v = 0.0;
        for (int p = 0; p < P; ++p) v += eg[p] * sT[p * TS + j];
        const double av = a.w ? sqrt(a.w[g]) * fabs(v) : fabs(v);
        if (av > best) { best = av; bv = v; bg = g; }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64), ov = __shfl_xor(bv, off, 64);
        const int og = __shfl_xor(bg, off, 64);
        if (ob > best || (ob == best && og < bg)) { best = ob; bv = ov; bg = og; }
      }
      if (lane == 0) sG[j] = bv >= 0.0 ? 1.0 : -1.0;
    }
  }
  wsync();
  double* bo = a.b + ((size_t)cs * K + k) * J * P;
  if (lane < P)
    for (int j = 0; j < J; ++j) bo[(size_t)j * P + lane] = sG[j] * sT[lane * TS + j];
}

// tiles [t0, ..) of the call's tiles, numbered kj TG + gt, times nb blocks of draws
__global__ __launch_bounds__(CE_NT) void k_ceig_values(const double* E, const double* b, int K, int J, int P, int G, long long N,
                                                       long long t0, int nb, long long r0, long long rows, double* V) {
  __shared__ double sB[CE_DB * (CE_PMAX + 1)];
  __shared__ double sE[CE_GT * CE_PMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int db = (int)(blockIdx.x % (unsigned)nb);
  const long long tile = t0 + (long long)(blockIdx.x / (unsigned)nb);
  const int TG = (G + CE_GT - 1) / CE_GT;
  const long long kj = tile / TG;
  const int gt = (int)(tile - kj * TG);
  const int g0 = gt * CE_GT, g1 = min(g0 + CE_GT, G);
  const long long efirst = kj * G + g0, elast = kj * G + g1 - 1;
  if (elast < r0 || efirst >= r0 + rows) return;
  const int PS = P | 1;
  const long long cs0 = (long long)db * CE_DB;
  for (int i = tid; i < CE_DB * P; i += CE_NT) {
    const int d = i / P, p = i - d * P;
    const long long cs = cs0 + d;
    sB[d * PS + p] = cs < N ? b[((size_t)cs * K * J + (size_t)kj) * P + p] : 0.0;
  }
  for (int i = tid; i < (g1 - g0) * P; i += CE_NT) sE[i] = E[(size_t)g0 * P + i];
  __syncthreads();
  const long long cs = cs0 + lane;
  if (cs >= N) return;
  for (int gi = wave; gi < g1 - g0; gi += CE_NT / 64) {
    const long long e = kj * G + g0 + gi - r0;
    if (e < 0 || e >= rows) continue;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += sE[gi * P + p] * sB[lane * PS + p];
    V[(size_t)cs + (size_t)N * (size_t)e] = s;
  }
}

// what the model fixes: the instance, the LDS of a wave and of the workgroup, the waves of a workgroup
struct CeigGeom {
  int MB = 0, DX = 0, ws = 0, nw = 0, mfma = 0, PR = 0, QS = 0;
  size_t lds = 0;
};

std::string ceig_geom(const Ctx& c, const CeigCall& f, CeigGeom& g) {
  const Dims& d = c.d;
  if (d.K < 1 || d.K > KMAX) return "K outside 1 .. 8";
  if (d.M < 1 || d.M > CE_MMAX) return "n_eigen outside 1 .. 16";
  if (d.D < 0 || d.D > CE_DMAX) return "more than 8 covariates";
  if (d.P < 1 || d.P > CE_PMAX) return "P outside 1 .. 64";
  if (f.G < 1 || f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "range outside the chain storage";
  if (f.J < 0 || f.J > d.M) return "n_functions outside 0 .. n_eigen";
  if ((long long)c.nch * f.n_slots > (1LL << 22)) return "more than 2^22 draws";
  if ((long long)d.K * d.M * f.G > 0x7fffffffLL / CE_PMAX) return "G K n_eigen P above 2^31 - 1";
  // the form of S: measured, plain multiplies and additions unless bfmmm_set_cluster_eig_form says otherwise
  g.mfma = g_cluster_eig_form == 2 ? 1 : 0;
  g.MB = g.mfma ? 4 : (d.M + 3) / 4;
  g.DX = f.x ? d.D : 0;
  const int TS = 4 * g.MB + 1;
  g.PR = g.mfma ? (d.P + 15) / 16 * 16 : d.P;
  g.QS = g.mfma ? (((d.P + 3) / 4 * 4) | 1) : (d.P | 1);
  g.ws = g.PR * TS + 2 * d.M * TS + (g.mfma ? 16 * 17 : d.P * CE_YS) + 3 * CE_MMAX;
  const size_t q = sizeof(double) * (size_t)g.PR * g.QS;
  g.nw = 4;
  while (g.nw > 1 && q + sizeof(double) * (size_t)g.ws * g.nw > CE_LDS_MAX) g.nw >>= 1;
  g.lds = q + sizeof(double) * (size_t)g.ws * g.nw;
  return "";
}

template <int MB, bool MF>
std::string ceig_solve_launch(const CeigArgs& a, const CeigGeom& g, hipStream_t st) {
  if (hipFuncSetAttribute((const void*)k_ceig_solve<MB, MF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CE_LDS_MAX) != hipSuccess) {
    (void)hipGetLastError();
    return "k_ceig_solve: cannot set the LDS size";
  }
  const long long probs = a.N * a.K, blocks = (probs + g.nw - 1) / g.nw;
  hipLaunchKernelGGL((k_ceig_solve<MB, MF>), dim3((unsigned)blocks), dim3(64 * g.nw), g.lds, st, a, g.ws, g.PR, g.QS);
  if (hipGetLastError() != hipSuccess) return "k_ceig_solve: launch failed";
  return "";
}

}  // namespace

int g_cluster_eig_form = 0;      // bfmmm_set_cluster_eig_form

std::string ceig_check(const Ctx& c, const CeigCall& f) {
  CeigGeom g;
  return ceig_geom(c, f, g);
}

int ceig_sweep_cap() { return CE_CAP; }

// Q (P x P) and, where ref is given and J > 0, R (K J x P) of the call
std::string launch_ceig_gram(const Ctx& c, const CeigCall& f, hipStream_t st) {
  CeigGeom g;
  const std::string err = ceig_geom(c, f, g);
  if (!err.empty()) return "k_ceig_gram: " + err;
  const bool with_r = f.ref && f.J > 0;
  if (!f.E || !f.Q || (with_r && !f.R)) return "k_ceig_gram: bad arguments";
  const int P = c.d.P, KJ = with_r ? c.d.K * f.J : 0;
  const long long cnt = (long long)P * P + (long long)KJ * P;
  hipLaunchKernelGGL(k_ceig_gram, dim3((unsigned)((cnt + CE_NT - 1) / CE_NT)), dim3(CE_NT), 0, st, f.E, f.w, f.ref, f.G, P, KJ, f.Q, f.R);
  if (hipGetLastError() != hipSuccess) return "k_ceig_gram: launch failed";
  return "";
}

// every draw's lambda, pve, total (draw-fastest rows), signed b and status word
std::string launch_ceig_solve(const Ctx& c, const CeigCall& f, hipStream_t st) {
  CeigGeom g;
  const std::string err = ceig_geom(c, f, g);
  if (!err.empty()) return "k_ceig_solve: " + err;
  const bool with_r = f.ref && f.J > 0;
  if (!f.perm || !f.Q || !f.lam || !f.pve || !f.tot || !f.status || (f.J > 0 && (!f.b || !f.E)) || (with_r && !f.R) ||
      (f.x && (!c.covariance_adj || c.d.D < 1)))
    return "k_ceig_solve: bad arguments";
  const Dims& d = c.d;
  CeigArgs a;
  a.c_Phi = c.c_Phi; a.c_xi = g.DX > 0 ? c.c_xi : nullptr;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.perm = f.perm; a.x = g.DX > 0 ? f.x : nullptr; a.E = f.E; a.w = f.w; a.Q = f.Q; a.R = with_r ? f.R : nullptr;
  a.lam = f.lam; a.pve = f.pve; a.tot = f.tot; a.b = f.b; a.status = f.status;
  a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.DX = g.DX; a.S = f.n_slots; a.first_slot = f.first_slot; a.G = f.G; a.J = f.J;
  a.N = (long long)c.nch * f.n_slots;
  if (g.mfma) return ceig_solve_launch<4, true>(a, g, st);
  switch (g.MB) {
    case 1: return ceig_solve_launch<1, false>(a, g, st);
    case 2: return ceig_solve_launch<2, false>(a, g, st);
    case 3: return ceig_solve_launch<3, false>(a, g, st);
    default: return ceig_solve_launch<4, false>(a, g, st);
  }
}

// the values V[cs + N (e - r0)] of result rows e = (k J + j) G + g in [r0, r0 + rows)
std::string launch_ceig_values(const Ctx& c, const CeigCall& f, long long r0, long long rows, double* V, hipStream_t st) {
  CeigGeom g;
  const std::string err = ceig_geom(c, f, g);
  if (!err.empty()) return "k_ceig_values: " + err;
  const long long len = (long long)c.d.K * f.J * f.G;
  if (rows < 1 || r0 < 0 || r0 + rows > len || !V || !f.E || !f.b) return "k_ceig_values: bad arguments";
  const long long N = (long long)c.nch * f.n_slots, nb = (N + CE_DB - 1) / CE_DB;
  const long long TG = (f.G + CE_GT - 1) / CE_GT;
  auto row_tile = [&](long long e) { return (e / f.G) * TG + (e % f.G) / CE_GT; };
  const long long t0 = row_tile(r0), t1 = row_tile(r0 + rows - 1) + 1;
  if ((t1 - t0) * nb > 0x7fffffffLL) return "k_ceig_values: too many workgroups in one chunk";
  hipLaunchKernelGGL(k_ceig_values, dim3((unsigned)((t1 - t0) * nb)), dim3(CE_NT), 0, st, f.E, f.b, c.d.K, f.J, c.d.P, f.G, N, t0, (int)nb,
                     r0, rows, V);
  if (hipGetLastError() != hipSuccess) return "k_ceig_values: launch failed";
  return "";
}

}  // namespace bfmmm
