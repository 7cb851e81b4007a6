// Prediction of held-out curves from the chain slots: for a new curve with record (G, s, yy, n*) and covariates x,
// every chain q and slot t, the integral of the marginal density l(z) of kernels_curve_ll.hip over Z_new ~ Dir(alpha_3 pi) by staged
// importance sampling.  With the draw's directions theta_a, a = (k, mt) (mt = 0: nu_k + eta_k x, mt = m: phi_km + xi_km x), A = K (M + 1):
//     Gamma_ab = theta_a' G theta_b,  tau_a = theta_a' s                                   (once per curve and draw)
//     c'Gc = sum_kk' z_k z_k' Gamma_(k0)(k'0),  c's = sum_k z_k tau_(k0),  rr = yy - 2 c's + c'Gc,
//     u_m = sum_k z_k tau_(km) - sum_kk' z_k z_k' Gamma_(km)(k'0),  W_ml = sum_kk' z_k z_k' Gamma_(km)(k'l),  A = sigma^2 I_M + W,
//     l(z) = -1/2 [ n* log 2 pi + (n* - M) log sigma^2 + log det A + (rr - u'A^-1 u) / sigma^2 ]
// so that a value of l costs about K^2 (M + 1)(M + 2) / 2 multiply-adds on a table in LDS and an M x M Cholesky, whatever n* and P.
//
// Geometry.  One workgroup of 256 threads owns a new curve, a chain and a run of SCH slots; the band of G and s sit in LDS for the
// whole launch.  Per draw:
//   (1) theta directions-major [a PS + p] with x folded in, rows padded with zeros to AP = A rounded up to 16, columns to 4
//   (2) H = Theta G over the band window, tau_a (p in order)
//   (3) Gamma = Theta H' on v_mfma_f64_16x16x4_f64, the upper-triangle 16 x 16 tiles only, dealt to the four waves; lane l holds
//       A[row l & 15][k = 4 kb + (l >> 4)] and B[k][col l & 15] and receives D[row (l >> 4) + 4 reg][col l & 15] (the mapping of
//       k_ceig_solve); an off-diagonal tile is also stored transposed
//   (4) the R stages: one lane per sample (a loop where J > 256): the gamma variates of rng.hpp, z, l(z) from broadcast reads of
//       Gamma with the lane's M x M system in its own LDS column, then the stage's sums in a fixed tree (the lane's samples in order,
//       the wave by DPP and two shuffles, the four waves in order) and the next proposal by thread 0
// Gamma and tau never leave LDS.  fp64, no atomics; every sum's order depends on (J, R) and the lane count of the workgroup alone: a
// value's bits depend on (curve, chain, slot, seed, J, R), not on the chunk, the grid or a repeated call.
#include "model.hpp"
#include "launchers.hpp"
#include "rng.hpp"

#include <algorithm>
#include <cfloat>
#include <string>

namespace bfmmm {

namespace {

constexpr int PR_NT = 256;
constexpr size_t PR_LDS_HARD = 160 * 1024;
constexpr int PR_PAR = 64;      // scalars of the draw and the stage (offsets below)
enum { PP_PRIOR = 0, PP_A = 8, PP_M = 16, PP_Q = 24, PP_TMP = 32, PP_SIG = 40, PP_LBC = 41 };

struct PredArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_nu, *c_Phi, *c_sigma, *c_eta, *c_xi, *c_pi, *c_alpha3;
  const double *rec, *X, *zs;
  const int* ni;
  const int32_t* perm;
  double *lpd_t, *ess_t, *m_t, *q_t, *prop, *samples;
  size_t chain_bytes, chain_bytes_cov;
  unsigned long long seed;
  uint32_t chain0, chain_stride;
  int n_new, K, P, M, D, BW, LG, LREC, cadj;
  int C, first_slot, S, J, R, r0, rows, SCH;
};

// LDS doubles (the layout of k_predict)
struct PredLds {
  int A, AP, PP, PS, GS, NQ;
  size_t rec, x, th, h, tau, gam, q, z, lw, red, par, total;
};
__host__ __device__ inline PredLds pred_lds(int K, int P, int M, int LG, int J, int KT) {
  PredLds L;
  L.A = K * (M + 1);
  L.AP = (L.A + 15) / 16 * 16;
  L.PP = (P + 3) / 4 * 4;
  L.PS = L.PP | 1;
  L.GS = L.AP + 1;
  L.NQ = M + M * (M + 1) / 2;
  size_t o = 0;
  L.rec = o; o += (size_t)LG + P;
  L.x = o; o += 8;
  L.th = o; o += (size_t)L.AP * L.PS;
  L.h = o; o += (size_t)L.AP * L.PS;
  L.tau = o; o += L.AP;
  L.gam = o; o += (size_t)L.AP * L.GS;
  L.q = o; o += (size_t)L.NQ * PR_NT;
  L.z = o; o += (size_t)K * J;
  L.lw = o; o += J;
  L.red = o; o += 4 * (size_t)(2 + 2 * KT);
  L.par = o; o += PR_PAR;
  L.total = o;
  return L;
}

// the sum of v[i], i < NV, over the workgroup's 256 threads, to every thread: the wave by DPP and two shuffles, the four waves in
// order.  Two barriers; sRed: 4 NV doubles.
template <int NV>
__device__ inline void block_sum(double (&v)[NV], double* sRed, int lane, int wave) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = group_sum<64>(v[i]);
    if (lane == 0) sRed[wave * NV + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = (sRed[i] + sRed[NV + i]) + (sRed[2 * NV + i] + sRed[3 * NV + i]);
  __syncthreads();
}
template <bool MAX>
__device__ inline double block_extreme(double v, double* sRed, int lane, int wave) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = MAX ? fmax(v, w) : fmin(v, w);
  }
  if (lane == 0) sRed[wave] = v;
  __syncthreads();
  v = MAX ? fmax(fmax(sRed[0], sRed[1]), fmax(sRed[2], sRed[3])) : fmin(fmin(sRed[0], sRed[1]), fmin(sRed[2], sRed[3]));
  __syncthreads();
  return v;
}

// l(z) of the draw whose Gamma and tau are in LDS; Q: the lane's column (stride PR_NT) of M + M (M + 1) / 2 doubles, u then the packed
// upper triangle of W, factorised in place as step 4 of k_chain_curve_ll does
template <int KT>
__device__ inline double pred_ell(const double (&z)[KT], int K, int M, const double* sGam, int GS, const double* sTau, double* Q,
                                  double yy, double sig, int ni) {
  const int M1 = M + 1;
  // no branch inside the sums: the entries k >= K of z are 0.0 and read the table at k = K - 1, so that a sum's loads go out together
  int ko[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) ko[k] = min(k, K - 1) * M1;
  double cs_ = 0.0, cGc = 0.0;
#pragma unroll
  for (int k = 0; k < KT; ++k) cs_ += z[k] * sTau[ko[k]];
#pragma nounroll
  for (int mt = 0; mt <= M; ++mt)
#pragma nounroll
    for (int l = mt; l <= M; ++l) {
      // mt = 0: Gamma_(k l)(k' 0), the row of u_l; else Gamma_(k mt)(k' l)
      const int ro = mt == 0 ? l : mt, co = mt == 0 ? 0 : l;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const double* g = sGam + (ko[k] + ro) * GS + co;
        double t = 0.0;
#pragma unroll
        for (int k2 = 0; k2 < KT; ++k2) t += z[k2] * g[ko[k2]];
        acc += z[k] * t;
      }
      if (mt == 0 && l == 0) cGc = acc;
      else if (mt == 0) {
        double tz = 0.0;
#pragma unroll
        for (int k = 0; k < KT; ++k) tz += z[k] * sTau[ko[k] + l];
        Q[(l - 1) * PR_NT] = tz - acc;
      } else {
        Q[(M + tri_index(M, mt - 1, l - 1)) * PR_NT] = acc;
      }
    }
  const double rr = yy - 2.0 * cs_ + cGc;
  double* b = Q;
  double* A = Q + (size_t)M * PR_NT;
  double logdet = 0.0, ww = 0.0;
#pragma nounroll
  for (int c = 0; c < M; ++c) {
    double dg = A[tri_index(M, c, c) * PR_NT] + sig;
    for (int k2 = 0; k2 < c; ++k2) { const double l2 = A[tri_index(M, k2, c) * PR_NT]; dg -= l2 * l2; }
    const double l = sqrt(dg);
    double wv = b[c * PR_NT];
    for (int k2 = 0; k2 < c; ++k2) wv -= A[tri_index(M, k2, c) * PR_NT] * b[k2 * PR_NT];
    wv /= l;
    b[c * PR_NT] = wv;
    logdet += 2.0 * log(l);
    ww += wv * wv;
    for (int r3 = c + 1; r3 < M; ++r3) {
      double v = A[tri_index(M, c, r3) * PR_NT];
      for (int k2 = 0; k2 < c; ++k2) v -= A[tri_index(M, k2, r3) * PR_NT] * A[tri_index(M, k2, c) * PR_NT];
      A[tri_index(M, c, r3) * PR_NT] = v / l;
    }
  }
  const double ld = (double)(ni - M) * log(sig) + logdet;
  const double quad = (rr - ww) / sig;
  return -(0.5 * ni) * 1.83787706640934548356 - 0.5 * ld - 0.5 * quad;
}

// KT: the compile-time bound on K (4 or KMAX), so that a lane's z stays in registers
template <int KT>
__global__ __launch_bounds__(PR_NT) void k_predict(PredArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr int NV = 2 + 2 * KT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, P = a.P, M = a.M, D = a.D, M1 = M + 1, BW = a.BW, LG = a.LG, J = a.J, R = a.R;
  const PredLds L = pred_lds(K, P, M, LG, J, KT);
  const int A = L.A, AP = L.AP, PS = L.PS, GS = L.GS;
  double* sRec = sm + L.rec;       // the band of G [d P + p] = G(p, p + d), then s
  double* sX = sm + L.x;
  double* sTh = sm + L.th;
  double* sH = sm + L.h;
  double* sTau = sm + L.tau;
  double* sGam = sm + L.gam;
  double* sQ = sm + L.q + tid;
  double* sZ = sm + L.z;           // [k J + j]
  double* sLw = sm + L.lw;
  double* sRed = sm + L.red;
  double* sPar = sm + L.par;

  const int rr = blockIdx.x;                    // the curve's row in the chunk
  const int r = a.r0 + rr;                      // its position in the call
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const long long N = (long long)a.C * a.S;
  const double* c_nu = ptr_shift(a.c_nu, (size_t)q_chain * a.chain_bytes);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q_chain * a.chain_bytes);
  const double* c_sigma = ptr_shift(a.c_sigma, (size_t)q_chain * a.chain_bytes);
  const double* c_pi = ptr_shift(a.c_pi, (size_t)q_chain * a.chain_bytes);
  const double* c_alpha3 = ptr_shift(a.c_alpha3, (size_t)q_chain * a.chain_bytes);
  const double* c_eta = D > 0 ? ptr_shift(a.c_eta, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  const double* c_xi = D > 0 ? ptr_shift(a.c_xi, (size_t)q_chain * a.chain_bytes_cov) : nullptr;

  // ---- once per workgroup: the record, x, zeroed operand rows ----
  const double* rec = a.rec + (size_t)r * a.LREC;
  for (int e = tid; e < LG; e += PR_NT) { const int d = e / P, p = e - d * P; sRec[e] = p + d < P ? rec[e] : 0.0; }
  for (int e = tid; e < P; e += PR_NT) sRec[LG + e] = rec[LG + e];
  const double yy = rec[LG + P];
  const int ni = a.ni[r];
  if (tid < D) sX[tid] = a.X[r + (size_t)a.n_new * tid];
  for (int e = tid; e < AP * PS; e += PR_NT) { sTh[e] = 0.0; sH[e] = 0.0; }

  for (int s = s_lo; s < s_hi; ++s) {
    const size_t t = (size_t)(a.first_slot + s);
    const long long cs = (long long)q_chain * a.S + s;
    const size_t row = (size_t)rr * (size_t)N + (size_t)cs;
    __syncthreads();                            // the previous draw's readers are done (and the set-up above)
    // (1) theta, directions-major, x folded in (nu: [k + K p], Phi: [k + K (p + P m)], eta: [p + P (d + D k)], xi: [p + P (d + D (m + M k))])
    for (int e = tid; e < A * P; e += PR_NT) {
      const int dir = e / P, p = e - dir * P, k = dir / M1, mt = dir - k * M1;
      double v = mt == 0 ? c_nu[t * K * P + (size_t)p * K + k] : c_Phi[t * K * P * M + k + (size_t)K * (p + (size_t)P * (mt - 1))];
      if (D > 0 && (mt == 0 || a.cadj)) {
        const double* tx = mt == 0 ? c_eta + t * P * D * K + p + (size_t)P * D * k
                                   : c_xi + t * K * P * D * M + p + (size_t)P * D * ((mt - 1) + (size_t)M * k);
        for (int d = 0; d < D; ++d) v += sX[d] * tx[(size_t)P * d];
      }
      sTh[dir * PS + p] = v;
    }
    if (tid < K) sPar[PP_PRIOR + tid] = c_alpha3[t] * c_pi[t * K + tid];
    if (tid == 0) sPar[PP_SIG] = c_sigma[t];
    __syncthreads();
    // (2) H = Theta G over the band window, tau = Theta s
    for (int e = tid; e < A * P; e += PR_NT) {
      const int dir = e / P, p = e - dir * P;
      const double* th = sTh + dir * PS;
      double hv = 0.0;
      for (int d = -BW; d <= BW; ++d) {
        // (no branch: outside the row the entry of G counts as 0.0 and both reads are moved inside it)
        const int p2 = p + d, pc = min(max(p2, 0), P - 1);
        const double g = sRec[(d < 0 ? -d : d) * P + min(p, pc)];
        hv += (p2 == pc ? g : 0.0) * th[pc];
      }
      sH[dir * PS + p] = hv;
    }
    if (tid < A) {
      const double* th = sTh + tid * PS;
      double s_ = 0.0;
      for (int p = 0; p < P; ++p) s_ += th[p] * sRec[LG + p];
      sTau[tid] = s_;
    }
    __syncthreads();
    // (3) Gamma = Theta H', upper-triangle tiles
    {
      const int lr = lane & 15, lk = lane >> 4, AT = AP / 16, ntile = AT * (AT + 1) / 2;
      for (int tile = wave; tile < ntile; tile += PR_NT / 64) {
        int ti = 0, rem = tile;
        while (rem >= AT - ti) { rem -= AT - ti; ++ti; }
        const int tj = ti + rem;
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
        const double* pa = sTh + (16 * ti + lr) * PS + lk;
        const double* pb = sH + (16 * tj + lr) * PS + lk;
        for (int kb = 0; kb < L.PP / 4; ++kb) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * kb], pb[4 * kb], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int i = 16 * ti + lk + 4 * reg, j = 16 * tj + lr;
          sGam[i * GS + j] = acc[reg];
          if (ti != tj) sGam[j * GS + i] = acc[reg];
        }
      }
    }
    __syncthreads();

    // (4) the stages
    const double sig = sPar[PP_SIG];
    const RngKey key = make_key(a.seed, a.chain0 + (uint32_t)q_chain * a.chain_stride, (uint32_t)t);
    for (int st = 0; st < R; ++st) {
      if (st == 0 && tid < K) sPar[PP_A + tid] = sPar[PP_PRIOR + tid];
      __syncthreads();
      if (tid == 0) sPar[PP_LBC] = st > 0 ? calc_lB(K, sPar + PP_A) - calc_lB(K, sPar + PP_PRIOR) : 0.0;
      if (a.prop && tid < K) a.prop[(row * R + st) * K + tid] = sPar[PP_A + tid];
      __syncthreads();
      const double lbc = sPar[PP_LBC];
      double lmax = -INFINITY;
#pragma nounroll
      for (int j = tid; j < J; j += PR_NT) {
        double z[KT];
        if (a.zs) {
#pragma unroll
          for (int k = 0; k < KT; ++k) { const double zv = a.zs[((size_t)cs * J + j) * K + min(k, K - 1)]; z[k] = k < K ? zv : 0.0; }
        } else {
          const unsigned long long i0 = (((unsigned long long)r * R + st) * J + j) * K;
          double sum = 0.0;
#pragma nounroll
          for (int k = 0; k < K; ++k) {
            const double g = fmax(rgamma(key, UPD_PREDICT, (uint32_t)(i0 + k), sPar[PP_A + k], 1.0), DBL_MIN);
            sZ[k * J + j] = g;
            sum += g;
          }
#pragma unroll
          for (int k = 0; k < KT; ++k) { const double gv = sZ[min(k, K - 1) * J + j]; z[k] = k < K ? gv / sum : 0.0; }
        }
        double lw = pred_ell<KT>(z, K, M, sGam, GS, sTau, sQ, yy, sig, ni);
        if (st > 0) {
          double corr = lbc;
#pragma unroll
          for (int k = 0; k < KT; ++k) {      // (k >= K: log 1 = 0 times a difference that is there)
            const int kc = min(k, K - 1);
            corr += (sPar[PP_PRIOR + kc] - sPar[PP_A + kc]) * log(k < K ? z[k] : 1.0);
          }
          lw += corr;
        }
#pragma unroll
        for (int k = 0; k < KT; ++k)
          if (k < K) {
            sZ[k * J + j] = z[k];
            if (a.samples) a.samples[((row * R + st) * J + j) * K + k] = z[k];
          }
        sLw[j] = lw;
        lmax = fmax(lmax, lw);
      }
      lmax = block_extreme<true>(lmax, sRed, lane, wave);
      // the stage's sums: v[0] = sum w, v[1] = sum w^2, v[2 + k] = sum w z_k, v[2 + KT + k] = sum w z_k^2; sLw keeps w
      double v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = 0.0;
#pragma nounroll
      for (int j = tid; j < J; j += PR_NT) {
        const double w = exp(sLw[j] - lmax);
        sLw[j] = w;
        v[0] += w;
        v[1] += w * w;
#pragma unroll
        for (int k = 0; k < KT; ++k) {          // (k >= K: a copy of k = K - 1 that nobody reads)
          const double zk = sZ[min(k, K - 1) * J + j], wz = w * zk;
          v[2 + k] += wz;
          v[2 + KT + k] += wz * zk;
        }
      }
      block_sum<NV>(v, sRed, lane, wave);
      const double sw = v[0];
      double mk[KT], vv[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) { mk[k] = v[2 + k] / sw; vv[k] = 0.0; }
      if (st + 1 < R) {
        // v_k in a second pass
#pragma nounroll
        for (int j = tid; j < J; j += PR_NT) {
          const double w = sLw[j];
#pragma unroll
          for (int k = 0; k < KT; ++k) { const double dz = sZ[min(k, K - 1) * J + j] - mk[k]; vv[k] += w * (dz * dz); }
        }
        block_sum<KT>(vv, sRed, lane, wave);
      }
      if (tid == 0) {
        if (st + 1 < R) {
          // the next proposal: the median of r_k = m_k (1 - m_k) / v_k - 1 over v_k > 0, sorted in LDS
          double* rs = sPar + PP_TMP;
          int cnt = 0;
#pragma unroll
          for (int k = 0; k < KT; ++k)
            if (k < K) {
              const double vk = vv[k] / sw;
              if (vk > 0.0) {
                const double rk = mk[k] * (1.0 - mk[k]) / vk - 1.0;
                int pos = cnt++;
                while (pos > 0 && rs[pos - 1] > rk) { rs[pos] = rs[pos - 1]; --pos; }
                rs[pos] = rk;
              }
            }
          double a0 = cnt == 0 ? 1e4 : (cnt & 1) ? rs[cnt / 2] : 0.5 * (rs[cnt / 2 - 1] + rs[cnt / 2]);
          a0 = fmin(fmax(a0, 1.0), 1e4);
#pragma unroll
          for (int k = 0; k < KT; ++k)
            if (k < K) sPar[PP_A + k] = fmax(a0 * mk[k], 0.5);
        } else {
#pragma unroll
          for (int k = 0; k < KT; ++k)
            if (k < K) { sPar[PP_M + k] = mk[k]; sPar[PP_Q + k] = v[2 + KT + k] / sw; }
          a.lpd_t[row] = lmax + log(sw / (double)J);
          a.ess_t[row] = sw * sw / v[1];
        }
      }
    }
    __syncthreads();
    if (tid < K) {
      const int src = a.perm ? a.perm[(size_t)cs * K + tid] : tid;
      a.m_t[row * K + tid] = sPar[PP_M + src];
      a.q_t[row * K + tid] = sPar[PP_Q + src];
    }
  }
}

// One workgroup per row: lpd = log mean exp lpd_t by a max-shifted sum, the means of m, q and ess and the least ess, every sum in the
// order of block_sum (a thread's draws in order first)
__global__ __launch_bounds__(PR_NT) void k_predict_pool(int K, long long N, const double* lpd_t, const double* ess_t, const double* m_t,
                                                        const double* q_t, double* lpd, double* z_mean, double* z_sd, double* ess_mean,
                                                        double* ess_min) {
  __shared__ double sRed[4 * (2 + 2 * KMAX)];
  constexpr int NV = 2 + 2 * KMAX;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r = blockIdx.x;
  const double* lp = lpd_t + r * (size_t)N;
  const double* es = ess_t + r * (size_t)N;
  double mx = -INFINITY, mn = INFINITY;
  for (long long o = tid; o < N; o += PR_NT) { mx = fmax(mx, lp[o]); mn = fmin(mn, es[o]); }
  mx = block_extreme<true>(mx, sRed, lane, wave);
  mn = block_extreme<false>(mn, sRed, lane, wave);
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  for (long long o = tid; o < N; o += PR_NT) {
    v[0] += exp(lp[o] - mx);
    v[1] += es[o];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {          // (k >= K: a copy of k = K - 1 that nobody reads; the loads go out together)
      const size_t e = (r * (size_t)N + (size_t)o) * K + min(k, K - 1);
      v[2 + k] += m_t[e];
      v[2 + KMAX + k] += q_t[e];
    }
  }
  block_sum<NV>(v, sRed, lane, wave);
  if (tid == 0) {
    const double n = (double)N;
    lpd[r] = mx + log(v[0] / n);
    ess_mean[r] = v[1] / n;
    ess_min[r] = mn;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        const double m = v[2 + k] / n;
        z_mean[r * K + k] = m;
        z_sd[r * K + k] = sqrt(fmax(v[2 + KMAX + k] / n - m * m, 0.0));
      }
  }
}

int pred_kt(int K) { return K <= 4 ? 4 : KMAX; }

}  // namespace

std::string predict_check(const Ctx& c, const PredictCall& f, size_t* lds_bytes) {
  const Dims& d = c.d;
  if (d.P < 1 || d.P > PMAX) return "k_predict: P outside 1 .. 64";
  if (d.M < 1 || d.M > 16) return "k_predict: n_eigen outside 1 .. 16";
  if (d.K < 1 || d.K > KMAX) return "k_predict: K outside 1 .. 8";
  if (d.D < 0 || d.D > 8) return "k_predict: more than 8 covariates";
  if (d.BW < 0 || d.BW > BWWIDE) return "k_predict: band half-width above 31";
  if (c.nch < 1 || c.nch > 65535) return "k_predict: more than 65535 chains";
  if (f.J < 1 || f.R < 1 || f.n_slots < 1 || f.first_slot < 0 || f.first_slot + f.n_slots > c.T) return "k_predict: range outside the chain storage";
  // J (K + 1) doubles of a stage's samples: beyond 2^24 samples nothing fits, whatever the rest
  const PredLds L = pred_lds(d.K, d.P, d.M, d.LG, std::min(f.J, 1 << 24), pred_kt(d.K));
  const size_t bytes = L.total * sizeof(double);
  if (lds_bytes) *lds_bytes = bytes;
  if (bytes > PR_LDS_HARD || f.J > (1 << 24))
    return "k_predict: the tables of a draw (Gamma of " + std::to_string(L.AP) + " x " + std::to_string(L.AP) + " for K (n_eigen + 1) = " +
           std::to_string(L.A) + " directions, the " + std::to_string((long long)f.J) + " x (K + 1) values of a stage's samples) need " +
           (f.J > (1 << 24) ? std::string("more than 1073741824") : std::to_string(bytes)) + " bytes of LDS, above the limit of " +
           std::to_string(PR_LDS_HARD) + " (160 KiB)";
  return "";
}

std::string launch_predict(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                           double* prop, double* samples, hipStream_t st) {
  size_t lds = 0;
  const std::string bad = predict_check(c, f, &lds);
  if (!bad.empty()) return bad;
  if (rows < 1 || r0 < 0 || (long long)r0 + rows > f.n_new) return "k_predict: curves outside the call";
  const Dims& d = c.d;
  PredArgs a;
  a.c_nu = c.c_nu; a.c_Phi = c.c_Phi; a.c_sigma = c.c_sigma; a.c_pi = c.c_pi; a.c_alpha3 = c.c_alpha3;
  a.c_eta = d.D > 0 ? c.c_eta : nullptr; a.c_xi = d.D > 0 ? c.c_xi : nullptr;
  a.rec = f.rec; a.X = d.D > 0 ? f.X : nullptr; a.zs = f.zs; a.ni = f.ni; a.perm = f.perm;
  a.lpd_t = lpd_t; a.ess_t = ess_t; a.m_t = m_t; a.q_t = q_t; a.prop = prop; a.samples = samples;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.seed = f.seed; a.chain0 = c.chain; a.chain_stride = c.chain_id_stride;
  a.n_new = f.n_new; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.BW = d.BW; a.LG = d.LG; a.LREC = d.LREC;
  a.cadj = (d.D > 0 && c.covariance_adj) ? 1 : 0;
  a.C = c.nch; a.first_slot = f.first_slot; a.S = f.n_slots; a.J = f.J; a.R = f.R; a.r0 = r0; a.rows = rows;
  // slots per workgroup: several workgroups per curve and chain while the grid stays below about eight per CU
  long long sch = ((long long)rows * c.nch * f.n_slots + 2047) / 2048;
  sch = std::max<long long>(1, std::min<long long>(sch, f.n_slots));
  while (((long long)f.n_slots + sch - 1) / sch > 65535) sch *= 2;
  a.SCH = (int)sch;
  const dim3 grid((unsigned)rows, (unsigned)((f.n_slots + a.SCH - 1) / a.SCH), (unsigned)c.nch);
  void (*fn)(PredArgs) = pred_kt(d.K) == 4 ? k_predict<4> : k_predict<KMAX>;
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_predict: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, grid, dim3(PR_NT), lds, st, a);
  if (hipGetLastError() != hipSuccess) return "k_predict: launch failed";
  return "";
}

std::string launch_predict_pool(int K, long long N, int rows, const double* lpd_t, const double* ess_t, const double* m_t, const double* q_t,
                                double* lpd, double* z_mean, double* z_sd, double* ess_mean, double* ess_min, hipStream_t st) {
  if (K < 1 || K > KMAX || N < 1 || rows < 1) return "k_predict_pool: bad shape";
  hipLaunchKernelGGL(k_predict_pool, dim3((unsigned)rows), dim3(PR_NT), 0, st, K, N, lpd_t, ess_t, m_t, q_t, lpd, z_mean, z_sd, ess_mean, ess_min);
  if (hipGetLastError() != hipSuccess) return "k_predict_pool: launch failed";
  return "";
}

}  // namespace bfmmm
