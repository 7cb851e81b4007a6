// What k_predict (kernels_predict.hip) and k_predict_fit (kernels_predict_fit.hip; 7n) share: the arguments and the LDS
// layout of a workgroup, its sums, l(z) from the tables in LDS, the set-up of a workgroup and the whole of a draw -- steps (1) to (4)
// of kernels_predict.hip's header, the tables Gamma and tau and the R stages of the importance sampler.  Written once, so that the two
// kernels draw the same samples and return the same lpd, ess and memberships bit for bit.  k_lz_refine (kernels_loo_marginal.hip;
// 7o) runs the same set-up and draw once more for a listed (curve, draw) pair, from a given starting proposal (pred_draw<KT, true>).
// k_predict_lap (kernels_predict_laplace.hip; 7p) shares the set-up and steps (1) to (3), pred_tables, and has stages of its own.
#pragma once
#include "model.hpp"
#include "launchers.hpp"
#include "rng.hpp"

#include <cfloat>

namespace bfmmm {

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
  double *lpd_t, *ess_t, *m_t, *q_t, *prop, *samples;      // m_t and q_t go together; they, prop and samples may be null
  double* a_last;              // [row K + k]: the proposal of the draw's last stage (null: not stored)
  const double* a_start;       // [row K + k]: the proposal stage 0 starts from (pred_draw<KT, true> alone reads it)
  size_t chain_bytes, chain_bytes_cov;
  unsigned long long seed;
  uint32_t chain0, chain_stride;
  int n_new, K, P, M, D, BW, LG, LREC, cadj;
  int C, first_slot, S, J, R, r0, rows, SCH;
};

// the slot storage of the workgroup's chain
struct PredSlots { const double *c_nu, *c_Phi, *c_sigma, *c_pi, *c_alpha3, *c_eta, *c_xi; };
__device__ inline PredSlots pred_slots(const PredArgs& a, int q_chain) {
  PredSlots c;
  c.c_nu = ptr_shift(a.c_nu, (size_t)q_chain * a.chain_bytes);
  c.c_Phi = ptr_shift(a.c_Phi, (size_t)q_chain * a.chain_bytes);
  c.c_sigma = ptr_shift(a.c_sigma, (size_t)q_chain * a.chain_bytes);
  c.c_pi = ptr_shift(a.c_pi, (size_t)q_chain * a.chain_bytes);
  c.c_alpha3 = ptr_shift(a.c_alpha3, (size_t)q_chain * a.chain_bytes);
  c.c_eta = a.D > 0 ? ptr_shift(a.c_eta, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  c.c_xi = a.D > 0 ? ptr_shift(a.c_xi, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  return c;
}

// LDS doubles (the layout of k_predict; k_predict_fit puts its own tables behind `total`)
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
// upper triangle of W, factorised in place as step 4 of k_chain_curve_ll does.  It leaves b = L^-1 u in the first M entries and the
// off-diagonal entries of the factor L of A = sigma^2 I + W in the triangle (L_ck at tri_index(M, k, c), k < c); the diagonal entries
// still hold W_cc.
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

// Once per workgroup: the record of new curve r (the band of G [d P + p] = G(p, p + d), then s) and its x into LDS, the operand rows
// zeroed; *yy and *ni of the curve.  The first barrier of pred_draw closes it.
__device__ inline void pred_setup(const PredArgs& a, const PredLds& L, double* sm, int r, double* yy, int* ni) {
  const int tid = threadIdx.x, P = a.P, LG = a.LG;
  double* sRec = sm + L.rec;
  double* sX = sm + L.x;
  double* sTh = sm + L.th;
  double* sH = sm + L.h;
  const double* rec = a.rec + (size_t)r * a.LREC;
  for (int e = tid; e < LG; e += PR_NT) { const int d = e / P, p = e - d * P; sRec[e] = p + d < P ? rec[e] : 0.0; }
  for (int e = tid; e < P; e += PR_NT) sRec[LG + e] = rec[LG + e];
  *yy = rec[LG + P];
  *ni = a.ni[r];
  if (tid < a.D) sX[tid] = a.X[r + (size_t)a.n_new * tid];
  for (int e = tid; e < L.AP * L.PS; e += PR_NT) { sTh[e] = 0.0; sH[e] = 0.0; }
}

// Steps (1) to (3) of a draw at slot t of the workgroup's chain: theta, H, tau and Gamma into LDS, the draw's prior alpha_3 pi
// (PP_PRIOR) and sigma^2 (PP_SIG) into L.par.  It opens with the barrier that ends the previous draw's reads (and the set-up) and
// closes with the one behind Gamma.  pred_draw and k_predict_lap (kernels_predict_laplace.hip) both run it.
__device__ inline void pred_tables(const PredArgs& a, const PredLds& L, double* sm, const PredSlots& ch, size_t t) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, P = a.P, M = a.M, D = a.D, M1 = M + 1, BW = a.BW, LG = a.LG;
  const int A = L.A, AP = L.AP, PS = L.PS, GS = L.GS;
  double* sRec = sm + L.rec;
  double* sX = sm + L.x;
  double* sTh = sm + L.th;
  double* sH = sm + L.h;
  double* sTau = sm + L.tau;
  double* sGam = sm + L.gam;
  double* sPar = sm + L.par;
  const double *c_nu = ch.c_nu, *c_Phi = ch.c_Phi, *c_eta = ch.c_eta, *c_xi = ch.c_xi;
  __syncthreads();                            // the previous draw's readers are done (and the set-up)
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
  if (tid < K) sPar[PP_PRIOR + tid] = ch.c_alpha3[t] * ch.c_pi[t * K + tid];
  if (tid == 0) sPar[PP_SIG] = ch.c_sigma[t];
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
}

// One draw of new curve r (row rr of the chunk), chain q_chain, slot s (relative to first_slot): steps (1) to (4) into the chunk's
// traces.  It leaves in LDS theta (sm + L.th, rows and columns padded with zeros), sigma^2 (PP_SIG), the last stage's samples z
// [k J + j] and their weights w_j = exp(lw_j - max) (sm + L.lw), and in the lanes' Q columns what pred_ell left for the samples of
// the last pass of the lanes (j >= J - J % 256, or the last 256).  Returns the sum of those weights, the same bits on every thread.
// KT: the compile-time bound on K (4 or KMAX), so that a lane's z stays in registers.
// START (k_lz_refine of kernels_loo_marginal.hip): stage 0 proposes from a.a_start of the draw's row in place of the
// prior, so the Dirichlet correction applies in stage 0 as well; the variates come under UPD_LOO_REFINE, and the proposals and
// samples go to row prow of a.prop and a.samples, the pair's place in the list, not to the draw's row of the traces.
template <int KT, bool START = false>
__device__ inline double pred_draw(const PredArgs& a, const PredLds& L, double* sm, const PredSlots& ch, int r, int rr, int q_chain, int s,
                                   double yy, int ni, size_t prow = 0) {
  constexpr int NV = 2 + 2 * KT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, M = a.M, J = a.J, R = a.R;
  const int GS = L.GS;
  double* sTau = sm + L.tau;
  double* sGam = sm + L.gam;
  double* sQ = sm + L.q + tid;
  double* sZ = sm + L.z;           // [k J + j]
  double* sLw = sm + L.lw;
  double* sRed = sm + L.red;
  double* sPar = sm + L.par;
  const long long N = (long long)a.C * a.S;

  const size_t t = (size_t)(a.first_slot + s);
  const long long cs = (long long)q_chain * a.S + s;
  const size_t row = (size_t)rr * (size_t)N + (size_t)cs;
  if (!START) prow = row;
  constexpr uint32_t upd = START ? UPD_LOO_REFINE : UPD_PREDICT;
  double sw_last = 0.0;
  pred_tables(a, L, sm, ch, t);

  // (4) the stages
  const double sig = sPar[PP_SIG];
  const RngKey key = make_key(a.seed, a.chain0 + (uint32_t)q_chain * a.chain_stride, (uint32_t)t);
  for (int st = 0; st < R; ++st) {
    if (st == 0 && tid < K) sPar[PP_A + tid] = START ? a.a_start[row * K + tid] : sPar[PP_PRIOR + tid];
    __syncthreads();
    if (tid == 0) sPar[PP_LBC] = (START || st > 0) ? calc_lB(K, sPar + PP_A) - calc_lB(K, sPar + PP_PRIOR) : 0.0;
    if (a.prop && tid < K) a.prop[(prow * R + st) * K + tid] = sPar[PP_A + tid];
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
          const double g = fmax(rgamma(key, upd, (uint32_t)(i0 + k), sPar[PP_A + k], 1.0), DBL_MIN);
          sZ[k * J + j] = g;
          sum += g;
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) { const double gv = sZ[min(k, K - 1) * J + j]; z[k] = k < K ? gv / sum : 0.0; }
      }
      double lw = pred_ell<KT>(z, K, M, sGam, GS, sTau, sQ, yy, sig, ni);
      if (START || st > 0) {
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
          if (a.samples) a.samples[((prow * R + st) * J + j) * K + k] = z[k];
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
    sw_last = sw;
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
  if (a.m_t && tid < K) {
    const int src = a.perm ? a.perm[(size_t)cs * K + tid] : tid;
    a.m_t[row * K + tid] = sPar[PP_M + src];
    a.q_t[row * K + tid] = sPar[PP_Q + src];
  }
  if (a.a_last && tid < K) a.a_last[row * K + tid] = sPar[PP_A + tid];
  return sw_last;
}

inline int pred_kt(int K) { return K <= 4 ? 4 : KMAX; }
// the arguments of a launch over new curves [r0, r0 + rows) of call f, SCH included (kernels_predict.hip); a_start null
PredArgs pred_args(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t, double* prop,
                   double* samples, double* a_last = nullptr);

}  // namespace bfmmm
