// The Laplace mixture proposal for the membership integral of the prediction and of the marginal LOO: per (curve,
// chain, slot) log p(y | draw) = log int exp g(eta) d eta over the log-ratios eta of the memberships (laplace_core.hpp), by
// importance sampling in one round from a mixture of Student-t components with 4 degrees of freedom:
//   component 0 (defensive, always there): centre log-ratios of p = alpha / alpha_0, scale [alpha_0 (diag p - p p')]^-1,
//               J_0 = max(1, J / 16) samples
//   component c >= 1: a converged mode eta_c of g with Sigma_c = (-H_c)^-1 = L_c L_c', mass w_c ~ exp(g_c) prod diag L_c,
//               J_c = floor((J - J_0) w_c) samples, the remainder to the heaviest; J_c = 0 leaves the mixture
// Geometry, set-up and steps (1) to (3) of a draw are k_predict's (pred_setup and pred_tables of predict_core.hpp).  Then
//   (4) the search: K + 1 starts (z = alpha / alpha_0; for each k, 0.9 at k and 0.1 / (K - 1) elsewhere), one wave a start, dealt
//       to the four waves in turn, the tables of a derivative evaluation dealt to the wave's lanes (lap_search of laplace_core.hpp);
//       thread 0 keeps the converged starts that lie further than 1e-3 (max norm) from an earlier one, in start order, and forms
//       the sample counts
//   (5) one pass with one lane a sample (a loop where J > 256), samples contiguous by component in component order:
//       eta_j = eta_c + L_c eps_j sqrt(4 / chi2_j), eps from rnorm, chi2 = -2 log(U1 U2) from runif, key (seed, RNG chain id, slot),
//       update id UPD_PREDICT_LAPLACE, index (r J + j)(d + 2) + i (i < d: the normals, d and d + 1: the uniforms);
//       lw_j = g(eta_j) - log sum_c (J_c / J) t4(eta_j; eta_c, L_c) with l from pred_ell, then the sums of k_predict's last stage in
//       its order (block_extreme, block_sum): lpd = max + log(sum w / J), ess, m_k, q_k
// The search's scratch lies where the lanes' Q columns, the samples and the weights of step (5) go afterwards.  fp64, vector stores
// only, no atomics; a value's bits depend on (curve, chain, slot, seed, J) alone, not on the chunk, the grid or a repeated call.
#include "model.hpp"
#include "launchers.hpp"
#include "predict_core.hpp"
#include "laplace_core.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

// The LDS of k_predict_lap: k_predict's record, theta, H, tau and Gamma where they are; behind them the scalars, the sums, the
// results of the K + 1 starts and the K + 2 components (CS doubles each: centre, packed L, g, J_c, sum log diag L, and the converged
// flag of a start or the log constant of a component), then the search's scratch (SS doubles a start) under Q, z and lw.
struct LapLds {
  PredLds p;
  int SS, CS;
  size_t scr, res, comp, total;
};
__host__ __device__ inline LapLds lap_lds(int K, int P, int M, int LG, int J, int KT) {
  LapLds L;
  L.p = pred_lds(K, P, M, LG, J, KT);
  const int d = K - 1;
  L.CS = d + d * (d + 1) / 2 + 4;
  L.SS = lap_scratch(K, M) | 1;
  size_t o = L.p.q;
  L.p.par = o; o += PR_PAR;
  L.p.red = o; o += 4 * (size_t)(2 + 2 * KT);
  L.res = o; o += (size_t)(K + 1) * L.CS;
  L.comp = o; o += (size_t)(K + 2) * L.CS;
  L.p.q = o; o += (size_t)L.p.NQ * PR_NT;
  L.p.z = o; o += (size_t)K * J;
  L.p.lw = o; o += J;
  L.scr = L.p.q;
  L.total = std::max(o, L.scr + (size_t)(K + 1) * L.SS);
  L.p.total = L.total;
  return L;
}

struct LapOut {
  int32_t* n_modes;            // [row]
  double *comps, *eta;         // [(row (K + 2) + c) (CS - 2) + .], [(row J + j) d + i]; either may be null
};

// z of a lane's eta (entries k >= d of eta are not read), clamped as lap_z does; z_k = 0 for k >= K
template <int KT>
__device__ inline void lap_z_lane(int K, const double (&eta)[KT], double (&z)[KT]) {
  const int d = K - 1;
  double mx = 0.0, sum = 0.0;
#pragma unroll
  for (int k = 0; k < KT; ++k) mx = k < d ? fmax(mx, eta[k]) : mx;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    z[k] = k < K ? exp((k < d ? eta[k] : 0.0) - mx) : 0.0;
    sum += z[k];
  }
#pragma unroll
  for (int k = 0; k < KT; ++k) z[k] = k < K ? fmax(z[k] / sum, DBL_MIN) : 0.0;
}

template <int KT>
__device__ inline void lap_draw(const PredArgs& a, const LapOut& out, const LapLds& LL, double* sm, const PredSlots& ch, int r, int rr,
                                int q_chain, int s, double yy, int ni) {
  constexpr int NV = 2 + 2 * KT;
  const PredLds& L = LL.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, M = a.M, J = a.J, d = K - 1, CS = LL.CS, NL = d * (d + 1) / 2, GS = L.GS;
  double* sTau = sm + L.tau;
  double* sGam = sm + L.gam;
  double* sQ = sm + L.q + tid;
  double* sZ = sm + L.z;           // [k J + j]
  double* sLw = sm + L.lw;
  double* sRed = sm + L.red;
  double* sPar = sm + L.par;
  double* sRes = sm + LL.res;
  double* sComp = sm + LL.comp;
  const long long N = (long long)a.C * a.S;
  const size_t t = (size_t)(a.first_slot + s);
  const long long cs = (long long)q_chain * a.S + s;
  const size_t row = (size_t)rr * (size_t)N + (size_t)cs;
  pred_tables(a, L, sm, ch, t);
  if (tid == 0) sPar[PP_LBC] = calc_lB(K, sPar + PP_PRIOR);
  __syncthreads();
  const double sig = sPar[PP_SIG], lBa = sPar[PP_LBC];

  // (4) the search: wave w runs starts w, w + 4, ... one after the other, its 64 lanes together (lap_eval); every lane ends with
  // the same values and writes the same result
  for (int st = wave; st <= K; st += PR_NT / 64) {
    const LapWs w = lap_ws(sm + LL.scr + (size_t)st * LL.SS, K, M);
    LapCase c;
    c.Gam = sGam; c.tau = sTau; c.alpha = sPar + PP_PRIOR; c.lBa = lBa; c.yy = yy; c.sig = sig; c.GS = GS; c.K = K; c.M = M; c.ni = ni;
    double a0 = 0.0;
    for (int k = 0; k < K; ++k) a0 += sPar[PP_PRIOR + k];
    const double off = d > 0 ? 0.1 / (double)d : 0.0;
    const double zl = st == 0 ? sPar[PP_PRIOR + d] / a0 : (st - 1 == d ? 0.9 : off);
    for (int k = 0; k < d; ++k) w.eta[k] = log((st == 0 ? sPar[PP_PRIOR + k] / a0 : (st - 1 == k ? 0.9 : off)) / zl);
    double g, g0;
    int iters;
    const bool ok = lap_search(c, w, &g, &g0, &iters, lane, 64);
    double* res = sRes + st * CS;
    double sl = 0.0;
    if (ok) sl = lap_scale_factor(d, w.C, w.H, res + d);
    for (int k = 0; k < d; ++k) res[k] = w.eta[k];
    res[d + NL] = ok ? g : g0;
    res[d + NL + 1] = g0;                    // (a component's J_c goes here)
    res[d + NL + 2] = sl;
    res[d + NL + 3] = (ok && fabs(sl) < INFINITY) ? 1.0 : 0.0;
  }
  __syncthreads();
  // the components and their sample counts
  if (tid == 0) {
    const double lconst = lgamma_pos(0.5 * (4.0 + d)) - 0.5 * d * log(4.0 * 3.14159265358979323846);
    for (int e = 0; e < (K + 2) * CS; ++e) sComp[e] = 0.0;
    // component 0: L_0 L_0' = (diag(1 / p) + 1 1' / p_K) / alpha_0, factorised through the scratch of start 0
    {
      double* tmp = sm + LL.scr;
      for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) tmp[i * d + j] = ((i == j ? 1.0 / sPar[PP_PRIOR + i] : 0.0) + 1.0 / sPar[PP_PRIOR + d]);
      double* C0 = tmp + d * d;
      double sl = 0.0;
      const bool ok0 = lap_chol(d, tmp, 0.0, 1.0, C0);
      for (int i = 0; i < d; ++i) {
        sComp[i] = log(sPar[PP_PRIOR + i] / sPar[PP_PRIOR + d]);
        for (int j = 0; j <= i; ++j) sComp[d + i * (i + 1) / 2 + j] = ok0 ? C0[i * d + j] : (i == j ? 1.0 : 0.0);
        sl += ok0 ? log(C0[i * d + i]) : 0.0;
      }
      sComp[d + NL] = sRes[d + NL + 1];        // g at the centre, the first value of start 0
      sComp[d + NL + 2] = sl;
    }
    int nm = 0;
    for (int st = 0; st <= K; ++st) {
      const double* res = sRes + st * CS;
      if (res[d + NL + 3] == 0.0) continue;
      bool dup = false;
      for (int c = 1; c <= nm && !dup; ++c) {
        double dist = 0.0;
        for (int k = 0; k < d; ++k) dist = fmax(dist, fabs(res[k] - sComp[c * CS + k]));
        dup = dist < LAP_SAME;
      }
      if (dup) continue;
      ++nm;
      for (int e = 0; e < CS; ++e) sComp[nm * CS + e] = res[e];
    }
    const int J0 = nm == 0 ? J : max(1, J / 16), rest = J - J0;
    sComp[d + NL + 1] = (double)J0;
    double mx = -INFINITY, sw = 0.0;
    for (int c = 1; c <= nm; ++c) mx = fmax(mx, sComp[c * CS + d + NL] + sComp[c * CS + d + NL + 2]);
    for (int c = 1; c <= nm; ++c) sw += exp(sComp[c * CS + d + NL] + sComp[c * CS + d + NL + 2] - mx);
    int given = 0, heavy = 1;
    double wbest = -1.0;
    for (int c = 1; c <= nm; ++c) {
      const double wc = exp(sComp[c * CS + d + NL] + sComp[c * CS + d + NL + 2] - mx) / sw;
      const int Jc = min(rest - given, (int)floor((double)rest * wc));
      sComp[c * CS + d + NL + 1] = (double)Jc;
      given += Jc;
      if (wc > wbest) { wbest = wc; heavy = c; }
    }
    if (nm > 0) sComp[heavy * CS + d + NL + 1] += (double)(rest - given);
    // the log constant of a component's term of the mixture density
    for (int c = 0; c <= nm; ++c) {
      const double Jc = sComp[c * CS + d + NL + 1];
      sComp[c * CS + d + NL + 3] = Jc > 0.0 ? log(Jc / (double)J) + lconst - sComp[c * CS + d + NL + 2] : -INFINITY;
    }
    out.n_modes[row] = nm;
    if (out.comps) {
      double* oc = out.comps + row * (size_t)(K + 2) * (CS - 2);
      for (int c = 0; c < K + 2; ++c)
        for (int e = 0; e < CS - 2; ++e) oc[c * (CS - 2) + e] = sComp[c * CS + e];
    }
    sPar[PP_TMP] = (double)nm;
  }
  __syncthreads();

  // (5) the samples and their weights
  const int nc = (int)sPar[PP_TMP] + 1;
  const RngKey key = make_key(a.seed, a.chain0 + (uint32_t)q_chain * a.chain_stride, (uint32_t)t);
  double lmax = -INFINITY;
#pragma nounroll
  for (int j = tid; j < J; j += PR_NT) {
    int c = 0, upto = (int)sComp[d + NL + 1];
    while (j >= upto && c + 1 < nc) { ++c; upto += (int)sComp[c * CS + d + NL + 1]; }
    const double* cp = sComp + c * CS;
    const unsigned long long i0 = ((unsigned long long)r * J + j) * (unsigned long long)(d + 2);
    double eps[KT], eta[KT], z[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) eps[i] = i < d ? rnorm(key, UPD_PREDICT_LAPLACE, (uint32_t)(i0 + i)) : 0.0;
    const double u1 = runif(key, UPD_PREDICT_LAPLACE, (uint32_t)(i0 + d)), u2 = runif(key, UPD_PREDICT_LAPLACE, (uint32_t)(i0 + d + 1));
    const double sc = sqrt(4.0 / (-2.0 * log(u1 * u2)));
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      double v = 0.0;
#pragma unroll
      for (int i2 = 0; i2 < KT; ++i2) v += (i2 <= i && i < d) ? cp[d + i * (i + 1) / 2 + i2] * eps[i2] : 0.0;
      eta[i] = i < d ? cp[i] + sc * v : 0.0;
    }
    lap_z_lane<KT>(K, eta, z);
    double g = pred_ell<KT>(z, K, M, sGam, GS, sTau, sQ, yy, sig, ni) - lBa;
#pragma unroll
    for (int k = 0; k < KT; ++k) g += k < K ? sPar[PP_PRIOR + k] * log(z[k]) : 0.0;
    // log q: a max-shifted sum over the components in order
    double qmx = -INFINITY, qs = 0.0;
    for (int c2 = 0; c2 < nc; ++c2) {
      const double* c2p = sComp + c2 * CS;
      const double lc = c2p[d + NL + 3];
      if (!(lc > -INFINITY)) continue;
      double x[KT], q2 = 0.0;
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        double v = i < d ? eta[i] - c2p[i] : 0.0;
#pragma unroll
        for (int i2 = 0; i2 < KT; ++i2) v -= (i2 < i && i < d) ? c2p[d + i * (i + 1) / 2 + i2] * x[i2] : 0.0;
        x[i] = i < d ? v / c2p[d + i * (i + 1) / 2 + i] : 0.0;
        q2 += x[i] * x[i];
      }
      const double term = lc - 0.5 * (4.0 + d) * log1p(0.25 * q2);
      if (term > qmx) { qs = qs * exp(qmx - term) + 1.0; qmx = term; }
      else qs += exp(term - qmx);
    }
    const double lw = g - (qmx + log(qs));
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (k < K) sZ[k * J + j] = z[k];
    if (out.eta) {
#pragma unroll
      for (int i = 0; i < KT; ++i)
        if (i < d) out.eta[(row * J + j) * d + i] = eta[i];
    }
    sLw[j] = lw;
    lmax = fmax(lmax, lw);
  }
  lmax = block_extreme<true>(lmax, sRed, lane, wave);
  // v[0] = sum w, v[1] = sum w^2, v[2 + k] = sum w z_k, v[2 + KT + k] = sum w z_k^2
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
#pragma nounroll
  for (int j = tid; j < J; j += PR_NT) {
    const double w = exp(sLw[j] - lmax);
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
  if (tid == 0) {
    a.lpd_t[row] = lmax + log(sw / (double)J);
    a.ess_t[row] = sw * sw / v[1];
  }
  if (a.m_t) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      // thread l writes column l, which holds label perm[l]
      const int src = (tid < K && a.perm) ? a.perm[(size_t)cs * K + tid] : tid;
      if (tid < K && src == k) {
        a.m_t[row * K + tid] = v[2 + k] / sw;
        a.q_t[row * K + tid] = v[2 + KT + k] / sw;
      }
    }
  }
}

template <int KT>
__global__ __launch_bounds__(PR_NT) void k_predict_lap(PredArgs a, LapOut out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const LapLds LL = lap_lds(a.K, a.P, a.M, a.LG, a.J, KT);
  const int rr = blockIdx.x;                    // the curve's row in the chunk
  const int r = a.r0 + rr;                      // its position in the call
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const PredSlots ch = pred_slots(a, q_chain);
  double yy;
  int ni;
  pred_setup(a, LL.p, sm, r, &yy, &ni);
  for (int s = s_lo; s < s_hi; ++s) lap_draw<KT>(a, out, LL, sm, ch, r, rr, q_chain, s, yy, ni);
}

}  // namespace

std::string predict_lap_check(const Ctx& c, const PredictCall& f, size_t* lds_bytes) {
  PredictCall f1 = f;
  f1.R = 1;
  f1.J = 1;                                     // k_predict's limits on the shape; the LDS is this kernel's own, below
  std::string bad = predict_check(c, f1, nullptr);
  if (!bad.empty()) return bad.replace(0, 9, "k_predict_lap");
  if (f.J < 1) return "k_predict_lap: range outside the chain storage";
  const Dims& d = c.d;
  const LapLds L = lap_lds(d.K, d.P, d.M, d.LG, std::min(f.J, 1 << 24), pred_kt(d.K));
  const size_t bytes = L.total * sizeof(double);
  if (lds_bytes) *lds_bytes = bytes;
  if (bytes > PR_LDS_HARD || f.J > (1 << 24))
    return "k_predict_lap: the tables of a draw (Gamma of " + std::to_string(L.p.AP) + " x " + std::to_string(L.p.AP) + " for K (n_eigen + 1) = " +
           std::to_string(L.p.A) + " directions), the scratch of the K + 1 = " + std::to_string(d.K + 1) + " starts of the mode search (" +
           std::to_string(L.SS) + " doubles each) and the " + std::to_string((long long)f.J) + " x (K + 1) values of the samples need " +
           (f.J > (1 << 24) ? std::string("more than 1073741824") : std::to_string(bytes)) + " bytes of LDS, above the limit of " +
           std::to_string(PR_LDS_HARD) + " (160 KiB)";
  return "";
}

int predict_lap_comp_doubles(int K) { return (K - 1) + (K - 1) * K / 2 + 2; }

std::string launch_predict_lap(const Ctx& c, const PredictCall& f, int r0, int rows, double* lpd_t, double* ess_t, double* m_t, double* q_t,
                               int32_t* n_modes, double* comps, double* eta, hipStream_t st) {
  size_t lds = 0;
  const std::string bad = predict_lap_check(c, f, &lds);
  if (!bad.empty()) return bad;
  if (rows < 1 || r0 < 0 || (long long)r0 + rows > f.n_new) return "k_predict_lap: curves outside the call";
  if (!m_t != !q_t) return "k_predict_lap: m_t and q_t go together";
  if (!n_modes || !lpd_t || !ess_t || f.zs) return "k_predict_lap: bad arguments";
  PredictCall f1 = f;
  f1.R = 1;
  const PredArgs a = pred_args(c, f1, r0, rows, lpd_t, ess_t, m_t, q_t, nullptr, nullptr);
  LapOut out;
  out.n_modes = n_modes; out.comps = comps; out.eta = eta;
  const dim3 grid((unsigned)rows, (unsigned)((f.n_slots + a.SCH - 1) / a.SCH), (unsigned)c.nch);
  void (*fn)(PredArgs, LapOut) = pred_kt(c.d.K) == 4 ? k_predict_lap<4> : k_predict_lap<KMAX>;
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_predict_lap: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, grid, dim3(PR_NT), lds, st, a, out);
  if (hipGetLastError() != hipSuccess) return "k_predict_lap: launch failed";
  return "";
}

}  // namespace bfmmm
