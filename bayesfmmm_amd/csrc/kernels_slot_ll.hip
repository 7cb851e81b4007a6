// Log-likelihood of chain slots given the scores: for every chain q, slot t and curve i
//     theta_i = sum_k Z_ik (nu_k + eta_k x_i) + sum_m chi_im sum_k Z_ik (phi_km + xi_km x_i),
//     rss_i   = yy_i - 2 theta_i's_i + theta_i'G_i theta_i,
// from the resident record alone, and loglik(q, t) from sum_i rss_i by the closed form of k_loglik (kernels_sweep.hip).  It is what
// the sweep stores in the "loglik" slots, recomputed from the slots: for chains that were loaded (bfmmm_set_chain), and as a check of
// the stored array for chains the sampler ran itself.
//
// k_slot_rss is a sibling of k_chain_curve_ll (kernels_curve_ll.hip) and has its geometry: a group of LPC lanes (32 for P <= 32,
// else 64) owns ONE curve for the whole launch, lane p keeps row p of the band of G_i and s_i[p] in registers (spline degrees; wider
// bands keep the record's G part in LDS).  A workgroup of NG = 256 / LPC groups takes NG consecutive curves, one chain and a run of
// slots, and stages TB draws at a time in LDS: the draw's parameters transposed to direction-major, the groups' Z_i. and chi_i..
//   (1) lane p: theta[p] -> the group's one row (zero padded by BW on both sides)
//   (2) lane p: g[p] = (G theta)[p] over the band window, u[p] = theta[p] (g[p] - 2 s_i[p])
//   (3) rss = yy_i + sum_p u[p], a butterfly over the group's lanes in a fixed order; lane g keeps draw g's
// and after the TB draws lane g stores rss of draw g: draw fastest, one coalesced store.  One quadratic form where k_chain_curve_ll
// has 1 + M + M (M + 1) / 2, and no Cholesky.
// k_slot_ll_reduce: one thread a (chain, slot) adds the chunk's rows to the call's accumulator in curve order (reads coalesced along
// the draws); where the per-curve values are asked for it replaces rss_i by l_i in place; the last chunk applies the closed form.
// fp64, every sum in a fixed order that depends on (curve, chain, slot) only, no atomics: the bits do not depend on the chunk, the
// grid or TB.
#include "model.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

constexpr int SLL_NT = 256;
constexpr int SLL_TB_MAX = 16;                 // draws staged together (<= LPC: lane g keeps draw g's sum)
constexpr int SLL_UN = 4;                      // independent loads per thread of a staging pass
constexpr size_t SLL_LDS_SOFT = 64 * 1024;     // two workgroups per CU where the shape allows
constexpr size_t SLL_LDS_HARD = 160 * 1024;

struct SllArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Z, *c_chi, *c_nu, *c_Phi, *c_eta, *c_xi;
  const double *rec, *X;
  double* out;
  size_t chain_bytes, chain_bytes_cov;
  int n, K, P, M, D, BW, LG, LREC, cadj;
  int C, first_slot, S, i0, rows;
  int TB, SCH;                                 // draws per staged batch, slots per workgroup (a multiple of TB)
};

// LDS doubles of k_slot_rss (`rec_lds`: the G part of the groups' records is staged)
struct SllLds {
  int NTH, NTX, RS, ZS, MS, NG;
  size_t th, thx, z, chi, rows, x, recs, total;
};
__host__ __device__ inline SllLds sll_lds(int K, int P, int M, int D, int BW, int LG, int LPC, int TB, bool rec_lds) {
  SllLds L;
  L.NG = SLL_NT / LPC;
  L.NTH = K * (M + 1) * P;
  L.NTX = L.NTH * D;
  L.RS = (P + 2 * BW) | 1;
  L.ZS = K | 1;
  L.MS = M | 1;
  size_t o = 0;
  L.th = o; o += (size_t)TB * L.NTH;
  L.thx = o; o += (size_t)TB * L.NTX;
  L.z = o; o += (size_t)TB * L.NG * L.ZS;
  L.chi = o; o += (size_t)TB * L.NG * L.MS;
  L.rows = o; o += (size_t)L.NG * L.RS;
  L.x = o; o += (size_t)L.NG * 8;
  L.recs = o; o += rec_lds ? (size_t)L.NG * LG : 0;
  L.total = o;
  return L;
}

// Batched global -> LDS pass with an index map (copy_to_lds with a transposing destination): every thread issues SLL_UN
// independent loads before its first store.
template <typename Map>
__device__ inline void sll_stage(double* dst, const double* __restrict__ src, int count, int tid, Map map) {
  for (int base = 0; base < count; base += SLL_NT * SLL_UN) {
    double v[SLL_UN];
#pragma unroll
    for (int u = 0; u < SLL_UN; ++u) v[u] = src[min(base + tid + SLL_NT * u, count - 1)];
#pragma unroll
    for (int u = 0; u < SLL_UN; ++u) {
      const int idx = base + tid + SLL_NT * u;
      if (idx < count) dst[map(idx)] = v[u];
    }
  }
}

// BWT >= 0: the band half-width, row p of G_i's band in 2 BWT + 1 registers; BWT < 0: band a.BW, the G part in LDS
template <int BWT, int LPC>
__global__ __launch_bounds__(SLL_NT) void k_slot_rss(SllArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool REC_LDS = BWT < 0;
  const int tid = threadIdx.x, lp = tid % LPC, grp = tid / LPC;
  const int K = a.K, P = a.P, M = a.M, D = a.D, M1 = M + 1, n = a.n;
  const int BW = REC_LDS ? a.BW : BWT;
  const int TB = a.TB;
  const SllLds L = sll_lds(K, P, M, D, BW, a.LG, LPC, TB, REC_LDS);
  const int NG = L.NG, NTH = L.NTH, NTX = L.NTX, RS = L.RS, ZS = L.ZS, MS = L.MS;
  double* sTh = sm + L.th;
  double* sThX = sm + L.thx;
  double* sZ = sm + L.z;
  double* sChi = sm + L.chi;
  double* sRow = sm + L.rows + (size_t)grp * RS;               // the group's row; entry p at [BW + p]
  double* sX = sm + L.x + (size_t)grp * 8;
  double* sRec = sm + L.recs + (REC_LDS ? (size_t)grp * a.LG : 0);

  const int tile0 = a.i0 + (int)blockIdx.x * NG;              // first curve of the workgroup
  const int i = tile0 + grp;
  const bool act = i < a.i0 + a.rows;                          // the group has a curve
  const bool lane_on = act && lp < P;
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const double* c_Z = ptr_shift(a.c_Z, (size_t)q_chain * a.chain_bytes);
  const double* c_chi = ptr_shift(a.c_chi, (size_t)q_chain * a.chain_bytes);
  const double* c_nu = ptr_shift(a.c_nu, (size_t)q_chain * a.chain_bytes);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q_chain * a.chain_bytes);
  const double* c_eta = D > 0 ? ptr_shift(a.c_eta, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  const double* c_xi = D > 0 ? ptr_shift(a.c_xi, (size_t)q_chain * a.chain_bytes_cov) : nullptr;

  // ---- once per workgroup: the zeroed row, the groups' records ----
  for (int e = lp; e < RS; e += LPC) sRow[e] = 0.0;
  const double* rec = a.rec + (size_t)(act ? i : a.i0) * a.LREC;
  double GR[REC_LDS ? 1 : 2 * BWT + 1];
  double s_p = 0.0, yy = 0.0;
  if constexpr (REC_LDS) {
    // entries G(p, p + d) beyond the last column are cleared: the window product below multiplies them by a padding zero
    for (int e = lp; e < a.LG; e += LPC) { const int d = e / P, p = e - d * P; sRec[e] = (act && p + d < P) ? rec[e] : 0.0; }
    GR[0] = 0.0;
  } else {
#pragma unroll
    for (int j = 0; j <= 2 * BWT; ++j) {
      const int d = j - BWT, p2 = lp + d;                      // G(p, p + d) = rec[|d| P + min(p, p + d)]
      const bool in = lane_on && p2 >= 0 && p2 < P;
      GR[j] = in ? rec[(d < 0 ? -d : d) * P + min(lp, p2)] : 0.0;
    }
  }
  if (lane_on) s_p = rec[a.LG + lp];
  if (act) yy = rec[a.LG + P];
  if (act && lp < D) sX[lp] = a.X[i + (size_t)n * lp];

  for (int sb = s_lo; sb < s_hi; sb += TB) {
    const int gn = min(TB, s_hi - sb);
    __syncthreads();                                           // the previous batch's readers are done (and the set-up above)
    // ---- stage the batch: parameters to direction-major [(k (M+1) + mt) P + p] (x D, d-major rows, for the covariate part) ----
    for (int g = 0; g < gn; ++g) {
      const size_t t = (size_t)(a.first_slot + sb + g);
      double* th = sTh + (size_t)g * NTH;
      sll_stage(th, c_nu + t * K * P, K * P, tid, [=](int e) { const int p = e / K, k = e - p * K; return (k * M1) * P + p; });
      sll_stage(th, c_Phi + t * K * P * M, K * P * M, tid, [=](int e) {
        const int k = e % K, r = e / K, m = r / P, p = r - m * P;
        return (k * M1 + m + 1) * P + p;
      });
      if (D > 0) {
        double* tx = sThX + (size_t)g * NTX;
        sll_stage(tx, c_eta + t * P * D * K, P * D * K, tid, [=](int e) {       // [p + P (d + D k)]
          const int p = e % P, r = e / P, k = r / D, d = r - k * D;
          return ((k * M1) * D + d) * P + p;
        });
        if (a.cadj)
          sll_stage(tx, c_xi + t * K * P * D * M, K * P * D * M, tid, [=](int e) {     // [p + P (d + D (m + M k))]
            const int p = e % P, r = e / P, d = r % D, r2 = r / D, k = r2 / M, m = r2 - k * M;
            return ((k * M1 + m + 1) * D + d) * P + p;
          });
      }
    }
    for (int e = tid; e < gn * K * NG; e += SLL_NT) {
      const int g = e / (K * NG), r = e - g * K * NG, k = r / NG, gg = r - k * NG;
      const int ii = min(tile0 + gg, a.i0 + a.rows - 1);
      sZ[((size_t)g * NG + gg) * ZS + k] = c_Z[(size_t)(a.first_slot + sb + g) * n * K + ii + (size_t)n * k];
    }
    for (int e = tid; e < gn * M * NG; e += SLL_NT) {
      const int g = e / (M * NG), r = e - g * M * NG, m = r / NG, gg = r - m * NG;
      const int ii = min(tile0 + gg, a.i0 + a.rows - 1);
      sChi[((size_t)g * NG + gg) * MS + m] = c_chi[(size_t)(a.first_slot + sb + g) * n * M + ii + (size_t)n * m];
    }
    __syncthreads();

    double mine = 0.0;                                         // lane g: rss of draw sb + g
    for (int g = 0; g < gn; ++g) {
      const double* th = sTh + (size_t)g * NTH;
      const double* tx = sThX + (size_t)g * NTX;
      const double* z = sZ + ((size_t)g * NG + grp) * ZS;
      const double* ch = sChi + ((size_t)g * NG + grp) * MS;
      // (1) theta at p: the mean part, then the M score directions in order
      double thp = 0.0;
      if (lane_on) {
        for (int mt = 0; mt < M1; ++mt) {
          const bool cov = D > 0 && (mt == 0 || a.cadj);
          double v = 0.0;
          for (int k = 0; k < K; ++k) {
            const int r = k * M1 + mt;
            double x = th[r * P + lp];
            if (cov)
              for (int d = 0; d < D; ++d) x += sX[d] * tx[(r * D + d) * P + lp];
            v += z[k] * x;
          }
          thp = mt == 0 ? v : thp + ch[mt - 1] * v;
        }
        sRow[BW + lp] = thp;
      }
      __builtin_amdgcn_wave_barrier();
      // (2) G theta at p over the band window [p - BW, p + BW]
      double u = 0.0;
      if (lane_on) {
        const double* w = sRow + lp;                           // w[j] = entry p - BW + j
        double hv = 0.0;
        if constexpr (REC_LDS) {
          for (int j = 0; j <= 2 * BW; ++j) {
            const int d = j - BW;
            hv += sRec[(d < 0 ? -d : d) * P + max(min(lp, lp + d), 0)] * w[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j <= 2 * BWT; ++j) hv += GR[j] * w[j];
        }
        u = thp * (hv - 2.0 * s_p);
      }
      __builtin_amdgcn_wave_barrier();                         // the row is rewritten by the next draw
      // (3) the group's sum; every lane takes part (lanes without a basis function add 0.0)
      const double tot = yy + group_sum<LPC>(u);
      if (lp == g) mine = tot;
    }
    if (act && lp < gn)
      a.out[(size_t)(i - a.i0) * a.C * a.S + (size_t)q_chain * a.S + (size_t)(sb + lp)] = mine;
  }
}

using SllKernel = void (*)(SllArgs);
template <int LPC>
SllKernel sll_pick(int BW) {
  switch (BW) {
    case 0: return k_slot_rss<0, LPC>;
    case 1: return k_slot_rss<1, LPC>;
    case 2: return k_slot_rss<2, LPC>;
    case 3: return k_slot_rss<3, LPC>;
    case 4: return k_slot_rss<4, LPC>;
    case 5: return k_slot_rss<5, LPC>;
    default: return k_slot_rss<-1, LPC>;
  }
}

struct SllReduce {
  const double* c_sigma;      // chain 0's sigma^2 slots
  double* c_loglik;           // chain 0's "loglik" slots (store)
  const int* ni;
  double *part, *acc;
  size_t chain_bytes;
  long long N, n_obs_total;
  int S, first_slot, i0, rows, n, P, mv;
  int first, last, per_curve, store;
};

// thread cs = q S + t: acc[cs] (+)= the chunk's rss rows in curve order; per_curve: part[r N + cs] becomes l_i; last: acc[cs]
// becomes loglik(q, t), k_loglik's expression term for term, and with store it goes to slot first_slot + t of chain q as well
__global__ __launch_bounds__(SLL_NT) void k_slot_ll_reduce(SllReduce a) {
  const long long cs = (long long)blockIdx.x * SLL_NT + threadIdx.x;
  if (cs >= a.N) return;
  const int q = (int)(cs / a.S), t = (int)(cs - (long long)q * a.S);
  const double s2 = ptr_shift(a.c_sigma, (size_t)q * a.chain_bytes)[a.first_slot + t];
  const double lg = a.mv ? (a.P / 2) * log(2 * 3.14159265358979323846 * s2) : 0.91893853320467274178 + log(sqrt(s2));
  double acc = a.first ? 0.0 : a.acc[cs];
  for (int r = 0; r < a.rows; ++r) {
    double* p = a.part + (size_t)r * a.N + cs;
    const double rss = *p;
    acc += rss;
    if (a.per_curve) *p = a.mv ? -lg - (1 / (s2 * 2)) * rss : -(double)a.ni[a.i0 + r] * lg - rss / (2.0 * s2);
  }
  if (a.last) {
    // calcLikelihoodMV: (y_obs.n_cols / 2) is an integer division, CalculateLikelihood.h:155
    acc = a.mv ? -(double)a.n * lg - (1 / (s2 * 2)) * acc : -(double)a.n_obs_total * lg - acc / (2.0 * s2);
    if (a.store) ptr_shift(a.c_loglik, (size_t)q * a.chain_bytes)[a.first_slot + t] = acc;
  }
  a.acc[cs] = acc;
}

}  // namespace

// rss_i of curves [i0, i0 + rows), every chain, slots [first_slot, first_slot + n_slots) into out (rows x C x n_slots doubles on
// the device: draw fastest, then chain, then curve), on stream st.  c: the template context of the batch (chain 0's
// pointers).  Returns "" or what the kernel cannot take.
std::string launch_slot_rss(const Ctx& c, int first_slot, int n_slots, int i0, int rows, double* out, hipStream_t st) {
  const Dims& d = c.d;
  if (d.P < 1 || d.P > PMAX) return "k_slot_rss: P outside 1 .. 64";
  if (d.M < 1 || d.M > 16) return "k_slot_rss: n_eigen outside 1 .. 16";
  if (d.K < 1 || d.K > KMAX) return "k_slot_rss: K outside 1 .. 8";
  if (d.D < 0 || d.D > 8) return "k_slot_rss: more than 8 covariates";
  if (d.BW < 0 || d.BW > BWWIDE) return "k_slot_rss: band half-width above 31";
  if (c.nch < 1 || c.nch > 65535) return "k_slot_rss: more than 65535 chains";
  if (rows < 1 || i0 < 0 || i0 + rows > d.n || n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return "k_slot_rss: range outside the chain storage";
  const int LPC = d.P <= 32 ? 32 : 64;
  const bool rec_lds = d.BW > BWMAX;
  // draws per staged batch: as many as keep the workgroup at SLL_LDS_SOFT, at least one
  int TB = SLL_TB_MAX;
  auto bytes = [&](int tb) { return sll_lds(d.K, d.P, d.M, d.D, d.BW, d.LG, LPC, tb, rec_lds).total * sizeof(double); };
  while (TB > 1 && bytes(TB) > SLL_LDS_SOFT) --TB;
  if (bytes(TB) > SLL_LDS_HARD)
    return "k_slot_rss: one draw's parameters (K (n_eigen + 1) P (1 + D) = " +
           std::to_string((long long)d.K * (d.M + 1) * d.P * (1 + d.D)) + " values) and the groups' rows exceed the kernel's on-chip staging";
  SllArgs a;
  a.c_Z = c.c_Z; a.c_chi = c.c_chi; a.c_nu = c.c_nu; a.c_Phi = c.c_Phi;
  a.c_eta = d.D > 0 ? c.c_eta : nullptr; a.c_xi = d.D > 0 ? c.c_xi : nullptr;
  a.rec = c.rec; a.X = d.D > 0 ? c.X : nullptr; a.out = out;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.n = d.n; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.BW = d.BW; a.LG = d.LG; a.LREC = d.LREC;
  a.cadj = (d.D > 0 && c.covariance_adj) ? 1 : 0;
  a.C = c.nch; a.first_slot = first_slot; a.S = n_slots; a.i0 = i0; a.rows = rows;
  a.TB = TB;
  // slots per workgroup: eight batches, more where the grid's y extent would pass 65535
  long long sch = (long long)TB * 8;
  while (((long long)n_slots + sch - 1) / sch > 65535) sch *= 2;
  a.SCH = (int)sch;
  const int NG = SLL_NT / LPC;
  const dim3 grid((unsigned)((rows + NG - 1) / NG), (unsigned)((n_slots + a.SCH - 1) / a.SCH), (unsigned)c.nch);
  const SllKernel fn = LPC == 32 ? sll_pick<32>(d.BW) : sll_pick<64>(d.BW);
  const size_t lds = bytes(TB);
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_slot_rss: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, grid, dim3(SLL_NT), lds, st, a);
  if (hipGetLastError() != hipSuccess) return "k_slot_rss: launch failed";
  return "";
}

// The chunk's rows part[r N + cs] (curves i0 .. i0 + rows, N = C n_slots) added in curve order to acc[cs], which holds the sums of
// curves [0, i0) (i0 = 0: nothing).  per_curve: the rows become l_i.  The chunk that ends at curve n leaves loglik(q, t) in acc and,
// with store, in the "loglik" slots [first_slot, first_slot + n_slots) of every chain.  Chunks must come in ascending order.
std::string launch_slot_ll_reduce(const Ctx& c, int first_slot, int n_slots, int i0, int rows, int per_curve, int store, double* part,
                                  double* acc, hipStream_t st) {
  const Dims& d = c.d;
  if (!part || !acc || rows < 1 || i0 < 0 || i0 + rows > d.n || n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T)
    return "k_slot_ll_reduce: bad arguments";
  SllReduce a;
  a.c_sigma = c.c_sigma; a.c_loglik = c.c_loglik; a.ni = c.ni; a.part = part; a.acc = acc;
  a.chain_bytes = c.chain_bytes;
  a.N = (long long)c.nch * n_slots; a.n_obs_total = d.n_obs_total;
  a.S = n_slots; a.first_slot = first_slot; a.i0 = i0; a.rows = rows; a.n = d.n; a.P = d.P; a.mv = d.mv;
  a.first = i0 == 0; a.last = i0 + rows == d.n; a.per_curve = per_curve; a.store = store;
  const long long blocks = (a.N + SLL_NT - 1) / SLL_NT;
  if (blocks > 0x7fffffffLL) return "k_slot_ll_reduce: too many draws";
  hipLaunchKernelGGL(k_slot_ll_reduce, dim3((unsigned)blocks), dim3(SLL_NT), 0, st, a);
  if (hipGetLastError() != hipSuccess) return "k_slot_ll_reduce: launch failed";
  return "";
}

}  // namespace bfmmm
