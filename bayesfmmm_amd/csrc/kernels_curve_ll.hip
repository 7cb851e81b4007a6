// Per-curve marginal log-density of chain slots: for every chain q, slot t and curve i
//     l_i(q, t) = log N( y_i ; B_i c, sigma^2 I + U U' ),  c = sum_k Z_ik (nu_k + eta_k x_i),  U = B_i [V_1 .. V_M],
//     V_m = sum_k Z_ik (phi_km + xi_km x_i),
// the density k_post_cpo (kernels_post.hip) evaluates from the observations, here from the resident record alone:
//     g = G_i c,  rr = yy_i - 2 c's_i + c'g,  u_m = V_m'(s_i - g),  W_ml = V_m'G_i V_l,  A = sigma^2 I_M + W,
//     l = -1/2 [ n_i log 2 pi + (n_i - M) log sigma^2 + log det A + (rr - u'A^-1 u) / sigma^2 ].
// Label-invariant (a sum over k) and sign-invariant (quadratic in V_m): the quantity Sampler.curve_diagnostics and
// Sampler.loo reduce.  Cost per curve-draw independent of n_i; nothing is uploaded.
//
// Geometry.  A group of LPC lanes (32 for P <= 32, else 64: one lane per basis function, as in kernels_curve.hip) owns ONE
// curve for the whole launch: lane p keeps row p of the band of G_i and s_i[p] in registers (spline degrees; bands wider
// than 5 keep the record's G part in LDS instead, so that no instance spills).  A workgroup of NG = 256 / LPC groups takes
// NG consecutive curves, one chain and a run of slots, and stages TB draws at a time in LDS (copy_to_lds-style batched
// loads): the draw's K (M + 1) P (1 + D) parameter values, transposed to direction-major, the groups' Z_i. and sigma^2.
// Neither operand is re-read per curve-draw: the record never, a draw once per NG curves.
//   (1) lane p: c[p], V_m[p] -> the group's rows (zero padded by BW on both sides)
//   (2) lane p: (G V)[p] over the band window -> rows e = s - g, t = g - 2 s, h_m = G V_m
//   (3) lane q: the q-th of the NQ = 1 + M + M (M + 1) / 2 dot products c't, V_m'e, V_m'h_l, summed over p in order
//   (4) after the TB draws, lane g: Cholesky of draw g's M x M system in its own LDS column, l, one coalesced store
// fp64, every sum in a fixed order that depends on (curve, chain, slot) only, no atomics: the bits do not depend on the
// chunk, the grid or TB.
#include "model.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <string>

namespace bfmmm {

namespace {

constexpr int CLL_NT = 256;
constexpr int CLL_TB_MAX = 16;                 // draws staged together (= most lanes busy in step 4)
constexpr int CLL_UN = 4;                      // independent loads per thread of a staging pass
constexpr size_t CLL_LDS_SOFT = 64 * 1024;     // two workgroups per CU where the shape allows
constexpr size_t CLL_LDS_HARD = 160 * 1024;

struct CllArgs {
  // chain 0's slot storage; chain q's is q * chain_bytes (covariate blocks: chain_bytes_cov) further
  const double *c_Z, *c_nu, *c_Phi, *c_sigma, *c_eta, *c_xi;
  const double *rec, *X;
  const int* ni;
  double* out;
  size_t chain_bytes, chain_bytes_cov;
  int n, K, P, M, D, BW, LG, LREC, cadj;
  int C, first_slot, S, i0, rows;
  int TB, SCH;                                 // draws per staged batch, slots per workgroup (a multiple of TB)
};

// LDS doubles (the layout of k_chain_curve_ll; `rec_lds`: the G part of the groups' records is staged)
struct CllLds {
  int NTH, NTX, NQ, NQS, RS, NROW, ZS, NG;
  size_t th, thx, z, sig, tab, rows, q, x, recs, total;
};
__host__ __device__ inline CllLds cll_lds(int K, int P, int M, int D, int BW, int LG, int LPC, int TB, bool rec_lds) {
  CllLds L;
  L.NG = CLL_NT / LPC;
  L.NTH = K * (M + 1) * P;
  L.NTX = L.NTH * D;
  L.NQ = 1 + M + M * (M + 1) / 2;
  L.NQS = L.NQ | 1;
  L.RS = (P + 2 * BW) | 1;
  L.NROW = 2 * M + 3;
  L.ZS = K | 1;
  size_t o = 0;
  L.th = o; o += (size_t)TB * L.NTH;
  L.thx = o; o += (size_t)TB * L.NTX;
  L.z = o; o += (size_t)TB * L.NG * L.ZS;
  L.sig = o; o += CLL_TB_MAX;
  L.tab = o; o += (size_t)(L.NQ + 1) / 2;                  // NQ ints
  L.rows = o; o += (size_t)L.NG * L.NROW * L.RS;
  L.q = o; o += (size_t)L.NG * TB * L.NQS;
  L.x = o; o += (size_t)L.NG * 8;
  L.recs = o; o += rec_lds ? (size_t)L.NG * LG : 0;
  L.total = o;
  return L;
}

// Batched global -> LDS pass with an index map (copy_to_lds with a transposing destination): every thread issues CLL_UN
// independent loads before its first store.
template <typename Map>
__device__ inline void stage_mapped(double* dst, const double* __restrict__ src, int count, int tid, Map map) {
  for (int base = 0; base < count; base += CLL_NT * CLL_UN) {
    double v[CLL_UN];
#pragma unroll
    for (int u = 0; u < CLL_UN; ++u) v[u] = src[min(base + tid + CLL_NT * u, count - 1)];
#pragma unroll
    for (int u = 0; u < CLL_UN; ++u) {
      const int idx = base + tid + CLL_NT * u;
      if (idx < count) dst[map(idx)] = v[u];
    }
  }
}

// BWT >= 0: the band half-width, row p of G_i's band in 2 BWT + 1 registers; BWT < 0: band a.BW, the G part in LDS
template <int BWT, int LPC>
__global__ __launch_bounds__(CLL_NT) void k_chain_curve_ll(CllArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  constexpr bool REC_LDS = BWT < 0;
  const int tid = threadIdx.x, lp = tid % LPC, grp = tid / LPC;
  const int K = a.K, P = a.P, M = a.M, D = a.D, M1 = M + 1, n = a.n;
  const int BW = REC_LDS ? a.BW : BWT;
  const int TB = a.TB;
  const CllLds L = cll_lds(K, P, M, D, BW, a.LG, LPC, TB, REC_LDS);
  const int NG = L.NG, NTH = L.NTH, NTX = L.NTX, NQ = L.NQ, NQS = L.NQS, RS = L.RS, ZS = L.ZS;
  double* sTh = sm + L.th;
  double* sThX = sm + L.thx;
  double* sZ = sm + L.z;
  double* sSig = sm + L.sig;
  int* sTab = reinterpret_cast<int*>(sm + L.tab);
  double* sRow = sm + L.rows + (size_t)grp * L.NROW * RS;     // the group's rows; entry p of a row at [BW + p]
  double* sQ = sm + L.q + (size_t)grp * TB * NQS;
  double* sX = sm + L.x + (size_t)grp * 8;
  double* sRec = sm + L.recs + (REC_LDS ? (size_t)grp * a.LG : 0);

  const int tile0 = a.i0 + (int)blockIdx.x * NG;              // first curve of the workgroup
  const int i = tile0 + grp;
  const bool act = i < a.i0 + a.rows;                          // the group has a curve
  const bool lane_on = act && lp < P;
  const int q_chain = blockIdx.z;
  const int s_lo = (int)blockIdx.y * a.SCH, s_hi = min(a.S, s_lo + a.SCH);     // slots relative to first_slot
  const double* c_Z = ptr_shift(a.c_Z, (size_t)q_chain * a.chain_bytes);
  const double* c_nu = ptr_shift(a.c_nu, (size_t)q_chain * a.chain_bytes);
  const double* c_Phi = ptr_shift(a.c_Phi, (size_t)q_chain * a.chain_bytes);
  const double* c_sigma = ptr_shift(a.c_sigma, (size_t)q_chain * a.chain_bytes);
  const double* c_eta = D > 0 ? ptr_shift(a.c_eta, (size_t)q_chain * a.chain_bytes_cov) : nullptr;
  const double* c_xi = D > 0 ? ptr_shift(a.c_xi, (size_t)q_chain * a.chain_bytes_cov) : nullptr;

  // ---- once per workgroup: the dot-product table, zeroed rows, the groups' records ----
  for (int q = tid; q < NQ; q += CLL_NT) {
    int ra, rb;
    if (q == 0) { ra = 0; rb = 2 * M + 2; }                    // c't
    else if (q <= M) { ra = q; rb = M + 1; }                   // V_m'e
    else { int m = 0, rem = q - M - 1; while (rem >= M - m) { rem -= M - m; ++m; } ra = m + 1; rb = M + 2 + m + rem; }   // V_m'h_l, m <= l
    sTab[q] = ra | (rb << 8);
  }
  for (int e = lp; e < L.NROW * RS; e += LPC) sRow[e] = 0.0;
  const double* rec = a.rec + (size_t)(act ? i : a.i0) * a.LREC;
  double GR[REC_LDS ? 1 : 2 * BWT + 1];
  double s_p = 0.0, yy = 0.0;
  int ni = 0;
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
  if (act) { yy = rec[a.LG + P]; ni = a.ni[i]; }
  if (act && lp < D) sX[lp] = a.X[i + (size_t)n * lp];

  for (int sb = s_lo; sb < s_hi; sb += TB) {
    const int gn = min(TB, s_hi - sb);
    __syncthreads();                                           // the previous batch's readers are done (and the set-up above)
    // ---- stage the batch: parameters to direction-major [(k (M+1) + mt) P + p] (x D, d-major rows, for the covariate part) ----
    for (int g = 0; g < gn; ++g) {
      const size_t t = (size_t)(a.first_slot + sb + g);
      double* th = sTh + (size_t)g * NTH;
      stage_mapped(th, c_nu + t * K * P, K * P, tid, [=](int e) { const int p = e / K, k = e - p * K; return (k * M1) * P + p; });
      stage_mapped(th, c_Phi + t * K * P * M, K * P * M, tid, [=](int e) {
        const int k = e % K, r = e / K, m = r / P, p = r - m * P;
        return (k * M1 + m + 1) * P + p;
      });
      if (D > 0) {
        double* tx = sThX + (size_t)g * NTX;
        stage_mapped(tx, c_eta + t * P * D * K, P * D * K, tid, [=](int e) {       // [p + P (d + D k)]
          const int p = e % P, r = e / P, k = r / D, d = r - k * D;
          return ((k * M1) * D + d) * P + p;
        });
        if (a.cadj)
          stage_mapped(tx, c_xi + t * K * P * D * M, K * P * D * M, tid, [=](int e) {     // [p + P (d + D (m + M k))]
            const int p = e % P, r = e / P, d = r % D, r2 = r / D, k = r2 / M, m = r2 - k * M;
            return ((k * M1 + m + 1) * D + d) * P + p;
          });
      }
    }
    for (int e = tid; e < gn * K * NG; e += CLL_NT) {
      const int g = e / (K * NG), r = e - g * K * NG, k = r / NG, gg = r - k * NG;
      const int ii = min(tile0 + gg, a.i0 + a.rows - 1);
      sZ[((size_t)g * NG + gg) * ZS + k] = c_Z[(size_t)(a.first_slot + sb + g) * n * K + ii + (size_t)n * k];
    }
    if (tid < gn) sSig[tid] = c_sigma[a.first_slot + sb + tid];
    __syncthreads();

    for (int g = 0; g < gn; ++g) {
      const double* th = sTh + (size_t)g * NTH;
      const double* tx = sThX + (size_t)g * NTX;
      const double* z = sZ + ((size_t)g * NG + grp) * ZS;
      // (1) c and V_m at p
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
          sRow[mt * RS + BW + lp] = v;
        }
      }
      __builtin_amdgcn_wave_barrier();
      // (2) G times each of them at p, over the band window [p - BW, p + BW]
      if (lane_on) {
        for (int mt = 0; mt < M1; ++mt) {
          const double* w = sRow + mt * RS + lp;               // w[j] = entry p - BW + j
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
          if (mt == 0) {
            sRow[(M + 1) * RS + BW + lp] = s_p - hv;
            sRow[(2 * M + 2) * RS + BW + lp] = hv - 2.0 * s_p;
          } else {
            sRow[(M + 1 + mt) * RS + BW + lp] = hv;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      // (3) the dot products, one per lane and pass, p in order
      if (act) {
        for (int q = lp; q < NQ; q += LPC) {
          const int tb = sTab[q];
          const double* ra = sRow + (tb & 255) * RS + BW;
          const double* rb = sRow + (tb >> 8) * RS + BW;
          double s_ = 0.0;
          for (int p = 0; p < P; ++p) s_ += ra[p] * rb[p];
          sQ[(size_t)g * NQS + q] = s_;
        }
      }
      __builtin_amdgcn_wave_barrier();                         // the rows are rewritten by the next draw
    }
    // (4) lane g: the M x M system of draw g, factorised in place in the draw's own column (packed upper triangle: entry
    //     (m, l), m <= l, at M + 1 + tri_index(M, m, l); L(l, m) overwrites it)
    if (act && lp < gn) {
      double* Q = sQ + (size_t)lp * NQS;
      double* b = Q + 1;
      double* A = Q + M + 1;
      const double sig = sSig[lp];
      const double rr = yy + Q[0];
      double logdet = 0.0, ww = 0.0;
      for (int c = 0; c < M; ++c) {
        double dg = A[tri_index(M, c, c)] + sig;
        for (int k2 = 0; k2 < c; ++k2) { const double l2 = A[tri_index(M, k2, c)]; dg -= l2 * l2; }
        const double l = sqrt(dg);
        double wv = b[c];
        for (int k2 = 0; k2 < c; ++k2) wv -= A[tri_index(M, k2, c)] * b[k2];
        wv /= l;
        b[c] = wv;
        logdet += 2.0 * log(l);
        ww += wv * wv;
        for (int r3 = c + 1; r3 < M; ++r3) {
          double v = A[tri_index(M, c, r3)];
          for (int k2 = 0; k2 < c; ++k2) v -= A[tri_index(M, k2, r3)] * A[tri_index(M, k2, c)];
          A[tri_index(M, c, r3)] = v / l;
        }
      }
      const double ld = (double)(ni - M) * log(sig) + logdet;
      const double quad = (rr - ww) / sig;
      a.out[(size_t)(i - a.i0) * a.C * a.S + (size_t)q_chain * a.S + (size_t)(sb + lp)] =
          -(0.5 * ni) * 1.83787706640934548356 - 0.5 * ld - 0.5 * quad;
    }
  }
}

using CllKernel = void (*)(CllArgs);
template <int LPC>
CllKernel cll_pick(int BW) {
  switch (BW) {
    case 0: return k_chain_curve_ll<0, LPC>;
    case 1: return k_chain_curve_ll<1, LPC>;
    case 2: return k_chain_curve_ll<2, LPC>;
    case 3: return k_chain_curve_ll<3, LPC>;
    case 4: return k_chain_curve_ll<4, LPC>;
    case 5: return k_chain_curve_ll<5, LPC>;
    default: return k_chain_curve_ll<-1, LPC>;
  }
}

}  // namespace

// l of curves [i0, i0 + rows), every chain, slots [first_slot, first_slot + n_slots) into out (rows x C x n_slots doubles on
// the device: draw fastest, then chain, then curve), on stream st.  c: the template context of the batch (chain 0's
// pointers).  Returns "" or what the kernel cannot take.
std::string launch_chain_curve_ll(const Ctx& c, int first_slot, int n_slots, int i0, int rows, double* out, hipStream_t st) {
  const Dims& d = c.d;
  if (d.P < 1 || d.P > PMAX) return "k_chain_curve_ll: P outside 1 .. 64";
  if (d.M < 1 || d.M > 16) return "k_chain_curve_ll: n_eigen outside 1 .. 16";
  if (d.K < 1 || d.K > KMAX) return "k_chain_curve_ll: K outside 1 .. 8";
  if (d.D < 0 || d.D > 8) return "k_chain_curve_ll: more than 8 covariates";
  if (d.BW < 0 || d.BW > BWWIDE) return "k_chain_curve_ll: band half-width above 31";
  if (c.nch < 1 || c.nch > 65535) return "k_chain_curve_ll: more than 65535 chains";
  if (rows < 1 || i0 < 0 || i0 + rows > d.n || n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return "k_chain_curve_ll: range outside the chain storage";
  const int LPC = d.P <= 32 ? 32 : 64;
  const bool rec_lds = d.BW > BWMAX;
  // draws per staged batch: as many as keep the workgroup at CLL_LDS_SOFT, at least one
  int TB = CLL_TB_MAX;
  auto bytes = [&](int tb) { return cll_lds(d.K, d.P, d.M, d.D, d.BW, d.LG, LPC, tb, rec_lds).total * sizeof(double); };
  while (TB > 1 && bytes(TB) > CLL_LDS_SOFT) --TB;
  if (bytes(TB) > CLL_LDS_HARD)
    return "k_chain_curve_ll: one draw's parameters (K (n_eigen + 1) P (1 + D) = " +
           std::to_string((long long)d.K * (d.M + 1) * d.P * (1 + d.D)) + " values) and the groups' rows exceed the kernel's on-chip staging";
  CllArgs a;
  a.c_Z = c.c_Z; a.c_nu = c.c_nu; a.c_Phi = c.c_Phi; a.c_sigma = c.c_sigma;
  a.c_eta = d.D > 0 ? c.c_eta : nullptr; a.c_xi = d.D > 0 ? c.c_xi : nullptr;
  a.rec = c.rec; a.X = d.D > 0 ? c.X : nullptr; a.ni = c.ni; a.out = out;
  a.chain_bytes = c.chain_bytes; a.chain_bytes_cov = c.chain_bytes_cov;
  a.n = d.n; a.K = d.K; a.P = d.P; a.M = d.M; a.D = d.D; a.BW = d.BW; a.LG = d.LG; a.LREC = d.LREC;
  a.cadj = (d.D > 0 && c.covariance_adj) ? 1 : 0;
  a.C = c.nch; a.first_slot = first_slot; a.S = n_slots; a.i0 = i0; a.rows = rows;
  a.TB = TB;
  // slots per workgroup: eight batches, more where the grid's y extent would pass 65535
  long long sch = (long long)TB * 8;
  while (((long long)n_slots + sch - 1) / sch > 65535) sch *= 2;
  a.SCH = (int)sch;
  const int NG = CLL_NT / LPC;
  const dim3 grid((unsigned)((rows + NG - 1) / NG), (unsigned)((n_slots + a.SCH - 1) / a.SCH), (unsigned)c.nch);
  const CllKernel fn = LPC == 32 ? cll_pick<32>(d.BW) : cll_pick<64>(d.BW);
  const size_t lds = bytes(TB);
  if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return "k_chain_curve_ll: cannot set the LDS size";
  }
  hipLaunchKernelGGL(fn, grid, dim3(CLL_NT), lds, st, a);
  if (hipGetLastError() != hipSuccess) return "k_chain_curve_ll: launch failed";
  return "";
}

}  // namespace bfmmm
