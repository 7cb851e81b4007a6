// The pair-Gram contraction of the Phi / nu block (fp64 MFMA) and its reductions.
//
// Every Gaussian full conditional of the block (kernels_sweep.hip) needs  H_ab = sum_i w_ai w_bi G_i  and  t_a = sum_i w_ai s_i.
// Z and chi do not change between the Phi and nu blocks of a sweep, so ONE pass over the per-curve records yields every H_ab and
// t_a of the iteration.
//
//   k_pair_gram      : [R pair weights x n] * [n x LG record columns] -> v_mfma_f64_16x16x4_f64, split-K; the general body
//                      (one chain, or a loop over the chains of a batch) and the single-chain bodies pg_solo_g / pg_solo_s
//                      (pi / alpha_3, the deferred delta / A / gamma / tau job and the deferred log-likelihood ride as extra
//                      workgroups: scalar_jobs.hpp)
//   k_pg_reduce      : fixed-order sum of the split-K partial tiles -> H (R x LG), H2, t (A x P)
//   k_pair_gram_pack : the contraction of chain batches and long curve sets: row tiles packed across the chains, chunked k-loop
//   k_pg_reduce_pack : its reduction, in k_pg_reduce's order
//   host             : pg_geometry, pg_route_decide -- the one decision of which of these a (sub-)batch runs and with what
//                      geometry -- and the launchers, which launch what the route says
#include "model.hpp"
#include "scalar_jobs.hpp"
#include "sweep_helpers.hpp"
#include "launchers.hpp"

#include <algorithm>

namespace bfmmm {

// ---------------------------------------------------------------------------------------------
// pair-Gram
// ---------------------------------------------------------------------------------------------
// grid = (CTG + 2, NKS); block = 256 (4 waves).  Workgroup (ct, ks) owns the 16 record columns
// [16 ct, 16 ct + 16) of the G part for the KS curves of k-slice ks: it stages them once in LDS
// (coalesced 128-byte segments) and its four waves walk the RT row tiles of pair weights, each
// wave issuing one v_mfma_f64_16x16x4_f64 per 4 curves and row tile; the weights w_ai w_bi are
// rebuilt on the fly from Z and chi (also staged in LDS).  Workgroup (CTG, ks) does the same for the
// single-weight rows against the s part of the records (t_a = sum_i w_ai s_i).
//
// LDS per curve i:  raw row  sW = [ Z_i1 .. Z_iK | 1, chi_i1 .. chi_iM | 0 ]  and, for the G workgroups,
// the pair row  sP = [ Z_ij Z_ij' (j <= j') | chit_im chit_im' (m <= m') | 0 ].  Every MFMA weight is then the
// branch-free product of two LDS entries (padding rows point at the 0 slot), so the inner loop has
// no divergence and the TPW accumulators of a wave stay in flight together.
#ifdef BFMMM_TIMELINE
__device__ unsigned long long g_wgtrace[3 * 1024];
void fetch_wgtrace(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgtrace), sizeof(unsigned long long) * 3 * 1024); }
#endif

constexpr int PG_THREADS = 512;   // 8 waves, two per SIMD: a wave's LDS reads and weight products issue while the other wave's MFMAs execute
                                  // (within one wave MFMA, VALU and LDS issue strictly in order: tools/ubench_mfma.hip)

// Single-chain body of the G workgroups of k_pair_gram (k_pair_gram<false, false> launched with do_pg == PG_SOLO).  Same
// output and the same canonical summation order as the general body below (and as k_pair_gram_pack), three differences:
//  * the pair rows are formed at staging, from the registers that load a curve's Z and chi (thread il owns curve il of the
//    slice), and stored with them: no LDS re-read of the raw rows and no second barrier (the general body spends 1.7 us there);
//  * a wave runs exactly its row tiles wave, wave + 8, .. (1 .. PGS_TMAX, scalar count): the general body issues TPW = 2
//    MFMA chains per wave whether or not the second tile exists, so every SIMD ran four 44-step chains at config 2 where
//    three suffice (row tiles of SIMD s: s, s + 4, s + 8, ..: 3/3/3/2 for 11 tiles);
//  * the B operand (one record column per lane, the same for every tile of the workgroup) is read once per step pair for all
//    tiles of the wave, and the k-loop stops at the last live 16-curve chunk of a partial slice.
// Limits (otherwise the general body): functional model, no covariates, K <= 4, M <= 8, P <= 32, LG <= 128, KS <= 256.
constexpr int PG_SOLO = 2;                 // do_pg flag that selects it
constexpr int PGS_TMAX = 4;                // row tiles per wave: RT <= 32
constexpr int PGS_KS = 256;                // curves per k-slice: one weight-loading thread per curve, 8 record loads per thread

inline bool pg_solo_fits(const Dims& d, int KS) {
  return !d.mv && d.D == 0 && d.K <= 4 && d.MD - 1 <= 8 && d.P <= 32 && d.LG <= 128 && KS <= PGS_KS &&
         d.RT <= PGS_TMAX * (PG_THREADS / 64);
}

// Z and chi of curve iw into registers (zero beyond K and M, and for a thread without a live curve): the first global loads of
// both single-chain bodies
__device__ __forceinline__ void pg_solo_load_zx(const Ctx& c0, bool wl, int iw, double (&z)[4], double (&x)[8]) {
  const int n = c0.d.n, K = c0.d.K, MD = c0.d.MD;
#pragma unroll
  for (int a = 0; a < 4; ++a) z[a] = (wl && a < K) ? c0.Z[iw + (size_t)n * a] : 0.0;
#pragma unroll
  for (int m = 0; m < 8; ++m) x[m] = (wl && m < MD - 1) ? c0.chi[iw + (size_t)n * m] : 0.0;
}

template <int NTL>
__device__ inline void pg_solo_tiles(const double* sP, const double* sB, int KSP, int KQ, int nchunk, const int (&o1)[PGS_TMAX],
                                     const int (&o2)[PGS_TMAX], int lr, int kq, double4_t (&acc)[PGS_TMAX]) {
  const v2d* pa[NTL]; const v2d* pb[NTL];
#pragma unroll
  for (int q = 0; q < NTL; ++q) {
    pa[q] = (const v2d*)(sP + o1[q] * KSP + kq * KQ);
    pb[q] = (const v2d*)(sP + o2[q] * KSP + kq * KQ);
  }
  const v2d* pc = (const v2d*)(sB + lr * KSP + kq * KQ);
  // chunk t = steps 4 t .. 4 t + 3 = v2d entries 2 t, 2 t + 1 of every row; the operands of chunk t + 1 are read into the other
  // set before the MFMAs of chunk t issue (as in the general body)
  struct Ops { v2d a[2][NTL], b[2][NTL], c[2]; };
  auto load = [&](Ops& o, int t) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      o.c[u] = pc[2 * t + u];
#pragma unroll
      for (int q = 0; q < NTL; ++q) { o.a[u][q] = pa[q][2 * t + u]; o.b[u][q] = pb[q][2 * t + u]; }
    }
  };
  auto mfma = [&](const Ops& o) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < NTL; ++q) {
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[u][q].x * o.b[u][q].x, o.c[u].x, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[u][q].y * o.b[u][q].y, o.c[u].y, acc[q], 0, 0, 0);
      }
  };
  Ops s0, s1;
  load(s0, 0);
  for (int t = 0; t < nchunk; t += 2) {
    if (t + 1 < nchunk) load(s1, t + 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma(s0);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nchunk) load(s0, t + 2);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nchunk) mfma(s1);
    __builtin_amdgcn_sched_barrier(0);
  }
}

__device__ inline void pg_solo_g(const Ctx& c0, int KS, int ks, int ct, double* smem) {
  const Dims& d = c0.d;
  const int n = d.n, K = d.K, MD = d.MD, tid = threadIdx.x;
#ifdef BFMMM_TIMELINE
  struct { Dyn* dyn; } c = {c0.dyn};
#endif
  TSTAMP0(c, 40);
  const int i0 = ks * KS;
  const int nlive = min(KS, n - i0);
  const int nchunk = (nlive + 15) >> 4;
  const int nst = nchunk * 16;               // curves staged: the live ones and the zero tail of the last chunk
  const int KSP = KS + 2, KQ = KS >> 2;      // the general body's layout: curve il at position (il & 3) KS/4 + (il >> 2)
  const int NZZ = d.NZZ, NP = NZZ + d.NCC;
  double* sB = smem;                         // 16 x KSP  record columns
  double* sP = sB + 16 * KSP;                // (NP + 1) x KSP  pair rows, row NP = 0 (padding rows of the last tile)
  // ---- every global load of the slice first: Z / chi of curve tid, the record entries of (curve tid / 16 + 32 u, column tid % 16)
  const bool wl = tid < nlive;
  const int iw = i0 + tid;
  double z[4], x[8];
  pg_solo_load_zx(c0, wl, iw, z, x);
  const int ccg = tid & 15, ilg = tid >> 4;
  const bool colok = ct * 16 + ccg < d.LG;
  const double* srcg = c0.rec + (size_t)i0 * d.LREC + min(ct * 16 + ccg, d.LREC - 1);
  double vb[PGS_KS / 32];
#pragma unroll
  for (int u = 0; u < PGS_KS / 32; ++u) {
    const int il = ilg + 32 * u;
    vb[u] = (il < nlive && colok) ? srcg[(size_t)il * d.LREC] : 0.0;
  }
  TSTAMP0(c, 47);
  // ---- pair rows of curve tid from registers: Z_a Z_b (a <= b), then chit_a chit_b (a <= b; chit_0 = 1), the order of the
  //      general body's pair table; each entry is the same product of two raw weights
  if (tid < nst) {
    double* dst = sP + (tid & 3) * KQ + (tid >> 2);
    int e = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b)
        if (b < K) { dst[e * KSP] = z[a] * z[b]; ++e; }
    const double xt[9] = {1.0, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]};
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
      for (int b = a; b < 9; ++b)
        if (b < MD) { dst[e * KSP] = xt[a] * xt[b]; ++e; }
    dst[NP * KSP] = 0.0;
  }
#pragma unroll
  for (int u = 0; u < PGS_KS / 32; ++u) {
    const int il = ilg + 32 * u;
    if (il < nst) sB[ccg * KSP + (il & 3) * KQ + (il >> 2)] = vb[u];
  }
  TSTAMP0(c, 41);
  lds_barrier();
  TSTAMP0(c, 42);
  // ---- MFMA phase: wave w owns row tiles w, w + 8, ..
  constexpr int NW = PG_THREADS / 64;
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int ntl = __builtin_amdgcn_readfirstlane(max(0, min(PGS_TMAX, (d.RT - wave + NW - 1) / NW)));
  int o1[PGS_TMAX], o2[PGS_TMAX];
#pragma unroll
  for (int q = 0; q < PGS_TMAX; ++q) {
    const int row = (wave + NW * q) * 16 + lr;
    o1[q] = o2[q] = NP;
    if (q < ntl && row < d.R) { const int zz = row / d.NCC; o1[q] = zz; o2[q] = NZZ + (row - zz * d.NCC); }
  }
  double4_t acc[PGS_TMAX];
#pragma unroll
  for (int q = 0; q < PGS_TMAX; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  switch (ntl) {
    case 1: pg_solo_tiles<1>(sP, sB, KSP, KQ, nchunk, o1, o2, lr, kq, acc); break;
    case 2: pg_solo_tiles<2>(sP, sB, KSP, KQ, nchunk, o1, o2, lr, kq, acc); break;
    case 3: pg_solo_tiles<3>(sP, sB, KSP, KQ, nchunk, o1, o2, lr, kq, acc); break;
    case 4: pg_solo_tiles<4>(sP, sB, KSP, KQ, nchunk, o1, o2, lr, kq, acc); break;
    default: break;
  }
  // partial tiles: the general body's layout and streaming stores
#pragma unroll
  for (int q = 0; q < PGS_TMAX; ++q)
    if (q < ntl) {
      double* out = c0.pg_part + ((size_t)ks * d.NT + (size_t)(wave + NW * q) * d.CTG + ct) * 256 + lane;
      __builtin_nontemporal_store(acc[q][0], out); __builtin_nontemporal_store(acc[q][1], out + 64);
      __builtin_nontemporal_store(acc[q][2], out + 128); __builtin_nontemporal_store(acc[q][3], out + 192);
    }
  TSTAMP0(c, 44);
}

// Single-chain body of the s-part workgroup (ct == CTG) of the same launch, beside pg_solo_g (do_pg carries PG_SOLO_S;
// bfmmm_set_solo_pair_gram_tail(0) keeps the general body).  Same output slots and the same canonical summation order:
//  * one round of global loads per thread, all issued before the first LDS store: Z and chi of curve tid, and the CTS 16
//    columns of s_i (record offset LG) of the slice's live curves, element (il, cc) = (tid / ncol + (512 / ncol) u, tid % ncol)
//    with ncol = 16 or 32 (shifts and constant offsets; the general body divides per element and runs two serial rounds);
//  * the single-weight rows Z_j chit_m are formed from the loading registers and stored once -- the same product of the same
//    two raw weights the general body forms at MFMA time, so the A operand is bit-identical; one barrier;
//  * each of the AT CTS tiles gets one wave and one MFMA chain (the general body issues TPW = 2 chains per wave although
//    there are at most 6 tiles for 8 waves) that stops at the last live 16-curve chunk; waves without a tile leave.
// Limits: pg_solo_fits, hence CTS <= 2 and A <= 36 (AT CTS <= 6 tiles).
constexpr int PG_SOLO_S = 4;               // do_pg flag (with PG_SOLO): the s-part workgroup runs pg_solo_s
constexpr int PG_SOLO_LL = 8;              // do_pg flag (with PG_SOLO): the deferred log-likelihood has an extra workgroup of its own
constexpr int PGS_SU = PGS_KS / (PG_THREADS / 32);      // s_i entries per thread (32 columns; 16 columns use the first half)

__device__ inline void pg_solo_s(const Ctx& c0, int KS, int ks, double* smem) {
  const Dims& d = c0.d;
  const int n = d.n, K = d.K, MD = d.MD, tid = threadIdx.x;
  const int i0 = ks * KS;
  const int nlive = min(KS, n - i0);
  const int nchunk = (nlive + 15) >> 4;
  const int nst = nchunk * 16;               // curves staged: the live ones and the zero tail of the last chunk
  const int KSP = KS + 2, KQ = KS >> 2;      // the general body's layout: curve il at position (il & 3) KS/4 + (il >> 2)
  const int ncol = d.CTS * 16;               // 16 or 32
  double* sB = smem;                         // ncol x KSP  columns of s_i
  double* sS = sB + ncol * KSP;              // (A + 1) x KSP  single-weight rows, row A = 0 (padding rows of the last row tile)
  // ---- every global load of the slice first
  const bool wl = tid < nlive;
  const int iw = i0 + tid;
  double z[4], x[8];
  pg_solo_load_zx(c0, wl, iw, z, x);
  const int sh = (d.CTS == 1) ? 4 : 5;
  const int cc = tid & (ncol - 1), ilg = tid >> sh, ilstep = PG_THREADS >> sh;
  const bool colok = cc < d.P;
  const double* src = c0.rec + (size_t)i0 * d.LREC + min(d.LG + cc, d.LREC - 1);
  double vb[PGS_SU];
#pragma unroll
  for (int u = 0; u < PGS_SU; ++u) {
    const int il = ilg + ilstep * u;
    vb[u] = (il < nlive && colok) ? src[(size_t)il * d.LREC] : 0.0;
  }
  // ---- single-weight rows of curve tid from registers: row j MD + m = Z_j chit_m (chit_0 = 1), the general body's product
  if (tid < nst) {
    double* dst = sS + (tid & 3) * KQ + (tid >> 2);
    const double xt[9] = {1.0, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int m = 0; m < 9; ++m)
        if (a < K && m < MD) dst[(a * MD + m) * KSP] = z[a] * xt[m];
    dst[d.A * KSP] = 0.0;
  }
#pragma unroll
  for (int u = 0; u < PGS_SU; ++u) {
    const int il = ilg + ilstep * u;
    if (il < nst) sB[cc * KSP + (il & 3) * KQ + (il >> 2)] = vb[u];
  }
  lds_barrier();
  // ---- MFMA phase: wave w owns tile w = (row tile w / CTS, column tile w % CTS)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  if (wave >= d.AT * d.CTS) return;
  const int at = wave / d.CTS, cs = wave - at * d.CTS;
  const int row = at * 16 + lr;
  const v2d* pa = (const v2d*)(sS + (row < d.A ? row : d.A) * KSP + kq * KQ);
  const v2d* pc = (const v2d*)(sB + (cs * 16 + lr) * KSP + kq * KQ);
  // chunk t = steps 4 t .. 4 t + 3 = v2d entries 2 t, 2 t + 1 of the two rows, double-buffered as in pg_solo_tiles
  struct Ops { v2d a[2], c[2]; };
  auto load = [&](Ops& o, int t) { o.a[0] = pa[2 * t]; o.c[0] = pc[2 * t]; o.a[1] = pa[2 * t + 1]; o.c[1] = pc[2 * t + 1]; };
  double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
  auto mfma = [&](const Ops& o) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[u].x, o.c[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[u].y, o.c[u].y, acc, 0, 0, 0);
    }
  };
  Ops s0, s1;
  load(s0, 0);
  for (int t = 0; t < nchunk; t += 2) {
    if (t + 1 < nchunk) load(s1, t + 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma(s0);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nchunk) load(s0, t + 2);
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nchunk) mfma(s1);
    __builtin_amdgcn_sched_barrier(0);
  }
  // partial tile: the general body's slot (tix = RT CTG + tile) and streaming stores
  double* out = c0.pg_part + ((size_t)ks * d.NT + (size_t)d.RT * d.CTG + wave) * 256 + lane;
  __builtin_nontemporal_store(acc[0], out); __builtin_nontemporal_store(acc[1], out + 64);
  __builtin_nontemporal_store(acc[2], out + 128); __builtin_nontemporal_store(acc[3], out + 192);
}

template <bool BATCH, bool GROUPS>
__global__ __launch_bounds__(PG_THREADS) void k_pair_gram(Ctx c0, int KS, int nks, int do_pg, int G) {
  // Chain batches (BATCH): the workgroup stages its record columns ONCE and walks the chains of the batch in groups of G
  // (the records are shared; Z / chi, the pair weights and the output tiles are per chain), so the grid has no chain
  // dimension.  The weights of a whole group are requested together (one memory round trip per group, not per chain) and
  // its (chain, row tile) items are dealt to the eight waves together: in the Nu_Z stage a chain has ONE row tile, and a
  // group of eight chains keeps all eight waves on the matrix cores.
  // The single-chain instantiation is the same code without the loop (and without the registers it keeps alive).
  const int nch = BATCH ? c0.nch : 1;
  TIMELINE(c0, 1);
#ifdef BFMMM_TIMELINE
  const int wgid = blockIdx.x + gridDim.x * blockIdx.y;
  if (threadIdx.x == 0 && wgid < 1024) {
    unsigned id, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    g_wgtrace[3 * wgid] = wall_clock64();
    g_wgtrace[3 * wgid + 1] = ((unsigned long long)(id & 0xf) << 32) | hw;
  }
  struct EndTrace { int w; __device__ ~EndTrace() { if (threadIdx.x == 0 && w < 1024) g_wgtrace[3 * w + 2] = wall_clock64(); } } et_{wgid};
#endif
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Dims& d = c0.d;
  const int n = d.n, K = d.K, MD = d.MD;
  const int ks = blockIdx.y, ct = blockIdx.x;
  if (ct == d.CTG + 1) {            // extra workgroups: pi / alpha_3 of chain ks, hidden under the contraction
    if (ks < nch && threadIdx.x < 256) {      // the scalar jobs are written for 256 threads (waves 4-7 leave)
      const Ctx c = chain_ctx(c0, (unsigned)ks);
      job_pi_alpha(c, BATCH || !(do_pg & PG_SOLO_LL), c0.zrec != nullptr);      // (PG_SOLO_LL: the deferred log-likelihood runs in workgroup 2 nch below)
      TSTAMP(c, 46);
    } else if (ks >= nch && ks < 2 * nch && threadIdx.x < 256) {
      // the previous iteration's scalar job (delta, A, gamma, tau), left pending by k_curve_chi (Ctx::defer_hyper): its results are
      // first read by k_factor, two kernels on
      const Ctx c = chain_ctx(c0, (unsigned)(ks - nch));
      if (c.dyn->hyper_pending) {
        job_hyper(c, false);
        __syncthreads();
        if (threadIdx.x == 0) c.dyn->hyper_pending = 0u;
      }
    } else if (!BATCH && (do_pg & PG_SOLO_LL) && ks == 2 * nch && threadIdx.x < 256) {
      // the previous iteration's log-likelihood, in a workgroup of its own: it shares nothing with pi / alpha_3 (reads rss,
      // rss_part, sigma2, ll_slot; writes rss, loglik, ll_pending and its chain slot), so it need not run in front of them
      if (c0.dyn->ll_pending) deferred_loglik(c0, smem);
    }
    return;
  }
  if (ks >= nks) return;            // (the grid's y extent is max(k-slices, chains))
  if (!do_pg) return;
  const bool single = ct == d.CTG;
  if constexpr (!BATCH) {
    if ((do_pg & PG_SOLO) && !single) { pg_solo_g(c0, KS, ks, ct, smem); return; }
    if ((do_pg & PG_SOLO_S) && single) { pg_solo_s(c0, KS, ks, smem); return; }
  }
  const int ncol = single ? d.CTS * 16 : 16;
  const int col0 = single ? d.LG : ct * 16;
  const int colend = single ? d.LG + d.P : d.LG;
  const int i0 = ks * KS;
  const int RS = K + MD + 1, ONE = K;
  const int NP = d.NZZ + d.NCC, RP = NP + 1;
  // LDS: every quantity is stored per table row (row f of a table = the KS curves of the slice, stride KSP) with curve il of the
  // slice at POSITION pos(il) = (il & 3) KS/4 + (il >> 2): MFMA k-slot kq of step s reads position kq KS/4 + s, i.e. curve
  // 4 s + kq -- the four curves of a step are consecutive curves (the CANONICAL summation order, shared with
  // k_pair_gram_pack, whose chunks are runs of consecutive curves: a chain gives bit-identical H and t through either kernel),
  // and a lane's operands of two consecutive steps are adjacent, so one 16-byte LDS read feeds two MFMAs.
  const int KSP = KS + 2;                    // even (16-byte alignment of the rows) and 2 mod 8 (row starts spread over banks)
  const int KQ4 = KS >> 2;
  auto pos = [&](int il) { return (il & 3) * KQ4 + (il >> 2); };
  const int GG = GROUPS ? G : 1;             // chains staged together (GROUPS: its own instantiation, so that the plain chain loop keeps its registers)
  const int TB = RS + (single ? 0 : RP);     // table rows of a chain
  double* sB = smem;                         // ncol x KSP  record columns
  double* sW = sB + (size_t)ncol * KSP;      // chain g of the group at + g TB KSP:  RS x KSP  raw weights: Z_1..Z_K | 1, chi_1..chi_M | 0
  double* sP = sW + (size_t)RS * KSP;        //                                      RP x KSP  pair weights (G workgroups only)
  const int tid = threadIdx.x;
  constexpr int UW = 12, UB = 6;
  const int ncw = K + MD - 1;                // source columns: Z_1..Z_K, chi_1..chi_M
  const int nB = KS * ncol;
  // staging: a thread issues all its global loads (one curve's Z / chi entries, UB record entries)
  // before its first LDS store, so the workgroup pays about one memory round trip
  auto loadW = [&](const double* Zq, const double* chiq, int il0, int cb, double (&v)[UW]) {
    const int i = min(i0 + il0 + tid, n - 1);
#pragma unroll
    for (int u = 0; u < UW; ++u) {
      const int col = min(cb + u, ncw - 1);
      v[u] = (col < K) ? Zq[i + (size_t)n * col] : chiq[i + (size_t)n * (col - K)];
    }
  };
  auto storeW = [&](int il0, int cb, const double (&v)[UW]) {
    const int il = il0 + tid;
    if (il >= KS) return;
    const bool live = i0 + il < n;
#pragma unroll
    for (int u = 0; u < UW; ++u) {
      const int col = cb + u;
      if (col < ncw) sW[((col < K) ? col : col + 1) * KSP + pos(il)] = live ? v[u] : 0.0;
    }
    if (cb == 0) { sW[ONE * KSP + il] = 1.0; sW[(K + MD) * KSP + il] = 0.0; }      // (constant rows: any order)
  };
  auto loadB = [&](const double* stilq, int base, double (&v)[UB]) {        // s-part workgroups (ncol = CTS * 16)
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int q = min(base + tid + PG_THREADS * u, nB - 1);
      const int il = q / ncol, cc = q - il * ncol;
      const int i = min(i0 + il, n - 1), col = min(col0 + cc, d.LREC - 1);
      // covariate-adjusted models contract against s~_i = s_i - G_i o_i (k_curve_z, per chain) instead of s_i
      v[u] = (d.D > 0) ? stilq[(size_t)i * d.P + min(cc, d.P - 1)] : c0.rec[(size_t)i * d.LREC + col];
    }
  };
  auto storeB = [&](int base, const double (&v)[UB]) {
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int q = base + tid + PG_THREADS * u;
      if (q < nB) {
        const int il = q / ncol, cc = q - il * ncol;
        sB[cc * KSP + pos(il)] = (i0 + il < n && col0 + cc < colend) ? v[u] : 0.0;
      }
    }
  };
  // G workgroups (16 record columns): element (il, cc) = (tid / 16 + 32 u, tid % 16), so a load costs one
  // multiply-add and a store a constant LDS offset
  const int ccg = tid & 15, ilg = tid >> 4;
  const double* srcg = c0.rec + min(col0 + ccg, d.LREC - 1);
  const bool colok = col0 + ccg < colend;
  auto loadG = [&](int ub0, double (&v)[UB]) {
#pragma unroll
    for (int u = 0; u < UB; ++u) v[u] = srcg[(size_t)min(i0 + ilg + (PG_THREADS / 16) * (ub0 + u), n - 1) * d.LREC];
  };
  auto storeG = [&](int ub0, const double (&v)[UB]) {
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int il = ilg + (PG_THREADS / 16) * (ub0 + u);
      if (il < KS) sB[ccg * KSP + pos(il)] = (i0 + il < n && colok) ? v[u] : 0.0;
    }
  };
  // pair slot -> (a, b) table (packed upper triangles of Z x Z and chit x chit), decoded once
  int* ptab = (int*)(sW + (size_t)GG * TB * KSP);
  if (!single && tid < NP) {
    int e = tid, off = 0, dim = K;
    if (e >= d.NZZ) { e -= d.NZZ; off = K; dim = MD; }
    int a = 0;
    while (e >= dim - a) { e -= dim - a; ++a; }
    ptab[tid] = (off + a) | ((off + a + e) << 16);
  }
  const bool shared_cols = !(single && d.D > 0);     // the staged columns are the same for every chain
  for (int q = 0; q < nch; q += GG) {
    const int gc = GROUPS ? min(GG, nch - q) : 1;         // chains of this group
    // the per-chain operands (only these: a whole per-chain Ctx costs a few hundred scalar registers)
    const size_t off1 = (size_t)q * c0.chain_bytes;
    const double* Zq = ptr_shift(c0.Z, off1);
    const double* chiq = ptr_shift(c0.chi, off1);
    const double* stilq = ptr_shift(c0.stil, (size_t)q * c0.chain_bytes_cov);
#ifdef BFMMM_TIMELINE
    struct { Dyn* dyn; } c = {ptr_shift(c0.dyn, off1)};
#endif
    {
      TSTAMP0(c, 40);
      double vw[UW], vb[UB];
      const bool stage_cols = (q == 0) || !shared_cols;
      // BATCH: element e = tid + 512 u of the group's (chain, column, curve) items, curve fastest (gc ncw KS <= 512 UW)
      const int nitem = gc * ncw * KS;
      constexpr bool grp = GROUPS;
      if (grp) {
#pragma unroll
        for (int u = 0; u < UW; ++u) {
          const int e = min(tid + PG_THREADS * u, nitem - 1);
          const int ci = e / KS, il = e - ci * KS;
          const int g = ci / ncw, col = ci - g * ncw;
          const int i = min(i0 + il, n - 1);
          const size_t offg = (size_t)g * c0.chain_bytes;
          vw[u] = (col < K) ? ptr_shift(Zq, offg)[i + (size_t)n * col] : ptr_shift(chiq, offg)[i + (size_t)n * (col - K)];
        }
      } else {
        loadW(Zq, chiq, 0, 0, vw);
      }
      if (stage_cols) { if (single) loadB(stilq, 0, vb); else loadG(0, vb); }
      TSTAMP0(c, 47);
      if (grp) {
#pragma unroll
        for (int u = 0; u < UW; ++u) {
          const int e = tid + PG_THREADS * u;
          if (e < nitem) {
            const int ci = e / KS, il = e - ci * KS;
            const int g = ci / ncw, col = ci - g * ncw;
            sW[((size_t)g * TB + ((col < K) ? col : col + 1)) * KSP + pos(il)] = (i0 + il < n) ? vw[u] : 0.0;
          }
        }
        for (int x = tid; x < gc * KS; x += PG_THREADS) {
          const int g = x / KS, il = x - g * KS;
          sW[((size_t)g * TB + ONE) * KSP + il] = 1.0; sW[((size_t)g * TB + K + MD) * KSP + il] = 0.0;
        }
      } else {
        storeW(0, 0, vw);
      }
      TSTAMP0(c, 48);
      if (stage_cols) { if (single) storeB(0, vb); else storeG(0, vb); }
      if (!grp)
      for (int il0 = 0; il0 < KS; il0 += PG_THREADS)
        for (int cb = 0; cb < ncw; cb += UW) {
          if (il0 == 0 && cb == 0) continue;
          loadW(Zq, chiq, il0, cb, vw);
          storeW(il0, cb, vw);
        }
      if (stage_cols) {
        if (single) { for (int base = PG_THREADS * UB; base < nB; base += PG_THREADS * UB) { loadB(stilq, base, vb); storeB(base, vb); } }
        else { for (int ub0 = UB; (PG_THREADS / 16) * ub0 < KS; ub0 += UB) { loadG(ub0, vb); storeG(ub0, vb); } }
      }
      TSTAMP0(c, 41);
    }
    __syncthreads();
    TSTAMP0(c, 42);
    if (!single) {
      // pair rows: thread (tx, ty) = (tid % 32, tid / 32) fills pair slots ty, ty + 16, .. of curves tx, tx + 32, ..
      const int tx = tid & 31, ty = tid >> 5;
      for (int il0 = 0; il0 < KS; il0 += 256) {
        for (int e = ty; e < NP * gc; e += PG_THREADS / 32) {
          const int g = GROUPS ? e / NP : 0, ep = e - g * NP;
          const int pk = ptab[ep], ia = pk & 0xffff, ib = pk >> 16;
          double* sPg = sP + (size_t)g * TB * KSP;
          const double* sWg = sW + (size_t)g * TB * KSP;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int il = il0 + tx + 32 * j;
            if (il < KS) sPg[ep * KSP + il] = sWg[ia * KSP + il] * sWg[ib * KSP + il];
          }
        }
        if (ty < gc)
#pragma unroll
          for (int j = 0; j < 8; ++j) { const int il = il0 + tx + 32 * j; if (il < KS) sP[((size_t)ty * TB + NP) * KSP + il] = 0.0; }
      }
      __syncthreads();
    }
    TSTAMP0(c, 43);
    const int wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, kq = lane >> 4;
    const int ntile = single ? d.AT * d.CTS : d.RT;
    const double* wsrc = single ? sW : sP;
    const int ZERO = single ? RS - 1 : RP - 1;
    const int KQ = KS / 4;                     // steps; k-slot kq of step s is curve kq * KQ + s  (KS is a multiple of 16)
    // each wave walks its tiles TPW at a time with independent accumulators
    constexpr int TPW = 2;
    constexpr int NW = PG_THREADS / 64;
    const int nitems = gc * ntile;             // (chain of the group, row tile)
    for (int t0 = wave; t0 < nitems; t0 += NW * TPW) {
      int tix[TPW], bcol[TPW], o1[TPW], o2[TPW], gch[TPW];
      bool tv[TPW];
#pragma unroll
      for (int qq = 0; qq < TPW; ++qq) {
        const int it = t0 + NW * qq;
        tv[qq] = it < nitems;
        gch[qq] = (GROUPS && tv[qq]) ? it / ntile : 0;
        const int tt = it - gch[qq] * ntile;
        o1[qq] = o2[qq] = ZERO; bcol[qq] = lr; tix[qq] = 0;
        if (tv[qq]) {
          if (!single) {
            const int row = tt * 16 + lr;
            tix[qq] = tt * d.CTG + ct;
            if (row < d.R) { const int zz = row / d.NCC; o1[qq] = zz; o2[qq] = d.NZZ + (row - zz * d.NCC); }
          } else {
            const int at = tt / d.CTS, cs = tt - at * d.CTS;
            const int row = at * 16 + lr;
            tix[qq] = d.RT * d.CTG + tt;
            bcol[qq] = cs * 16 + lr;
            if (row < d.A) { const int j = row / MD; o1[qq] = j; o2[qq] = K + (row - j * MD); }
          }
        }
      }
      double4_t acc[TPW];
#pragma unroll
      for (int qq = 0; qq < TPW; ++qq) acc[qq] = double4_t{0.0, 0.0, 0.0, 0.0};
      const v2d* pa[TPW]; const v2d* pb[TPW]; const v2d* pc[TPW];
#pragma unroll
      for (int qq = 0; qq < TPW; ++qq) {
        const double* wg = wsrc + (size_t)gch[qq] * TB * KSP;
        pa[qq] = (const v2d*)(wg + o1[qq] * KSP + kq * KQ);
        pb[qq] = (const v2d*)(wg + o2[qq] * KSP + kq * KQ);
        pc[qq] = (const v2d*)(sB + bcol[qq] * KSP + kq * KQ);
      }
      // The LDS pipe moves 1.5 KB per MFMA and wave -- three quarters of the time the matrix pipe needs for it -- so the
      // two must overlap: a trip is two pairs of k-steps (12 TPW MFMAs); the operands of trip t + 1 are read into the
      // other register set before the MFMAs of trip t are issued (the scheduling barriers keep the compiler from
      // moving the reads back next to their uses).
      struct OpSet { v2d wa[2][TPW], wb[2][TPW], bb[2][TPW]; };
      auto load_trip = [&](OpSet& o, int s2) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int qq = 0; qq < TPW; ++qq) { o.wa[u][qq] = pa[qq][s2 + u]; o.wb[u][qq] = pb[qq][s2 + u]; o.bb[u][qq] = pc[qq][s2 + u]; }
      };
      auto mfma_trip = [&](const OpSet& o, int npair) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
          if (u < npair)
#pragma unroll
            for (int qq = 0; qq < TPW; ++qq) {
              acc[qq] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.wa[u][qq].x * o.wb[u][qq].x, o.bb[u][qq].x, acc[qq], 0, 0, 0);
              acc[qq] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.wa[u][qq].y * o.wb[u][qq].y, o.bb[u][qq].y, acc[qq], 0, 0, 0);
            }
      };
      const int ntrip = KQ / 4;                // KS is a multiple of 16: trip t covers the step pairs 2t, 2t + 1
      OpSet s0, s1;
      load_trip(s0, 0);
      for (int t = 0; t < ntrip; t += 2) {
        if (t + 1 < ntrip) load_trip(s1, 2 * (t + 1));
        __builtin_amdgcn_sched_barrier(0);
        mfma_trip(s0, 2);
        __builtin_amdgcn_sched_barrier(0);
        if (t + 2 < ntrip) load_trip(s0, 2 * (t + 2));
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < ntrip) mfma_trip(s1, 2);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int qq = 0; qq < TPW; ++qq)
        if (tv[qq]) {
          double* out = ptr_shift(c0.pg_part, (size_t)(q + gch[qq]) * c0.chain_bytes) + ((size_t)ks * d.NT + tix[qq]) * 256 + lane;
          // (streaming stores: the 4.5 MB of partial tiles are read next by k_pg_reduce on other XCDs, never again by this one; written
          //  through as they are produced they do not sit dirty in this XCD's L2 until the end-of-kernel write-back)
          // (single chain only: the 8-chain Nu_Z batch measured 2 % slower with them)
          if constexpr (!BATCH) {
            __builtin_nontemporal_store(acc[qq][0], out); __builtin_nontemporal_store(acc[qq][1], out + 64);
            __builtin_nontemporal_store(acc[qq][2], out + 128); __builtin_nontemporal_store(acc[qq][3], out + 192);
          } else {
            out[0] = acc[qq][0]; out[64] = acc[qq][1]; out[128] = acc[qq][2]; out[192] = acc[qq][3];
          }
        }
      TSTAMP0(c, 44);
    }
    if (q + GG < nch) __syncthreads();       // the next group overwrites sW / sP
  }
}

// four lanes per element of every output tile (lane g sums the k-slices g, g + 4, ..: the same four interleaved partial sums
// as ever, combined in the same fixed order), so that the 25 dependent-latency loads of an element shrink to 7
__global__ __launch_bounds__(256) void k_pg_reduce(Ctx c0, int NKS) {
  const Ctx c = chain_view(c0);      // chain blockIdx.z of the batch
  TIMELINE(c, 2);
  const Dims& d = c.d;
  const int gid4 = blockIdx.x * 256 + threadIdx.x;
  const int gid = gid4 >> 2, g = gid4 & 3;
  const bool live = gid < d.NT * 256;
  const int gc = live ? gid : 0;
  const int t = gc >> 8, q = gc & 255;
  const int r = q >> 6, lane = q & 63;
  const int rit = (lane >> 4) + 4 * r, cit = lane & 15;   // D layout of v_mfma_f64_16x16x4_f64
  const double* src = c.pg_part + (size_t)t * 256 + q;
  const size_t stride = (size_t)d.NT * 256;
  double sg = 0.0;
  const int nfull = NKS & ~3;                             // slices 0 .. nfull-1 go to the four interleaved sums
  // eight loads of a lane go out together (the slabs were written by the previous kernel: every load is a trip to memory,
  // and a plain accumulation loop pays one trip per term); the additions keep the sequential order
  for (int k0 = g; k0 < nfull; k0 += 32) {
    double v8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v8[u] = src[(size_t)min(k0 + 4 * u, NKS - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) if (k0 + 4 * u < nfull) sg += v8[u];
  }
  {
    double vt[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) vt[u] = src[(size_t)min(nfull + u, NKS - 1) * stride];
#pragma unroll
    for (int u = 0; u < 3; ++u) if (g == 0 && nfull + u < NKS) sg += vt[u];
  }
  // (s0 + s1) + (s2 + s3), s_g on lane g of the quad
  const double s01 = sg + __shfl_xor(sg, 1, 4);
  const double s = s01 + __shfl_xor(s01, 2, 4);
  if (!live || g != 0) return;
  const int n_pair_tiles = d.RT * d.CTG;
  if (t < n_pair_tiles) {
    const int rt = t / d.CTG, ct = t - rt * d.CTG;
    const int row = rt * 16 + rit, col = ct * 16 + cit;
    if (d.mv) {
      // G_i = I: the block is s I (BW = 0: H2 rows are [G(p, p), 0])
      // (the 16 columns of the tile are the same column of ones: every lane of a row holds the same sum and takes its share
      //  of the P columns)
      if (row < d.R) {
        double* h2 = c.H2 + (size_t)row * d.P * 2;
        for (int p0 = cit; p0 < d.P; p0 += 16) { c.H[(size_t)row * d.LG + p0] = s; h2[2 * p0] = s; }
      }
    } else if (row < d.R && col < d.LG) {
      c.H[(size_t)row * d.LG + col] = s;
      // copy for k_factor / the sweep (h2_index): entry k of row p is G(p, p + k - BW)
      const int dd = col / d.P, p0 = col - dd * d.P, W = 2 * d.BW + 2;
      double* h2 = c.H2 + (size_t)row * d.P * W;
      h2[h2_index(d.P, p0, d.BW + dd)] = s;
      if (dd > 0 && p0 + dd < d.P) h2[h2_index(d.P, p0 + dd, d.BW - dd)] = s;
    }
  } else {
    const int t2 = t - n_pair_tiles;
    const int at = t2 / d.CTS, cs = t2 - at * d.CTS;
    const int row = at * 16 + rit, col = cs * 16 + cit;
    if (row < d.A && col < d.P) c.tvec[(size_t)row * d.P + col] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// pair-Gram for chain BATCHES and LONG curve sets (round 4): row tiles packed across the chains, chunked k-loop
// ---------------------------------------------------------------------------------------------
// The batch is ONE contraction  [nch R pair rows] x [n curves] x [LG record columns]  (+ [nch A single rows] x n x P for t_a):
//  * the 16-row MFMA tiles run over the rows of ALL chains of the (sub-)batch back to back, so only the last tile is padded
//    (8 x 168 rows = 84 full tiles instead of 8 x 11 with 8 rows of padding each; the s part 8 x 21 = 168 rows = 11 tiles
//    instead of 16);
//  * a wave owns ONE packed row tile and ALL column tiles of it (2 NP2 accumulators), so an A operand -- the product of two pair
//    weights -- is formed once per k-step for 2 NP2 MFMAs and the LDS pipe moves 640 B per MFMA instead of 1.5 KB;
//  * the workgroup walks its k-slice in CHUNKS of 16 curves (4 k-steps), double-buffered: the next chunk's records and weights
//    are requested before the MFMAs of this one and stored after them, one barrier per chunk; LDS is ~50 KB and the kernel
//    holds <= 128 VGPRs, so two workgroups (16 waves) share a CU and one's staging hides behind the other's MFMAs.  The
//    accumulators persist across the chunks: partial tiles are written once per k-slice whatever its length.
//  * records are staged as they lie in memory ([curve][column], no transposition): the 16-byte B read of lane (n, kq) holds columns
//    32 tp + 2 n and 32 tp + 2 n + 1 of curve 4 s + kq and feeds TWO column tiles (the even and the odd columns of a 32-column
//    pair) -- any assignment of columns to tiles will do, k_pg_reduce_pack knows it.
// Summation order (canonical, shared with k_pair_gram): slice ks = curves [ks KS, ks KS + KS), one MFMA chain over its k-steps,
// step s = curves 4 s .. 4 s + 3; A = (Z_j Z_j') (chit_m chit_m') resp. Z_j chit_m; slices combined by k_pg_reduce_pack in
// k_pg_reduce's order.  A chain's H and t are therefore bit-identical to what k_pair_gram + k_pg_reduce give it alone.
// Limits (otherwise the launcher keeps k_pair_gram): K <= 4, M <= 8, LG <= 128, P <= 32, no covariates, functional model.
constexpr int PGP_CH = 16;                     // chunk: 16 curves = 4 k-steps
constexpr int PGP_RB = 66;                     // row stride of the staged chunk (doubles): 64 record columns + 2 (16-byte aligned rows)
constexpr int PGP_NWV = 3;                     // most weight values (Z_ik, chi_im) a thread stages per chunk
constexpr int PGP_WPG = 4;                     // waves (= packed row tiles) per workgroup

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES, 4) void k_pair_gram_pack(Ctx c0, PgPack g, double* __restrict__ pack) {
  constexpr int PGP_THREADS = 64 * WAVES;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Dims& d = c0.d;
  const int n = d.n, K = d.K, MD = d.MD, nch = c0.nch;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int ks = blockIdx.y, wg = blockIdx.x;
  const int nwg_g = g.NRG * g.NCG;
  if (ks >= g.NKS || wg >= nwg_g + g.NWG_S) return;
  // A workgroup is (row group, column group): WAVES packed row tiles (one per wave) x 64 record columns (two 32-column pairs,
  // four accumulators per wave).  The s part -- single-weight rows against the P columns of s_i -- runs through the SAME code: its
  // rows multiply Z_j chit_m by 1 x 1 (exact), its 32 columns fill the first pair and the second pair's accumulators are dropped.
  const bool single = wg >= nwg_g;
  const int rg = single ? wg - nwg_g : wg / g.NCG, cg = single ? 0 : wg - rg * g.NCG;
  const int i0 = ks * g.KS;
  const int nchunk = (min(g.KS, n - i0) + PGP_CH - 1) / PGP_CH;
  const int SL = g.SLS;                     // raw weight row of a (chain, curve): Z_1 .. Z_K | 1, chi_1 .. chi_M | 0 (| pad)
  const int RW = single ? d.A : d.R;        // rows per chain
  const int tile0 = rg * WAVES;
  const int ntile = single ? g.TS : g.TG;
  const int q0 = min((tile0 * 16) / RW, nch - 1);       // the chains this workgroup's rows belong to
  const int q1 = min(((min(tile0 + WAVES, ntile)) * 16 - 1) / RW, nch - 1);
  const int nq = q1 - q0 + 1;
  constexpr int nbuf_b = 16 * PGP_RB;
  double* sBb = smem;                                   // 2 x 16 x RB     record chunk, [curve][column]
  double* sWb = smem + 2 * nbuf_b;                      // 2 x nq x 16 x SL   weights, [chain][curve][slot]
  const int nbuf_w = nq * 16 * SL;
  // ---- staging roles ----
  // records: ONE 16-byte piece per thread: curve il = tid / 32 of the chunk, columns cb0 + 2 pc, + 1 (pc = tid % 32); the s part
  // starts at column LG, which need not be 16-byte aligned: two 8-byte loads there
  constexpr int NPB = 512 / PGP_THREADS;          // pieces per thread: piece e = tid + PGP_THREADS u -> curve e / 32, columns 2 (e % 32), + 1
  const int b_pc = tid & 31;
  const int cb0 = single ? d.LG : 64 * cg, cend = single ? d.LG + d.P : d.LG;      // (columns beyond the part are zero)
  const int bc = cb0 + 2 * b_pc;
  const bool ok0 = bc < cend, ok1 = bc + 1 < cend;
  const int bc0 = min(bc, d.LREC - 2);
  v2d vb[NPB];
  // weights: value e = tid + 512 u of the workgroup's (chain, column, curve) items, curve fastest: chain q0 + e / (16 NV), source
  // column (e / 16) % NV (Z_1 .. Z_K, chi_1 .. chi_M), curve e % 16 -- sixteen consecutive threads read a 128-byte segment
  const int NV = K + MD - 1, nval = nq * NV * 16;
  double wv[PGP_NWV];
  const double* wsrc[PGP_NWV];
  int wdst[PGP_NWV];
#pragma unroll
  for (int u = 0; u < PGP_NWV; ++u) {
    const int e = min(tid + PGP_THREADS * u, nval - 1);
    const int qq = e / (16 * NV), v = (e >> 4) - qq * NV;
    const size_t offq = (size_t)(q0 + qq) * c0.chain_bytes;
    wsrc[u] = (v < K) ? ptr_shift(c0.Z, offq) + (size_t)n * v : ptr_shift(c0.chi, offq) + (size_t)n * (v - K);
    wdst[u] = (qq * 16 + (e & 15)) * SL + ((v < K) ? v : v + 1);
    wv[u] = 0.0;
  }
  const int w_il = tid & 15;
  auto load_chunk = [&](int t) {
    const int ib = i0 + t * PGP_CH;
#pragma unroll
    for (int u = 0; u < NPB; ++u) {
      const int b_il = (tid + PGP_THREADS * u) >> 5;
      const double* src = c0.rec + (size_t)min(ib + b_il, n - 1) * d.LREC + bc0;
      if (!single) vb[u] = *(const v2d*)src;
      else { vb[u].x = src[0]; vb[u].y = src[1]; }
    }
    const int i = min(ib + w_il, n - 1);
#pragma unroll
    for (int u = 0; u < PGP_NWV; ++u)
      if (PGP_THREADS * u < nval) wv[u] = wsrc[u][i];
  };
  auto store_chunk = [&](int t, int buf) {
    const int ib = i0 + t * PGP_CH;
#pragma unroll
    for (int u = 0; u < NPB; ++u) {
      const int b_il = (tid + PGP_THREADS * u) >> 5;
      const bool liveb = ib + b_il < n;
      v2d o2;
      o2.x = (liveb && ok0) ? vb[u].x : 0.0; o2.y = (liveb && ok1) ? vb[u].y : 0.0;
      *(v2d*)(sBb + buf * nbuf_b + b_il * PGP_RB + 2 * b_pc) = o2;
    }
    const bool live = ib + w_il < n;
    double* sW = sWb + buf * nbuf_w;
#pragma unroll
    for (int u = 0; u < PGP_NWV; ++u)
      if (tid + PGP_THREADS * u < nval) sW[wdst[u]] = live ? wv[u] : 0.0;
  };
  // the constant slots of both weight buffers: chit_0 = 1 at K, the zero slot (rows of the tile padding) at K + MD
  for (int x = tid; x < 2 * nq * 16; x += PGP_THREADS) {
    double* w = sWb + (x / (nq * 16)) * nbuf_w + (x % (nq * 16)) * SL;
    w[K] = 1.0; w[K + MD] = 0.0;
  }
  // ---- MFMA role of the wave: packed row tile tile0 + wave, four accumulators (column pair 0 even / odd, pair 1 even / odd) ----
  double4_t acc[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) acc[x] = double4_t{0.0, 0.0, 0.0, 0.0};
  // LDS offsets (doubles, within a weight buffer) of the four factors of this lane's row: A = (w[o0] w[o1]) (w[o2] w[o3]);
  // pair row (j, j', m, m'): Z_j Z_j' chit_m chit_m';  single row (j, m): Z_j chit_m 1 1;  padding rows: the zero slot
  const int ZERO = K + MD;
  int o0 = ZERO, o1 = ZERO, o2_ = ZERO, o3 = ZERO;
  const int tile = tile0 + wave;
  const bool has_tile = tile < ntile;
  if (has_tile) {
    const int grow = tile * 16 + lr;
    const int q = grow / RW, r = grow - q * RW;
    if (q < nch) {
      const int base = (q - q0) * 16 * SL;
      if (!single) {
        const int zz = r / d.NCC, cc = r - zz * d.NCC;
        int a = 0, e = zz;
        while (e >= K - a) { e -= K - a; ++a; }
        o0 = base + a; o1 = base + a + e;
        a = 0; e = cc;
        while (e >= MD - a) { e -= MD - a; ++a; }
        o2_ = base + K + a; o3 = base + K + a + e;
      } else {
        const int j = r / MD;
        o0 = base + j; o1 = base + K + (r - j * MD); o2_ = base + K; o3 = base + K;
      }
    }
  }
  auto mfma_chunk = [&](int buf) {
    const double* sB = sBb + buf * nbuf_b + 2 * lr;
    const double* sW = sWb + buf * nbuf_w;
#pragma unroll
    for (int s2 = 0; s2 < 4; s2 += 2) {
      double a[2];
      v2d b[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int il = 4 * (s2 + u) + kq;
        const double* w = sW + il * SL;
        a[u] = (w[o0] * w[o1]) * (w[o2_] * w[o3]);
        b[u][0] = *(const v2d*)(sB + il * PGP_RB);
        b[u][1] = *(const v2d*)(sB + il * PGP_RB + 32);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][0].x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][0].y, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][1].x, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][1].y, acc[3], 0, 0, 0);
      }
    }
  };
  // ---- the chunk pipeline: the next chunk is requested before the MFMAs of this one and stored behind them ----
  load_chunk(0);
  store_chunk(0, 0);
  __syncthreads();
  for (int t = 0; t < nchunk; ++t) {
    if (t + 1 < nchunk) load_chunk(t + 1);
    mfma_chunk(t & 1);
    if (t + 1 < nchunk) store_chunk(t + 1, (t + 1) & 1);
    __syncthreads();
  }
  // ---- partial tiles of this k-slice, accumulator layout (k_pg_reduce_pack): pair tile T, column pair tp, parity par at
  //      index (T NP2 + tp) 2 + par; single tile T, parity par at TG 2 NP2 + 2 T + par ----
  if (!has_tile) return;
  double* out0 = pack + (size_t)ks * g.NTP * 256 + lane;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int tp = 2 * cg + (x >> 1);
    const bool keep = single ? (x < 2) : (tp < g.NP2);
    if (keep) {
      const int idx = single ? g.TG * 2 * g.NP2 + tile * 2 + x : (tile * g.NP2 + tp) * 2 + (x & 1);
      double* out = out0 + (size_t)idx * 256;
      out[0] = acc[x][0]; out[64] = acc[x][1]; out[128] = acc[x][2]; out[192] = acc[x][3];
    }
  }
}

// pi / alpha_3 (+ the deferred log-likelihood) of every chain of the (sub-)batch: in k_pair_gram this job rides as an extra
// workgroup; inside k_pair_gram_pack it would cost that kernel its register budget (the job needs 177 VGPRs, the contraction 88),
// so it is a workgroup of the NEXT kernel, k_factor, whose register budget it fits; the spare jobs there that read pi / alpha_3
// wait for its flag (k_factor: pi_in_factor).  Tried first: as workgroups of the reduction kernel (its 177 VGPRs then set that
// memory-bound kernel's occupancy: 17.7 us instead of 12 for 8 chains, 59 instead of 40 for 32) and on a side stream forked and
// joined inside the captured graph (the two cross-stream edges cost the 8-chain batch 80 us per step).
// fixed-order sum of the k-slices of the packed partial tiles (the order of k_pg_reduce: four interleaved partial sums over the
// slices, then (s0 + s1) + (s2 + s3)) and scatter to the chains' H, H2, t
__global__ __launch_bounds__(256) void k_pg_reduce_pack(Ctx c0, PgPack g, const double* __restrict__ pack) {
  const Dims& d = c0.d;
  const int bx = blockIdx.x;
  const int gid4 = bx * 256 + threadIdx.x;
  const int gid = gid4 >> 2, gl = gid4 & 3;
  const bool live = gid < g.NTP * 256;
  const int gc = live ? gid : 0;
  const int t = gc >> 8, q = gc & 255;
  const int r = q >> 6, lane = q & 63;
  const int rit = (lane >> 4) + 4 * r, cit = lane & 15;   // D layout of v_mfma_f64_16x16x4_f64
  const double* src = pack + (size_t)t * 256 + q;
  const size_t stride = (size_t)g.NTP * 256;
  const int NKS = g.NKS;
  double sg = 0.0;
  const int nfull = NKS & ~3;
  for (int k0 = gl; k0 < nfull; k0 += 32) {
    double v8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v8[u] = src[(size_t)min(k0 + 4 * u, NKS - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) if (k0 + 4 * u < nfull) sg += v8[u];
  }
  {
    double vt[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) vt[u] = src[(size_t)min(nfull + u, NKS - 1) * stride];
#pragma unroll
    for (int u = 0; u < 3; ++u) if (gl == 0 && nfull + u < NKS) sg += vt[u];
  }
  const double s01 = sg + __shfl_xor(sg, 1, 4);
  const double s = s01 + __shfl_xor(s01, 2, 4);
  if (!live || gl != 0) return;
  const int NACC = 2 * g.NP2;
  if (t < g.TG * NACC) {
    const int tile = t / NACC, x = t - tile * NACC;      // x = 2 tp + par
    const int grow = tile * 16 + rit;
    const int qc = grow / d.R, row = grow - qc * d.R;
    const int col = 32 * (x >> 1) + 2 * cit + (x & 1);
    if (qc < c0.nch && col < d.LG) {
      const size_t off = (size_t)qc * c0.chain_bytes;
      ptr_shift(c0.H, off)[(size_t)row * d.LG + col] = s;
      const int dd = col / d.P, p0 = col - dd * d.P, W = 2 * d.BW + 2;
      double* h2 = ptr_shift(c0.H2, off) + (size_t)row * d.P * W;
      h2[h2_index(d.P, p0, d.BW + dd)] = s;
      if (dd > 0 && p0 + dd < d.P) h2[h2_index(d.P, p0 + dd, d.BW - dd)] = s;
    }
  } else {
    const int t2 = t - g.TG * NACC;
    const int tile = t2 >> 1, par = t2 & 1;
    const int grow = tile * 16 + rit;
    const int qc = grow / d.A, a = grow - qc * d.A;
    const int p = 2 * cit + par;
    if (qc < c0.nch && p < d.P) ptr_shift(c0.tvec, (size_t)qc * c0.chain_bytes)[(size_t)a * d.P + p] = s;
  }
}

// ---- host side: geometry, the route decision, launchers ---------------------------------------
void pg_geometry(const Dims& d, int& NKS, int& KS) {
  // k-slices of the pair-Gram contraction.  LDS doubles per curve: the raw weight row, the record columns and,
  // for the G workgroups, the pair-weight row (k_pair_gram); a workgroup never stages more than 96 KB.
  const int row_g = (d.K + d.MD + 1) + 16 + (d.NZZ + d.NCC + 1);
  const int row_s = (d.K + d.MD + 1) + d.CTS * 16;
  const int ks_cap = std::max(16, (int)((96 * 1024) / (sizeof(double) * (size_t)std::max(row_g, row_s)) - 2) / 16 * 16);
  // one workgroup per CU: (CTG + 2) column groups x NKS k-slices <= 256 whenever the LDS cap allows, so that
  // every workgroup is resident at once (a 257th would wait a whole workgroup lifetime for a free CU)
  NKS = std::max(1, std::min(256 / (d.CTG + 2), d.n / 16));
  KS = (d.n + NKS - 1) / NKS;
  KS = (KS + 15) / 16 * 16;                  // MFMA k-slots are taken in trips of 4 steps per slot (two 16-byte LDS reads)
  KS = std::min(KS, ks_cap);
  NKS = (d.n + KS - 1) / KS;
}

// LDS of k_pair_gram for groups of G chains: record columns + G chains' tables (G workgroups: 16 + G (RS + RP) rows; s workgroup:
// 16 CTS + G RS) + pair table, and at least the scalar jobs' scratch
static size_t pair_gram_lds_bytes(const Dims& d, int KS, int G) {
  const int RS = d.K + d.MD + 1, RP = d.NZZ + d.NCC + 1;
  const size_t tables = (size_t)(KS + 2) * std::max(16 + G * (RS + RP), d.CTS * 16 + G * RS) + 128;
  return std::max(tables, (size_t)std::max(PI_ALPHA_LDS_DOUBLES, HYPER_LDS_DOUBLES)) * sizeof(double);
}

// geometry of k_pair_gram_pack for this (sub-)batch; returns false when the shape is outside its limits (the route keeps k_pair_gram)
static size_t pgp_lds_bytes(const PgPack& g) {
  const size_t lg = 2 * (16 * (size_t)PGP_RB + (size_t)g.NQG * 16 * g.SLS), ls = 2 * (16 * (size_t)PGP_RB + (size_t)g.NQS * 16 * g.SLS);
  return std::max(lg, ls) * sizeof(double);
}
static bool pgp_geometry(const Dims& d, int nch, int KS, int NKS, PgPack& g) {
  if (d.mv || d.D > 0 || d.K > 4 || d.MD - 1 > 8 || d.P > 32 || (d.LREC & 1) || (KS & 15)) return false;
  g.KS = KS; g.NKS = NKS;
  g.NP2 = (d.LG + 31) / 32;
  g.TG = (nch * d.R + 15) / 16; g.TS = (nch * d.A + 15) / 16;
  g.WPG = PGP_WPG;
  g.NRG = (g.TG + PGP_WPG - 1) / PGP_WPG; g.NCG = (g.NP2 + 1) / 2; g.NWG_S = (g.TS + PGP_WPG - 1) / PGP_WPG;
  g.SLG = (d.NZZ + d.NCC + 1 + 1) & ~1; g.SLS = (d.K + d.MD + 1 + 1) & ~1;
  g.NQG = std::min(nch, (PGP_WPG * 16 + d.R - 2) / d.R + 1); g.NQS = std::min(nch, (PGP_WPG * 16 + d.A - 2) / d.A + 1);
  g.NTP = g.TG * 2 * g.NP2 + g.TS * 2;
  const int NV = d.K + d.MD - 1;
  if (std::max(g.NQG, g.NQS) * NV * 16 > PGP_NWV * 64 * PGP_WPG) return false;      // weight values a thread stages per chunk
  return pgp_lds_bytes(g) <= 64 * 1024;
}
size_t pgp_pack_doubles(const PgPack& g) { return (size_t)g.NKS * g.NTP * 256; }

// The one decision of how a (sub-)batch runs the contraction: nch chains (a sub-batch of a handle of nch_handle chains), pg =
// the plan runs the contraction (otherwise the launch only carries the extra workgroups' scalar jobs), pg_part_doubles = the
// capacity of Ctx::pg_part, may_pack = the driver can give the packed tiles a buffer.  Pure arithmetic on its arguments and
// the two process-wide switches; the launchers launch what it says and bfmmm_debug_get("pg_route") reports it.
// Packed: the batch has four or more chains -- warm-start and Nu_Z sweeps alike (measured, chain-iterations/s plain / packed:
// 4 warm chains 35.3 k / 40.4 k, 6: 44.9 / 46.9; 4 Nu_Z chains 65.0 / 68.3, 6: 84.4 / 92.6, 8: 105 / 114; two chains: no gain) --
// or the curve set is long (beyond the cache-resident sizes: k_pair_gram's k-slices are capped by its LDS staging, so at
// n = 262144 it writes 1366 slabs of partial tiles -- as many bytes as the records themselves; k_pair_gram_pack walks a slice
// of ANY length in 16-curve chunks with persistent accumulators: about 128 slices whatever n, chosen from n alone so that a
// chain of a batch and the same chain alone sum in the same order).  Both kernels sum in the same order.
PgRoute pg_route_decide(const Dims& d, int nch_handle, int nch, bool pg, bool defer_loglik, size_t pg_part_doubles, bool may_pack) {
  PgRoute r;
  pg_geometry(d, r.NKS, r.KS);
  const int KSl = ((d.n + 127) / 128 + 15) / 16 * 16, NKSl = (d.n + KSl - 1) / KSl;
  const bool long_set = d.n > 16384 && pgp_geometry(d, 1, KSl, NKSl, r.pk);
  if (long_set) { r.KS = KSl; r.NKS = NKSl; }
  if (may_pack && pg && (long_set || nch_handle >= 4) && pgp_geometry(d, nch, r.KS, r.NKS, r.pk)) {
    r.packed = true;
    r.lds = pgp_lds_bytes(r.pk);
    return r;
  }
  // k_pair_gram keeps the long-set slices where it can stage them (a chain then sums as it does alone), its own otherwise
  if (long_set && (pair_gram_lds_bytes(d, r.KS, 1) > 160 * 1024 || (size_t)r.NKS * d.NT * 256 > pg_part_doubles))
    pg_geometry(d, r.NKS, r.KS);
  // chains staged together (k_pair_gram): as many as 144 KB of LDS and 12 staged doubles per thread allow; covariate-adjusted
  // models stage s~_i per chain and keep one chain per group
  const int ncw = d.K + d.MD - 1;
  r.G = 1;
  if (nch > 1 && d.D == 0 && d.RT < 8)      // (with eight or more row tiles per chain the waves are busy chain by chain)
    while (r.G < nch && pair_gram_lds_bytes(d, r.KS, r.G + 1) <= 144 * 1024 && (size_t)(r.G + 1) * ncw * r.KS <= 12 * 512) ++r.G;
  // (the single-chain body of the G workgroups where the shape allows: pg_solo_g; bfmmm_set_solo_pair_gram(0) keeps the general one)
  r.body = nch > 1 ? (r.G > 1 ? 3 : 2) : (g_solo_pair_gram && pg_solo_fits(d, r.KS)) ? 1 : 0;
  r.lds = pair_gram_lds_bytes(d, r.KS, r.G);
  if (pg && r.body == 1) {
    // what else the single-chain launch does in bodies of its own: the s-part workgroup (pg_solo_s), the deferred
    // log-likelihood in the third extra workgroup (the grid's y extent is NKS: three k-slices or more); neither where a
    // condition fails or after bfmmm_set_solo_pair_gram_tail(0)
    if (g_solo_pair_gram_tail) {
      if (d.AT * d.CTS <= PG_THREADS / 64 && d.CTS <= 2) r.tail |= PG_SOLO_S;
      if (defer_loglik && r.NKS >= 3) r.tail |= PG_SOLO_LL;
    }
    r.do_pg = PG_SOLO | r.tail;
    // (pg_solo_s stages A + 1 single-weight rows where the general body stages RS raw ones; KS <= 256: at most 142 KB)
    if (r.tail & PG_SOLO_S) r.lds = std::max(r.lds, (size_t)(r.KS + 2) * (d.CTS * 16 + d.A + 1) * sizeof(double));
  } else {
    r.do_pg = pg ? 1 : 0;
  }
  return r;
}

bool pg_route_solo_ll(const PgRoute& r) { return !r.packed && r.body <= 1 && (r.do_pg & PG_SOLO_LL) != 0; }

void launch_pair_gram(const Ctx& c, const PgRoute& r, hipStream_t st) {
  const Dims& d = c.d;
  if (r.body == 3) hipLaunchKernelGGL((k_pair_gram<true, true>), dim3(d.CTG + 2, r.do_pg ? std::max(r.NKS, c.nch) : c.nch, 1), dim3(PG_THREADS), r.lds, st, c, r.KS, r.NKS, r.do_pg, r.G);
  else if (r.body == 2) hipLaunchKernelGGL((k_pair_gram<true, false>), dim3(d.CTG + 2, r.do_pg ? std::max(r.NKS, c.nch) : c.nch, 1), dim3(PG_THREADS), r.lds, st, c, r.KS, r.NKS, r.do_pg, 1);
  else hipLaunchKernelGGL((k_pair_gram<false, false>), dim3(d.CTG + 2, r.do_pg ? r.NKS : 1, 1), dim3(PG_THREADS), r.lds, st, c, r.KS, r.NKS, r.do_pg, 1);
}

void launch_pair_gram_pack(const Ctx& c, const PgRoute& r, hipStream_t st) {
  const PgPack& g = r.pk;
  const dim3 grid(g.NRG * g.NCG + g.NWG_S, g.NKS, 1);
  hipLaunchKernelGGL(k_pair_gram_pack<PGP_WPG>, grid, dim3(64 * PGP_WPG), r.lds, st, c, g, r.pack);
  const int nblk_red = (g.NTP * 256 * 4 + 255) / 256;
  hipLaunchKernelGGL(k_pg_reduce_pack, dim3(nblk_red), dim3(256), 0, st, c, g, r.pack);      // (the pi / alpha_3 job: a workgroup of k_factor, Ctx::pi_in_factor)
}

void launch_pg_reduce(const Ctx& c, int NKS, hipStream_t st) {
  const int nthreads = c.d.NT * 256 * 4;        // four lanes per element
  hipLaunchKernelGGL(k_pg_reduce, dim3((nthreads + 255) / 256, 1, c.nch), dim3(256), 0, st, c, NKS);
}

void prepare_pair_gram_kernels() {
  set_max_lds((const void*)k_pair_gram<false, false>); set_max_lds((const void*)k_pair_gram<true, false>); set_max_lds((const void*)k_pair_gram<true, true>);
}

}  // namespace bfmmm
