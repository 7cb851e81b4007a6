// The sequential side of the Phi / nu block: the Gauss-Seidel sweep over the directions, sigma^2 and the log-likelihood.
//
// With every H_ab and t_a of the iteration in hand (kernels_pair_gram.hip) and every C_a and L_a z_a factorised
// (kernels_factor.hip), the K*M + K sequentially dependent draws  theta_a = C_a rhs_a + L_a z_a  run on a few hundred KB of H
// inside one workgroup instead of K*M + K passes over all curves.
//
//   k_sweep        : Phi sweep, nu sweep, sigma^2 (the critical chain), general form
//   k_sweep_diag   : the same for the diagonal (multivariate) model: independent scalar chains per coordinate
//   k_sweep_chain  : the same with the chain in one wave and row threads around it (k_sweep_tables: its step tables)
//   k_loglik       : calcLikelihood (CalculateLikelihood.h:19-44) from the per-curve residual sums; k_loglik_flush runs the
//                    jobs a run's last iteration left pending
//   k_fill_slots   : broadcast of the blocks a sweep does not update into their chain slots
#include "model.hpp"
#include "rng.hpp"
#include "scalar_jobs.hpp"
#include "factor_core.hpp"
#include "sweep_helpers.hpp"
#include "launchers.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace bfmmm {

// ---------------------------------------------------------------------------------------------
// k_sweep: the sequentially dependent Gaussian block draws of one Gibbs iteration
// (updatePhi: j outer, m inner, UpdatePhi.h:40-84; then updateNu, UpdateNu.h:39-70) and sigma^2
// (UpdateSigma.h:22-58).  One workgroup of 1024 threads; two barriers per draw:
//   phase A  theta_a <- C_a rhs_a + (L z)_a                          (8 threads per row)
//   phase B  r_b -= H_ba (theta_a_new - theta_a_old) for every b     (one thread per element)
//            and, for the next direction a', rhs_a' = (beta/sigma^2)(r_a' + H_a'a' theta_a')
// The column blocks H_{.,a} and C_a of the NEXT step are fetched into registers while the
// current step runs and parked in the other half of an LDS double buffer, so no step waits on
// global memory.
// ---------------------------------------------------------------------------------------------
constexpr int SW_THREADS = 1024;
constexpr int NPF = 6;            // staged doubles per thread and step: A*LG + P*P <= 6144

__global__ __launch_bounds__(SW_THREADS) void k_sweep(Ctx c0, int direct) {
  const Ctx c = chain_view(c0);      // chain blockIdx.z of the batch
  TIMELINE(c, 4);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Dims& d = c.d;
  const int P = d.P, A = d.A, K = d.K, M = d.M, MD = d.MD, BW = d.BW, LG = d.LG;
  const int tid = threadIdx.x;
  Dyn* dyn = c.dyn;
  const int AP = A * P;
  const int PS = P + 2 * BW;                 // padded vector stride
  double* th = smem;                         // A x PS (zero pads)
  double* tv = th + A * PS;                  // A x P
  double* r = tv + AP;                       // A x P
  double* hq = r + AP;                       // A x P   H_aa theta_a
  double* lz = hq + AP;                      // A x P   L_a z_a
  double* rhs = lz + AP;                     // PMAX
  double* dlp = rhs + PMAX;                  // PMAX + 2*BWWIDE (zero pads)
  double* red = dlp + PMAX + 2 * BWWIDE;     // 32
  // direct != 0: the column blocks and C_a do not fit the LDS double buffer (A*LG + P*P > 6144 doubles or the total
  // beyond 160 KB): no staging, every step reads them from L2 (slower per step, but no size limit)
  // diagonal model (multivariate: G_i = I and priors I/tau, diag(tilde_tau gamma)): every H block and every C_a is
  // diagonal, so only the diagonal of C_a is staged and phase A is one multiply per coordinate
  const bool diag = (BW == 0 && d.BWP == 0);
  const int csz = diag ? P : P * P;
  const int pf_len = direct ? 0 : A * LG + csz;
  double* pbuf0 = red + 32;
  double* pbuf1 = pbuf0 + pf_len;
  int* htab = (int*)(pbuf1 + pf_len);        // A x A : H row of block (b, a)
  const uint32_t slot = dyn->slot;
  const uint32_t mask = c.mask;
  const double beta = dyn->beta;
  const double f = beta / dyn->sigma2;
  if (tid == 0) { dyn->iter_hyper = dyn->iter; dyn->slot_hyper = slot; }
  const RngKey key = make_key(c.seed, c.chain, dyn->iter, dyn->tt_step);
  const int n_phi = ((mask & U_PHI) && MD > 1) ? K * M : 0;
  const int n_nu = (mask & U_NU) ? K : 0;
  const int n_steps = n_phi + n_nu;

  // the standard gamma variate of the sigma^2 draw was produced by a spare k_factor workgroup (job_hyper_draws)
  const double sig_g = (mask & U_SIGMA) ? c.gstd[hyper_gstd_count(d)] : 0.0;
  for (int e = tid; e < A * PS; e += SW_THREADS) {
    const int b = e / PS, pp = e - b * PS - BW;
    th[e] = (pp >= 0 && pp < P) ? c.theta[(size_t)full_dir(d, b) * P + pp] : 0.0;
  }
  for (int e = tid; e < AP; e += SW_THREADS) { tv[e] = c.tvec[e]; r[e] = c.rvec[e]; hq[e] = c.hq[e]; lz[e] = c.Lz[e]; }
  for (int e = tid; e < PMAX + 2 * BWWIDE; e += SW_THREADS) dlp[e] = 0.0;
  for (int e = tid; e < A * A; e += SW_THREADS) htab[e] = hrow(d, e / A, e % A);
  __syncthreads();
  // per-thread prefetch map: element e of [ H column blocks | C ] of a step
  int pf_b[NPF], pf_off[NPF];
#pragma unroll
  for (int k = 0; k < NPF; ++k) {
    const int e = tid + SW_THREADS * k;
    pf_b[k] = -2; pf_off[k] = 0;
    if (e < A * LG) { pf_b[k] = e / LG; pf_off[k] = e - pf_b[k] * LG; }
    else if (e < pf_len) { pf_b[k] = -1; pf_off[k] = e - A * LG; }
  }
  double preg[NPF];
  // branch-free: every lane always loads from a valid address (dummy lanes re-read H[0]) so that the
  // NPF loads of a step are issued back to back instead of one memory latency apart
  auto pf_load = [&](int a) {
#pragma unroll
    for (int k = 0; k < NPF; ++k) {
      const int hb = max(pf_b[k], 0);
      const size_t offH = (size_t)htab[hb * A + a] * LG + pf_off[k];
      const size_t offC = (size_t)a * P * P + (diag ? (size_t)pf_off[k] * (P + 1) : (size_t)pf_off[k]);
      const double* src = (pf_b[k] == -1) ? (c.Cmat + offC) : (c.H + ((pf_b[k] >= 0) ? offH : 0));
      preg[k] = *src;
    }
  };
  auto pf_store = [&](double* buf) {
#pragma unroll
    for (int k = 0; k < NPF; ++k)
      if (pf_b[k] >= -1) buf[tid + SW_THREADS * k] = preg[k];
  };
  if (n_steps > 0) {
    // H and C were written by other XCDs (k_pg_reduce, k_factor): a first touch costs a trip to memory, several times a
    // step of the chain.  Touch both once with fire-and-forget loads (one 4-byte load per 128-byte line) so that the
    // per-step prefetch only sees L2 hits.
    {
      int w0 = 0;
      auto touch = [&](const double* src, size_t count) {
        const size_t nl = (count * 8 + 127) / 128;
        for (size_t x = tid; x < nl; x += SW_THREADS) {
          const uint32_t o = (uint32_t)(x * 128);
          asm volatile("global_load_dword %0, %1, %2" : "+v"(w0) : "v"(o), "s"(src));
        }
      };
      touch(c.H, (size_t)d.R * LG);
      touch(c.Cmat, (size_t)A * P * P);
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(w0) :: "memory");
    }
    const int a0 = step_dir(d, 0, n_phi);
    if (!direct) { pf_load(a0); pf_store(pbuf0); }
    if (tid < P) rhs[tid] = f * (r[a0 * P + tid] + hq[a0 * P + tid]);
  }
  __syncthreads();
  for (int st = 0; st < n_steps; ++st) {
    const int a = step_dir(d, st, n_phi);
    const bool more = st + 1 < n_steps;
    const int an = more ? step_dir(d, st + 1, n_phi) : -1;
    const double* buf = (st & 1) ? pbuf1 : pbuf0;
    const double* Cg = direct ? c.Cmat + (size_t)a * P * P : buf + (size_t)A * LG;
    if (more && !direct) pf_load(an);
    // phase A: new = C rhs + L z
    if (diag) {
      if (tid < P) {
        const double cd = direct ? Cg[(size_t)tid * (P + 1)] : Cg[tid];
        const double nw = cd * rhs[tid] + lz[a * P + tid];
        dlp[BW + tid] = nw - th[a * PS + BW + tid];
        th[a * PS + BW + tid] = nw;
      }
    } else
    for (int p = tid >> 3; p < P; p += SW_THREADS / 8) {
      const int seg = tid & 7;
      double acc = 0.0;
      for (int q = seg; q < P; q += 8) acc += Cg[p + P * q] * rhs[q];
      acc += __shfl_xor(acc, 1, 8);
      acc += __shfl_xor(acc, 2, 8);
      acc += __shfl_xor(acc, 4, 8);
      if (seg == 0) {
        const double nw = acc + lz[a * P + p];
        dlp[BW + p] = nw - th[a * PS + BW + p];
        th[a * PS + BW + p] = nw;
      }
    }
    lds_barrier();
    // phase B: r_b -= H_ba dl ; hq_a ; next rhs
    for (int e = tid; e < AP; e += SW_THREADS) {
      const int b = e / P, p = e - b * P;
      const double* Hb = direct ? c.H + (size_t)htab[b * A + a] * LG : buf + (size_t)b * LG;
      const double* dl = dlp + BW + p;
      double v = Hb[p] * dl[0];
      for (int dd = 1; dd <= BW; ++dd) v += Hb[dd * P + p] * dl[dd] + Hb[dd * P + p - dd] * dl[-dd];
      const double rn = r[e] - v;
      r[e] = rn;
      if (b == a) hq[e] += v;                       // H_aa theta_a follows theta_a
      if (b == an) rhs[p] = f * (rn + hq[e]);
    }
    if (more && !direct) pf_store((st & 1) ? pbuf0 : pbuf1);
    lds_barrier();
  }
  // ---------------- sigma^2 (updateSigma, UpdateSigma.h:22-58) ---------------------------------
  if (mask & U_SIGMA) {
    // RSS = YY - sum_a theta_a'(t_a + r_a), fixed-order reduction
    // (covariate-adjusted: YY is replaced by sum_i yy_i - 2 o_i's_i + o_i'G_i o_i, block partials of k_curve_z)
    double acc = 0.0;
    for (int e = tid; e < AP; e += SW_THREADS) {
      const int b = e / P, p = e - b * P;
      acc += th[b * PS + BW + p] * (tv[e] + r[e]);
    }
    if (d.D > 0)
      for (int e = tid; e < c.nblk_curve; e += SW_THREADS) acc -= c.yyp_part[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == SW_THREADS - 1) {
      double q = 0.0;
      for (int w = 0; w < SW_THREADS / 64; ++w) q += red[w];
      const double rss = (d.D > 0) ? -q : (c.YY - q);
      const bool tempered = (dyn->tt_step != 0);
      const double b = (tempered ? (beta / 2) * rss : 0.5 * rss) + c.h.beta_0;
      const double s2 = 1.0 / (sig_g * (1.0 / b));
      dyn->sigma2 = s2;
      dyn->rss = rss;
      c.c_sigma[slot] = s2;
    }
  } else if (tid == 0) {
    c.c_sigma[slot] = dyn->sigma2;
  }
  // ---------------- publish theta and its chain slots -------------------------------------------
  double* s_nu = c.c_nu + (size_t)slot * K * P;
  double* s_phi = c.c_Phi + (size_t)slot * K * P * M;
  for (int e = tid; e < AP; e += SW_THREADS) {
    const int b = e / P, p = e - b * P;
    const int jj = b / MD, mt = b - jj * MD;
    const double v = th[b * PS + BW + p];
    c.theta[(size_t)(jj * (M + 1) + mt) * P + p] = v;
    if (mt == 0) s_nu[jj + (size_t)K * p] = v;
    else s_phi[jj + (size_t)K * (p + (size_t)P * (mt - 1))] = v;
  }
  if (MD == 1)
    for (int e = tid; e < K * P * M; e += SW_THREADS) {
      const int k = e % K, pm = e / K, p = pm % P, m = pm / P;
      s_phi[e] = c.theta[(size_t)(k * (M + 1) + m + 1) * P + p];
    }
}

// ---------------------------------------------------------------------------------------------
// k_sweep_diag: the sweep of the DIAGONAL model (multivariate: G_i = I, priors I/tau and diag(tilde_tau gamma)).
// Every H block and every C_a is diagonal, so the coordinates p are independent scalar Gauss-Seidel chains: 8 lanes
// per coordinate share its A directions (direction b lives on lane b % 8, slot b / 8) and keep r_b, H_bb theta_b, C_a,
// L z, theta in registers; a step is a handful of FMAs, an 8-lane DPP sum that broadcasts delta, and the H entries of
// the next step requested one step ahead.  No LDS hand-off and no barrier inside the sweep.  r follows the general
// kernel's definition (r_a = t_a - sum_b H_ab theta_b over all b).  One workgroup of 8 P threads; A <= 64.
// ---------------------------------------------------------------------------------------------
constexpr int DG_RPL_MAX = 8;      // directions per lane, at most (k_sweep_diag<DG_RPL>: DG_RPL = ceil(A / 8), the slots a lane really has)

// SCALAR_BLOCKS: a compile-time switch (the two sources of a step's H column must not meet in one load: a selected LDS-or-global
// pointer is a FLAT load)
template <int DG_RPL, bool SCALAR_BLOCKS>
__global__ __launch_bounds__(512) void k_sweep_diag(Ctx c0) {
  const Ctx c = chain_view(c0);      // chain blockIdx.z of the batch
  TIMELINE(c, 4);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Dims& d = c.d;
  const int P = d.P, A = d.A, K = d.K, M = d.M, MD = d.MD, LG = d.LG;
  const int tid = threadIdx.x, nthr = blockDim.x;
  Dyn* dyn = c.dyn;
  double* red = smem;                          // 16
  double* sH = red + 16;                       // A x A : multivariate model: the blocks are scalars, H_{b,a} = sH[b A + a] I
  int* htab = (int*)(sH + A * A);              // A x A : element offset of block (b, a) in H
  int* sdir = htab + A * A;
  const uint32_t slot = dyn->slot;
  const uint32_t mask = c.mask;
  const double beta = dyn->beta;
  const double f = beta / dyn->sigma2;
  if (tid == 0) { dyn->iter_hyper = dyn->iter; dyn->slot_hyper = slot; }
#ifdef DG_STAMPS
#define DST(k) do { if (tid == 0) dyn->stamps[40 + (k)] = clock64(); } while (0)
#else
#define DST(k) do { } while (0)
#endif
  DST(0);
  const int n_phi = ((mask & U_PHI) && MD > 1) ? K * M : 0;
  const int n_nu = (mask & U_NU) ? K : 0;
  const int n_steps = n_phi + n_nu;
  for (int x = tid; x < A * A; x += nthr) htab[x] = hrow(d, x / A, x % A) * LG;
  for (int x = tid; x < n_steps + 2; x += nthr) sdir[x] = step_dir(d, min(x, max(n_steps - 1, 0)), n_phi);
  const int p = min(tid >> 3, P - 1), g = tid & 7;
  const bool live = (tid >> 3) < P;
  double sig_g = (mask & U_SIGMA) ? c.gstd[hyper_gstd_count(d)] : 0.0;
  uint32_t tt_step0 = dyn->tt_step;
  // (both are needed by one lane at the very end: requested here, with the rest of the set-up loads, or they are two trips to
  //  memory after the last step)
  asm volatile("" : "+v"(sig_g), "+v"(tt_step0));
  double r[DG_RPL], hq[DG_RPL], cd[DG_RPL], lz[DG_RPL], th[DG_RPL], tv[DG_RPL];
#pragma unroll
  for (int j = 0; j < DG_RPL; ++j) {
    const int b = min(g + 8 * j, A - 1);
    const bool on = g + 8 * j < A;
    const int e = b * P + p;
    const double rv = c.rvec[e], hv = c.hq[e], cv = c.Cmat[(size_t)b * P * P + (size_t)p * (P + 1)], lv = c.Lz[e];
    const double t0 = c.theta[(size_t)full_dir(d, b) * P + p], t1 = c.tvec[e];
    r[j] = on ? rv : 0.0; hq[j] = on ? hv : 0.0; cd[j] = on ? cv : 0.0; lz[j] = on ? lv : 0.0; th[j] = on ? t0 : 0.0; tv[j] = on ? t1 : 0.0;
  }
  __syncthreads();
  DST(1);
  // Multivariate model (G_i = I): every block of H is a multiple of the identity, so the A^2 scalars are read ONCE into LDS
  // and a step's H_{b,a} is an LDS read instead of a request to L2 two steps ahead (the steps of this kernel were bound by
  // that latency: 36 steps took 39 us)
  constexpr bool scalar_blocks = SCALAR_BLOCKS;      // (the launcher passes d.mv)
  if (scalar_blocks) {
    for (int x = tid; x < A * A; x += nthr) sH[x] = c.H[(size_t)htab[x]];
    __syncthreads();
  }
  // H was written by another XCD (k_pg_reduce): touch it once (one 4-byte load per 128-byte line, fire and forget) so
  // that the per-step requests are L2 hits; they are issued two steps ahead (three register sets, compile-time indexed)
  if (n_steps > 0 && !scalar_blocks) {
    int w0 = 0;
    const size_t nl = ((size_t)d.R * LG * 8 + 127) / 128;
    for (size_t x = tid; x < nl; x += nthr) {
      const uint32_t o = (uint32_t)(x * 128);
      asm volatile("global_load_dword %0, %1, %2" : "+v"(w0) : "v"(o), "s"(c.H));
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(w0) :: "memory");
  }
  DST(2);
  double hs[3][DG_RPL];
  auto fetch = [&](auto which, int a) {       // H_{b,a}[p] for this lane's directions
    constexpr int Q = decltype(which)::value;
    if constexpr (scalar_blocks) {
#pragma unroll
      for (int j = 0; j < DG_RPL; ++j) hs[Q][j] = sH[min(g + 8 * j, A - 1) * A + a];
    } else {
#pragma unroll
      for (int j = 0; j < DG_RPL; ++j) hs[Q][j] = c.H[(size_t)htab[min(g + 8 * j, A - 1) * A + a] + p];
    }
  };
  // a: this step's direction, a2: the direction two steps ahead (its H column is requested now).  Branch-free: the draw is
  // evaluated for all of a lane's slots and the step's slot selected (a taken branch costs ~40 clk here, eight of them a step
  // were half of it).
  auto step = [&](int a, int a2, auto which) {
    constexpr int Q = decltype(which)::value;
    fetch(std::integral_constant<int, (Q + 2) % 3>{}, a2);
    const int owner = a & 7, js = a >> 3;
    const bool mine_lane = g == owner;
    double dsel = 0.0;
#pragma unroll
    for (int j = 0; j < DG_RPL; ++j) {
      const double nw = cd[j] * (f * (r[j] + hq[j])) + lz[j];
      const bool mine = mine_lane && j == js;
      dsel = mine ? nw - th[j] : dsel;
      th[j] = mine ? nw : th[j];
    }
    dsel = dpp_add<0xB1>(dsel);
    dsel = dpp_add<0x4E>(dsel);
    const double delta = dpp_add<0x141>(dsel);           // broadcast to the 8 lanes of the coordinate
#pragma unroll
    for (int j = 0; j < DG_RPL; ++j) {
      const double v = hs[Q][j] * delta;
      r[j] = (g + 8 * j < A) ? r[j] - v : r[j];
      hq[j] = (mine_lane && j == js) ? hq[j] + v : hq[j];
    }
  };
  if (n_steps > 0) {
    using Q0 = std::integral_constant<int, 0>;
    using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>;
    // the directions of the steps travel in scalar registers, read from LDS three steps ahead of their use
    auto dir_at = [&](int s) { return __builtin_amdgcn_readfirstlane(sdir[min(s, n_steps + 1)]); };
    int a0 = dir_at(0), a1 = dir_at(1), a2 = dir_at(2), a3 = dir_at(3), a4 = dir_at(4);
    fetch(Q0{}, a0);
    fetch(Q1{}, a1);
    int s = 0;
    for (; s + 2 < n_steps; s += 3) {
      const int b0 = dir_at(s + 5), b1 = dir_at(s + 6), b2 = dir_at(s + 7);
      step(a0, a2, Q0{}); step(a1, a3, Q1{}); step(a2, a4, Q2{});
      a0 = a3; a1 = a4; a2 = b0; a3 = b1; a4 = b2;
    }
    if (s < n_steps) { step(a0, a2, Q0{}); ++s; }
    if (s < n_steps) { step(a1, a3, Q1{}); ++s; }
  }
  DST(3);
  // ---------------- sigma^2 (updateSigma, UpdateSigma.h:127-165 MV) ---------------------------------
  if (mask & U_SIGMA) {
    double acc = 0.0;                                       // RSS = YY - sum_a theta_a'(t_a + r_a)
    if (live) {
#pragma unroll
      for (int j = 0; j < DG_RPL; ++j) acc += th[j] * (tv[j] + r[j]);
    }
    if (d.D > 0)
      for (int x = tid; x < c.nblk_curve; x += nthr) acc -= c.yyp_part[x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      double qs = 0.0;
      for (int w = 0; w < nthr / 64; ++w) qs += red[w];
      const double rss = (d.D > 0) ? -qs : (c.YY - qs);
      const bool tempered = (tt_step0 != 0);
      const double bb = (tempered ? (beta / 2) * rss : 0.5 * rss) + c.h.beta_0;
      const double s2 = 1.0 / (sig_g * (1.0 / bb));
      dyn->sigma2 = s2;
      dyn->rss = rss;
      c.c_sigma[slot] = s2;
    }
  } else if (tid == 0) {
    c.c_sigma[slot] = dyn->sigma2;
  }
  DST(4);
  // ---------------- publish theta and its chain slots -------------------------------------------
  double* s_nu = c.c_nu + (size_t)slot * K * P;
  double* s_phi = c.c_Phi + (size_t)slot * K * P * M;
  if (live) {
#pragma unroll
    for (int j = 0; j < DG_RPL; ++j) {
      const int b = g + 8 * j;
      if (b < A) {
        const int jj = b / MD, mt = b - jj * MD;
        c.theta[(size_t)(jj * (M + 1) + mt) * P + p] = th[j];
        if (mt == 0) s_nu[jj + (size_t)K * p] = th[j];
        else s_phi[jj + (size_t)K * (p + (size_t)P * (mt - 1))] = th[j];
      }
    }
  }
  if (MD == 1) {
    __syncthreads();
    for (int x = tid; x < K * P * M; x += nthr) {
      const int k = x % K, pm = x / K, pp = pm % P, m = pm / P;
      s_phi[x] = c.theta[(size_t)(k * (M + 1) + m + 1) * P + pp];
    }
  }
}

__device__ inline const double* ptr_off(const double* base, uint32_t byte_off) {   // uniform base + 32-bit lane offset
  return (const double*)((const char*)base + byte_off);
}

// Software-managed prefetch of the chain wave.  The loads below are inline assembly, so the compiler neither tracks them nor
// inserts s_waitcnt for them (its own placement drained the queue every step); swc_wait_* are the matching waits: "at most N
// younger loads may still be in flight" -- vmcnt retires in issue order, and the chain wave issues the same loads in the same
// order at every step.  The loaded registers pass through the wait as read-write operands, so no use can be scheduled above it.
// The destination of a load is a read-write operand too: the register stays allocated to the variable across the load (the
// compiler believes inline assembly completes synchronously; a write-only destination that is dead until its next definition
// could be handed out as a temporary while the load is still in flight).
template <int BW> struct SweepH { v2d h[BW + 1]; };

// ---------------------------------------------------------------------------------------------
// k_sweep_chain: the register-resident sweep with the dependent chain in ONE wave (round 3; replaces k_sweep_fast, whose
// step cost ~2000 clk: two cross-wave hand-offs through LDS flags and a 14-wave barrier sat on the chain of every step).
//
// Wave 0 is the chain.  Lane (p, h), p = lane >> 1, h = lane & 1.  Step st with direction a = a_st:
//   mat-vec   theta_a <- C_a rhs + L_a z_a      lane (p, h) holds C_a(p, 16 h .. 16 h + 15) in registers (prefetched two
//             steps ahead from L2), reads rhs(16 h ..) from LDS (broadcast), 16 FMAs on four accumulators, one DPP add
//             joins the halves; delta_st -> LDS
//   band dot  the h = 0 lanes hold r of the direction of step st + 1, the h = 1 lanes r of the direction of step st + 2:
//             r -= H_{., a} delta_st from prefetched rows of H; the h = 0 lanes publish the next rhs; then the h = 1 value
//             moves to the h = 0 lane (DPP) and the h = 1 lanes pick up the row of step st + 3
// so both hand-offs of a step (delta -> band rows, rhs -> mat-vec rows) are LDS write / read pairs of the SAME wave: LDS
// executes a wave's operations in order, there is no flag, no poll and no barrier on the chain.
// The other waves ("row threads", thread 64 + rk P + p owns element p of the direction updated at step rk) do what is
// off the chain: r_rk -= H delta_s for s <= rk - 3 (the chain applies the last two deltas itself), hand the row over, and
// the row's term of the residual sum of squares, delta'(H_aa delta - 2 r_a), one step late.
// Hand-offs between the chain and the row threads carry their own validity: every slot (delta of step s, row of rank rk,
// r_a before its step) is written ONCE per launch into a slot of its own that starts as a NaN with a payload no arithmetic
// produces (SW_SENT); a reader that finds the sentinel reads again (bounded: a spin that runs out sets status bit 2 and goes
// on, so the grid always drains).  No ordering between different LDS locations is assumed anywhere.
// ---------------------------------------------------------------------------------------------
constexpr unsigned long long SW_SENT = 0x7FF8DEADBEEF5A5AULL;
constexpr int SWC_SPIN_LIMIT = 1 << 15;
constexpr unsigned SWC_STATUS_SPIN = 4u;      // status bit of a hand-off spin that ran out (bfmmm_capi.hip::run_impl reports it by name)
constexpr int SWC_THREADS = 448;            // chain wave + A ceil(P / 2) <= 384 row threads (two rows each): two waves per SIMD, 256 VGPRs

__device__ inline double lds_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline bool is_sent(double v) { return (unsigned long long)__double_as_longlong(v) == SW_SENT; }
__device__ inline double sw_sent() { return __longlong_as_double((long long)SW_SENT); }
template <int CTRL>
__device__ inline double dpp_get(double v) {      // the value of another lane of the quad
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

struct SwcC { v2d v[8]; };
template <int N>
__device__ inline void swc_wait_c(SwcC& s) {      // at most N younger loads still in flight; the registers pass through
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(s.v[0]), "+v"(s.v[1]), "+v"(s.v[2]), "+v"(s.v[3]), "+v"(s.v[4]), "+v"(s.v[5]), "+v"(s.v[6]), "+v"(s.v[7]) : "n"(N));
}
template <int N, int BW>
__device__ inline void swc_wait_h(SweepH<BW>& s) {
  if constexpr (BW == 0) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(s.h[0]) : "n"(N));
  if constexpr (BW == 1) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(s.h[0]), "+v"(s.h[1]) : "n"(N));
  if constexpr (BW == 2) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(s.h[0]), "+v"(s.h[1]), "+v"(s.h[2]) : "n"(N));
  if constexpr (BW == 3) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(s.h[0]), "+v"(s.h[1]), "+v"(s.h[2]), "+v"(s.h[3]) : "n"(N));
  if constexpr (BW == 4) asm volatile("s_waitcnt vmcnt(%5)" : "+v"(s.h[0]), "+v"(s.h[1]), "+v"(s.h[2]), "+v"(s.h[3]), "+v"(s.h[4]) : "n"(N));
  if constexpr (BW == 5) asm volatile("s_waitcnt vmcnt(%6)" : "+v"(s.h[0]), "+v"(s.h[1]), "+v"(s.h[2]), "+v"(s.h[3]), "+v"(s.h[4]), "+v"(s.h[5]) : "n"(N));
}
__device__ inline void sweep_ld16v(v2d& r, const double* sbase, uint32_t voff) {
  asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(r) : "v"(voff), "s"(sbase));
}

// Step tables of k_sweep_chain, built once per (MD, mask) of a run (bfmmm_capi.hip::run_impl), shared by the chains of a batch:
//   ent [2 (A + 2)] int4 : what lane half h of the chain wave needs for step st (entry 2 st + h):
//                          .x byte offset in H2 of block (a_{st + 1 + h}, a_st), .y byte offset of C_{a_st} in Cmat, .z a_st P
//   hstp[A x A]          : hstp[b A + s] = byte offset in H2 of block (b, a_s), a_s = direction of step s
// (their integer divisions cost the sweep kernel 1.6 us of its set-up when it built them itself)
size_t sweep_tab_ints(int A) { return (size_t)A * A + 8 * ((size_t)A + 2); }
__host__ __device__ inline int sweep_n_phi(const Dims& d, uint32_t mask) { return ((mask & U_PHI) && d.MD > 1) ? d.K * d.M : 0; }
__host__ __device__ inline int sweep_n_nu(const Dims& d, uint32_t mask) { return (mask & U_NU) ? d.K : 0; }

__global__ void k_sweep_tables(Ctx c, int* tab) {
  const Dims& d = c.d;
  const int A = d.A, P = d.P, W = 2 * d.BW + 2;
  const int n_phi = sweep_n_phi(d, c.mask), n_steps = n_phi + sweep_n_nu(d, c.mask);
  int4* ent = (int4*)tab;
  int* hstp = tab + 8 * (A + 2);
  for (int x = threadIdx.x; x < 2 * (A + 2); x += blockDim.x) {
    const int st = x >> 1, hh = x & 1;
    const int a = step_dir(d, min(st, max(n_steps - 1, 0)), n_phi), bb = step_dir(d, min(st + 1 + hh, max(n_steps - 1, 0)), n_phi);
    ent[x] = make_int4(hrow(d, bb, a) * P * W * 8, a * P * P * 8, a * P, 0);
  }
  for (int x = threadIdx.x; x < A * A; x += blockDim.x)
    hstp[x] = hrow(d, x / A, step_dir(d, min(x % A, max(n_steps - 1, 0)), n_phi)) * P * W * 8;
}
void launch_sweep_tables(const Ctx& c, hipStream_t st) { hipLaunchKernelGGL(k_sweep_tables, dim3(1), dim3(256), 0, st, c, (int*)c.sweep_tab); }

// direction that owns rank rk: ranks follow the order of the steps (Phi sweep j outer, m inner, then the nu sweep), the
// directions a sweep does not update come last
__device__ inline int rank_dir(const Dims& d, int rk, int n_phi, int n_nu) {
  const int n_steps = n_phi + n_nu;
  if (rk < n_steps) return step_dir(d, rk, n_phi);
  const int x = rk - n_steps;
  if (n_phi == 0 && n_nu == 0) return x;                       // nothing is updated: rank = direction
  if (n_nu == 0) return x * d.MD;                               // the nu directions of a Phi-only sweep
  if (d.MD == 1) return x;                                      // (no Phi directions at all)
  const int jx = x / (d.MD - 1);                                // the Phi directions of a nu-only sweep
  return jx * d.MD + 1 + (x - jx * (d.MD - 1));
}

template <int BW>
__global__ __launch_bounds__(SWC_THREADS) void k_sweep_chain(Ctx c0) {
  const Ctx c = chain_view(c0);      // chain blockIdx.z of the batch
  TIMELINE(c, 4);
#ifdef BFMMM_TIMELINE
  if (threadIdx.x == 0) { unsigned id; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id)); c.dyn->stamps[38] = ((c.dyn->stamps[38] << 4) | (id & 0xf)) & 0xFFFFFFFFFULL; }
#endif
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Dims& d = c.d;
  const int P = d.P, A = d.A, K = d.K, M = d.M, MD = d.MD;
  constexpr int W = 2 * BW + 2;              // doubles per row of an H2 block
  constexpr int DLS = 32 + 2 * BW + 2;       // one delta slot: BW zero pads | 32 | BW + 2 zero pads
  constexpr int NC = 8, NH = BW + 1;         // loads per step of the chain wave: C pieces, H row pieces
  const int tid = threadIdx.x, nthr = blockDim.x;
  Dyn* dyn = c.dyn;
  const int AP = A * P, PH = (P + 1) >> 1;
  const int APe = (AP + 1) & ~1;             // (16-byte alignment of what follows)
  double* th = smem;                         // A x P   theta, direction-major (theta_0, then the new values)
  double* lzs = th + APe;                    // A x P   L_a z_a
  double* hqs = lzs + APe;                   // A x P   H_aa theta_a(0)
  double* pick = hqs + APe;                  // A x P   rank-major: r of rank rk with the deltas of the steps <= rk - 3 applied
  double* rbef = pick + APe;                 // A x P   rank-major: r of rank rk just before its step
  double* rhs = rbef + APe;                  // 32 (zero beyond P)
  double* dl = rhs + 32;                     // A slots of DLS: delta of step s
  double* red = dl + A * DLS;                // 16
  int4* ent = (int4*)(red + 16);             // 2 (A + 2): what lane half h of the chain needs for step st
  int* hstp = (int*)(ent + 2 * (A + 2));     // A x A : hstp[b A + s] = byte offset of block (b, a_s) in H2, a_s = direction of step s
  const uint32_t mask = c.mask;
  const int n_phi = sweep_n_phi(d, mask), n_nu = sweep_n_nu(d, mask);
  const int n_steps = n_phi + n_nu;
  const bool chainw = tid < 64;              // wave-uniform
#ifndef SWC_NOPRIO
  if (chainw) __builtin_amdgcn_s_setprio(3);
#endif
  // ---- ONE round of global loads: the run's step tables, the iteration's scalars, and every thread's rows ----
  const int4* gent = (const int4*)c.sweep_tab;
  const int* ghstp = c.sweep_tab + 8 * (A + 2);
  // row thread 64 + rk LRK + pp (pp < PH) owns rows p0 = 2 pp and p0 + 1 of the direction updated at step rk; a rank takes
  // LRK = 4, 8 or 16 lanes, so that the threads of a rank sit in ONE 16-lane DPP row (the band entries below the diagonal come
  // from the neighbouring threads' registers, see the row threads' loads)
  const int lrk_log = (PH <= 4) ? 2 : (PH <= 8) ? 3 : 4, LRK = 1 << lrk_log;
  const int e2i = max(tid - 64, 0);
  const int ppr = e2i & (LRK - 1);
  const bool isB = tid >= 64 && (e2i >> lrk_log) < A && ppr < PH;
  const int rk = min(e2i >> lrk_log, A - 1), p0 = 2 * min(ppr, PH - 1);
  const bool two = p0 + 1 < P;               // (odd P: the last thread of a rank owns one row)
  const int p1 = two ? p0 + 1 : p0;
  const int b = rank_dir(d, rk, n_phi, n_nu);
  const int fd = full_dir(d, b);
  const int eb = b * P + p0, er = rk * P + p0;     // element of the direction-major / rank-major vectors
  // the chain wave: its first table entries straight into registers, so that its first C / H loads are in flight during the set-up
  const int hch = (tid >> 1) & 1;
  int4 ge0 = make_int4(0, 0, 0, 0), ge1 = ge0, ge2 = ge0;
  if (chainw && n_steps > 0) { ge0 = gent[hch]; ge1 = gent[2 + hch]; ge2 = gent[2 * min(2, n_steps + 1) + hch]; }
  const uint32_t slot = dyn->slot;
  const double beta = dyn->beta;
  const double sig2 = dyn->sigma2;
  const double sig_g = (mask & U_SIGMA) ? c.gstd[hyper_gstd_count(d)] : 0.0;
  double r_0 = 0.0, r_1 = 0.0, rss_acc = 0.0;      // rss_acc: this thread's share of RSS - YY
  double hq_0 = 0.0, hq_1 = 0.0, tv_0 = 0.0, tv_1 = 0.0, t_0 = 0.0, t_1 = 0.0, l_0 = 0.0, l_1 = 0.0;
  if (!chainw) {
    r_0 = c.rvec[eb]; r_1 = c.rvec[b * P + p1];
    hq_0 = c.hq[eb]; hq_1 = c.hq[b * P + p1]; tv_0 = c.tvec[eb]; tv_1 = c.tvec[b * P + p1];
    t_0 = c.theta[(size_t)fd * P + p0]; t_1 = c.theta[(size_t)fd * P + p1]; l_0 = c.Lz[eb]; l_1 = c.Lz[b * P + p1];
  }
  // (the tables go through registers: two entries of each kind per thread cover A <= 21; the loops take the rest)
  const int n_ent = 2 * (A + 2), n_hs = A * A;
  int4 ge_a = make_int4(0, 0, 0, 0);
  int gh_a = 0, gh_b = 0;
  if (tid < n_ent) ge_a = gent[tid];
  if (tid < n_hs) gh_a = ghstp[tid];
  if (tid + nthr < n_hs) gh_b = ghstp[tid + nthr];
  if (tid == 0) { dyn->iter_hyper = dyn->iter; dyn->slot_hyper = slot; }
  const double f = beta / sig2;
  // ---- LDS initialisation while the loads are in flight
  if (tid < 32) rhs[tid] = 0.0;
  for (int x = tid; x < A * DLS; x += nthr) {
    const int k = x % DLS;
    dl[x] = (k >= BW && k < BW + P) ? sw_sent() : 0.0;
  }
  if (tid < n_ent) ent[tid] = ge_a;
  for (int x = tid + nthr; x < n_ent; x += nthr) ent[x] = gent[x];
  if (tid < n_hs) hstp[tid] = gh_a;
  if (tid + nthr < n_hs) hstp[tid + nthr] = gh_b;
  for (int x = tid + 2 * nthr; x < n_hs; x += nthr) hstp[x] = ghstp[x];
  if (isB) {
    th[eb] = t_0; lzs[eb] = l_0; hqs[eb] = hq_0;
    rss_acc = -(t_0 * (tv_0 + r_0));       // RSS(theta_0) = YY - theta_0'(t + r_0)
    // ranks 0 .. 2 (no delta to apply first) and the directions that are not updated are handed over at once
    const bool now = (rk <= 2 || rk >= n_steps);
    pick[er] = now ? r_0 : sw_sent();
    rbef[er] = (rk == 0) ? r_0 : sw_sent();
    if (two) {
      th[eb + 1] = t_1; lzs[eb + 1] = l_1; hqs[eb + 1] = hq_1;
      rss_acc -= t_1 * (tv_1 + r_1);
      pick[er + 1] = now ? r_1 : sw_sent();
      rbef[er + 1] = (rk == 0) ? r_1 : sw_sent();
    }
  }
  TSTAMP0(c, 28);
  // the chain wave's per-lane constants and its first loads (C and H of steps 0 and 1) before the barrier
  const int pp = tid >> 2, g = tid & 3, h = hch;
  const int pbl = 2 * pp + (tid & 1), pb = min(pbl, P - 1);
  const bool wr = (h == 0) && (pbl < P);
  const int ppc = min(2 * pp, max(P - 2, 0));           // first row of the pair, clamped (a pair never leaves its matrix row)
  uint32_t coff[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) coff[u] = (uint32_t)(ppc + P * min(8 * g + u, P - 1)) * 8u;     // C(q, p), C(q, p + 1) = C(p, q), C(p + 1, q)
  const bool sel_y = (tid & 1) || (2 * pp < P && ppc < 2 * pp);      // odd P: the last row sits in the SECOND slot of the clamped pair
  uint32_t hoffk[NH];
#pragma unroll
  for (int k = 0; k < NH; ++k) hoffk[k] = (uint32_t)(k * P + pb) * 16u;      // piece k of row pb (h2_index)
  auto issueC = [&](SwcC& s, int cbase) {
#ifndef SWC_NO_LOADS
#pragma unroll
    for (int u = 0; u < NC; ++u) sweep_ld16v(s.v[u], c.Cmat, (uint32_t)cbase + coff[u]);
#endif
  };
  auto issueH = [&](SweepH<BW>& s, int hbase) {
#ifndef SWC_NO_LOADS
#pragma unroll
    for (int k = 0; k < NH; ++k) sweep_ld16v(s.h[k], c.H2, (uint32_t)hbase + hoffk[k]);
#endif
  };
  SwcC c0s = {}, c1s = {};
  SweepH<BW> h0s = {}, h1s = {};
  if (chainw && n_steps > 0) {
    // (the compiler waits for ge0 / ge1 here; everything issued above is older and already on its way)
    // the issue order of the steady state: C(st), H(st), C(st + 1), H(st + 1)
    // (s_nop 13 / 14 and 11 / 12 below are MARKERS for tools/isa_check.py, which verifies in the shipped code object that no
    //  instruction touches a prefetch destination between its load and the counted wait: tests/test_isa_sweep_chain.py)
    asm volatile("s_nop 13");
    issueC(c0s, ge0.y); issueH(h0s, ge0.x); issueC(c1s, ge1.y); issueH(h1s, ge1.x);
    asm volatile("s_nop 14");
  }
  __syncthreads();
#ifdef BFMMM_TIMELINE
  if (tid == 0) dyn->stamps[24] = wall_clock64();
  unsigned long long n_spin = 0;
#endif
  if (n_steps > 0 && chainw) {
    // ================= the chain wave =================
    // mat-vec role of lane l: rows 2 pp, 2 pp + 1 (pp = l >> 2), columns q = 8 g .. 8 g + 7 (g = l & 3)
    // band role of lane l   : row pb = 2 pp + (l & 1), rank half h = (l >> 1) & 1
    asm volatile("s_nop 11");
    int4 e0 = ge0, e1 = ge1, e2 = ge2;
    // rank 0 is complete: its rhs; the h = 0 lanes then hold rank 1, the h = 1 lanes rank 2
    {
      const double r0 = pick[pb], hq0 = hqs[e0.z + pb];
      if (wr) rhs[pb] = f * (r0 + hq0);
    }
    double r = pick[min((1 + h) * P + pb, AP - 1)];
    double lz0 = lzs[e0.z + pb], th0 = th[e0.z + pb];
    double hq1 = hqs[e1.z + pb];                    // H_aa theta_a of the direction of step st + 1
    asm volatile("" ::: "memory");
    // (LAST: the odd last step behind the pair loop issues no further prefetch -- nothing follows it)
    auto step = [&](auto last_tag, int st, SwcC& cs, SweepH<BW>& hs) {
      constexpr bool LAST = decltype(last_tag)::value;
      // ---- mat-vec operands first: rhs was written at the end of the previous step
      const v2d* rv = (const v2d*)(rhs + 8 * g);
      v2d x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = rv[u];
      // ---- small reads for later in this step / the next ones (no address here depends on a read of this step)
      const int4 e3 = ent[2 * min(st + 3, n_steps + 1) + h];
      const double lz1 = lzs[e1.z + pb], th1 = th[e1.z + pb];
      const double hq2 = hqs[e2.z + pb];
      // the row the h = 1 lanes take over for this step's band dot: rank st + 2, which the row threads hand over with the
      // deltas of the steps <= st - 1 applied (published a whole step ago); the read is checked just before its use
#ifdef SWC_NO_HELPERS
      const bool want_pick = false;
#else
      const bool want_pick = (st >= 1) && (st + 2 < n_steps);
#endif
      const double* pk_ptr = pick + min((st + 2) * P + pb, AP - 1);
      double pk = lds_ld(pk_ptr);
      swc_wait_c<NH + NC + NH>(cs);
      // cs.v[u] = (C(p, q), C(p + 1, q)), q = 8 g + u: four chains
      v2d s0 = cs.v[0] * x[0].x, s1 = cs.v[1] * x[0].y;
#pragma unroll
      for (int u = 1; u < 4; ++u) { s0 += cs.v[2 * u] * x[u].x; s1 += cs.v[2 * u + 1] * x[u].y; }
      if constexpr (!LAST) issueC(cs, e2.y);
      const v2d ss = s0 + s1;
      // sum over the four column groups of the quad (every lane of the quad ends with the same two sums), then this lane's row
      double a_x = ss.x, a_y = ss.y;
      a_x += dpp_get<0xB1>(a_x); a_y += dpp_get<0xB1>(a_y);       // quad_perm [1, 0, 3, 2]
      a_x += dpp_get<0x4E>(a_x); a_y += dpp_get<0x4E>(a_y);       // quad_perm [2, 3, 0, 1]
      const double acc = sel_y ? a_y : a_x;
      const double nw = acc + lz0;
      const double dlt = nw - th0;
      double* dls = dl + st * DLS;
      if (wr) { dls[BW + pb] = dlt; th[e0.z + pb] = nw; }
      asm volatile("" ::: "memory");
      // ---- band dot: the rows of the next two directions take delta_st
      double dv[W];
#pragma unroll
      for (int k = 0; k < W; ++k) dv[k] = dls[pb + k];
      if (h == 1 && want_pick) {
        int spins = 0;
#pragma nounroll
        while (is_sent(pk)) {
          if (++spins > SWC_SPIN_LIMIT) {       // (the extra memory operation would shift the counted waits: drain)
            atomicOr(&dyn->status, SWC_STATUS_SPIN);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            break;
          }
          pk = lds_ld(pk_ptr);
#ifdef BFMMM_TIMELINE
          ++n_spin;
#endif
        }
        r = pk;
      }
      swc_wait_h<(LAST ? 0 : NC) + NH + NC, BW>(hs);       // younger loads in flight: C(st + 2) (not issued by the last step), H(st + 1), C(st + 1)
      double v0 = hs.h[0].x * dv[0], v1 = hs.h[0].y * dv[1];
#pragma unroll
      for (int k = 1; k <= BW; ++k) { v0 += hs.h[k].x * dv[2 * k]; v1 += hs.h[k].y * dv[2 * k + 1]; }      // last .y is the zero pad
      if constexpr (!LAST) issueH(hs, e2.x);
      r -= (v0 + v1);
      if (wr && st + 1 < n_steps) { rhs[pb] = f * (r + hq1); rbef[(st + 1) * P + pb] = r; }
      asm volatile("" ::: "memory");
      // ---- the h = 1 value (rank st + 2, delta_st applied) moves to the h = 0 lane; the h = 1 lanes take the next row over
      //      at the next step
      const double rsw = dpp_get<0x4E>(r);            // quad_perm [2, 3, 0, 1]: lane l ^ 2 (same row, other half)
      if (h == 0) r = rsw;
      e0 = e1; e1 = e2; e2 = e3; lz0 = lz1; th0 = th1; hq1 = hq2;
    };
    // (pairs of steps in the loop and an odd last step behind it -- not `if (st + 1 < n_steps)` inside the loop: the control-flow
    //  graph then has no path "first half, skipped second half, first half again", which never runs but which a static check of
    //  the counted waits would have to assume: tools/isa_check.py)
    int st = 0;
    for (; st + 1 < n_steps; st += 2) {
      step(std::false_type{}, st, c0s, h0s);
      step(std::false_type{}, st + 1, c1s, h1s);
    }
    if (st < n_steps) step(std::true_type{}, st, c0s, h0s);
    // drain the prefetches of the (clamped) tail before their registers are reused
    swc_wait_c<0>(c0s); swc_wait_c<0>(c1s);
    swc_wait_h<0, BW>(h0s); swc_wait_h<0, BW>(h1s);
    asm volatile("s_nop 12");
#ifdef BFMMM_TIMELINE
    if (tid == 2) { dyn->stamps[25] = wall_clock64(); dyn->stamps[26] = n_spin; }
#endif
  } else if (n_steps > 0) {
    // ================= the row threads =================
    const bool live = isB && rk < n_steps;
    int rk_hi = live ? rk : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rk_hi = max(rk_hi, __shfl_xor(rk_hi, o, 64));
    int rk_lo = live ? rk : (1 << 20);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rk_lo = min(rk_lo, __shfl_xor(rk_lo, o, 64));
    const int* hs_b = hstp + b * A;                  // hs_b[s] = byte offset of block (b, a_s) in H2 (= twice its offset in H)
    // The rows of H_{b, a_s} come from the band-packed array H (G(p, p + d) at [d P + p]: half the bytes of the H2 rows; the sweep
    // is bound by the bytes one compute unit can pull through its L1): a thread loads the UPPER band entries of its two rows, one
    // 16-byte piece per diagonal, and takes the entries below the diagonal -- G(p, p - d) = G(p - d, p), which the thread owning
    // row p - d has loaded -- from its neighbours' registers on the DPP path (the threads of a rank share a 16-lane row).
    struct H2r { v2d u[BW + 1]; };                   // u[d] = (G(p0, p0 + d), G(p0 + 1, p0 + 1 + d))
    // (every lane loads at every step of its wave: predicating the loads on "the step is one of this lane's" made the kernel
    //  1.6 us slower -- the compiler then waits for each conditional group on its own)
    auto is_mine = [&](int s) { return live && (s <= rk - 3 || s == rk); };
    auto loadH = [&](H2r& s, int off) {
#ifndef SWC_HELPER_NOLOAD
      const char* blk = (const char*)c.H + ((uint32_t)off >> 1);
#pragma unroll
      for (int dd = 0; dd <= BW; ++dd) s.u[dd] = *(const v2d*)(blk + (size_t)(dd * P + p0) * 8);
#endif
    };
    // (va, vb) = (H_{b, a_s} delta)[p0], [p0 + 1] with dv[k] = delta[p0 - BW + k]
    auto band2 = [&](const H2r& hc, const double (&dv)[W + 1], double& va, double& vb) {
      double a0 = hc.u[0].x * dv[BW], a1 = 0.0, b0 = hc.u[0].y * dv[BW + 1], b1 = 0.0;
#pragma unroll
      for (int dd = 1; dd <= BW; ++dd) {
        // lower entries: row p0 takes G(p0 - dd, p0), row p0 + 1 takes G(p0 + 1 - dd, p0 + 1)
        double l0, l1;
        if (dd & 1) {
          constexpr int dummy = 0; (void)dummy;
          const int sh0 = (dd + 1) >> 1, sh1 = (dd - 1) >> 1;
          const double y = hc.u[dd].y, x = hc.u[dd].x;
          const double g0 = (sh0 == 1) ? dpp_get<0x111>(y) : (sh0 == 2) ? dpp_get<0x112>(y) : dpp_get<0x113>(y);
          const double g1 = (sh1 == 0) ? x : (sh1 == 1) ? dpp_get<0x111>(x) : dpp_get<0x112>(x);
          l0 = (ppr >= sh0) ? g0 : 0.0;
          l1 = (ppr >= sh1) ? g1 : 0.0;
        } else {
          const int sh = dd >> 1;
          const double y = hc.u[dd].y, x = hc.u[dd].x;
          const double g0 = (sh == 1) ? dpp_get<0x111>(x) : dpp_get<0x112>(x);
          const double g1 = (sh == 1) ? dpp_get<0x111>(y) : dpp_get<0x112>(y);
          l0 = (ppr >= sh) ? g0 : 0.0;
          l1 = (ppr >= sh) ? g1 : 0.0;
        }
        a0 += hc.u[dd].x * dv[BW + dd]; a1 += l0 * dv[BW - dd];
        b0 += hc.u[dd].y * dv[BW + 1 + dd]; b1 += l1 * dv[BW + 1 - dd];
      }
      va = a0 + a1; vb = b0 + b1;
    };
    // The steps the WAVE walks (wave-uniform): 0 .. rk_hi - 3 (some lane's lagging update), then rk_lo .. rk_hi (some lane's
    // own term).  Every lane loads the rows of H_{b, a_s} for every step of the wave, one step ahead, so that the two register
    // sets alternate without a copy; a lane uses the result when the step is one of its own: s <= rk - 3 or s == rk.
    auto next_w = [&](int s) { return (s + 1 <= rk_hi - 3 || s + 1 >= rk_lo) ? s + 1 : rk_lo; };
    auto process = [&](int s, const H2r& hc) {
      const bool mine = is_mine(s);
      const double* dls = dl + s * DLS;
      {
        int spins = 0;
#pragma nounroll
        while (is_sent(lds_ld(dls + BW))) {
#ifdef SWC_SLEEP
          __builtin_amdgcn_s_sleep(SWC_SLEEP);
#else
          __builtin_amdgcn_s_sleep(1);
#endif
          if (++spins > SWC_SPIN_LIMIT) { atomicOr(&dyn->status, SWC_STATUS_SPIN); break; }
        }
      }
      asm volatile("" ::: "memory");      // (compiler ordering only: an acquire fence would also wait for this wave's loads in flight)
      double dv[W + 1], va, vb;
      int tries = 0;
#pragma nounroll
      do {
#pragma unroll
        for (int k = 0; k <= W; ++k) dv[k] = lds_ld(dls + p0 + k);
        band2(hc, dv, va, vb);
        // a delta slot still holding the sentinel makes the sum a NaN: read again (the first element was seen, the rest of
        // the chain's one store instruction follows within cycles)
        bool bad = false;
        if (va != va || vb != vb) {
#pragma unroll
          for (int k = 0; k <= W; ++k) bad = bad || is_sent(dv[k]);
        }
        if (!__builtin_amdgcn_ballot_w64(mine && bad)) break;
      } while (++tries < SWC_SPIN_LIMIT);
      if (tries >= SWC_SPIN_LIMIT) atomicOr(&dyn->status, SWC_STATUS_SPIN);
      if (mine) {
        if (s == rk) {
          // RSS(theta + delta e_a) - RSS(theta) = delta'(H_aa delta - 2 r_a), r_a taken before the step
          double rb0 = lds_ld(rbef + er), rb1 = lds_ld(rbef + rk * P + p1);
          int spins = 0;
#pragma nounroll
          while (is_sent(rb0) || is_sent(rb1)) {
            if (++spins > SWC_SPIN_LIMIT) { atomicOr(&dyn->status, SWC_STATUS_SPIN); break; }
            rb0 = lds_ld(rbef + er); rb1 = lds_ld(rbef + rk * P + p1);
          }
          rss_acc += dv[BW] * (va - 2.0 * rb0);
          if (two) rss_acc += dv[BW + 1] * (vb - 2.0 * rb1);
        } else {
          r_0 -= va; r_1 -= vb;
          if (s == rk - 3) { pick[er] = r_0; if (two) pick[er + 1] = r_1; }
        }
      }
    };
#ifdef SWC_NO_HELPERS
    rk_hi = -1;
#endif
    if (rk_hi >= 0) {
      H2r hA = {}, hB = {};
      int s = (rk_hi >= 3) ? 0 : rk_lo;
      int s1 = next_w(s);
      int off1 = hs_b[min(s1, n_steps - 1)];           // offsets are read one step before the loads that use them
      loadH(hA, hs_b[s]);
      while (true) {
        int s2 = next_w(s1);
        int off2 = hs_b[min(s2, n_steps - 1)];
        loadH(hB, off1);
        process(s, hA);
        if (s1 > rk_hi) break;
        s = s2; s2 = next_w(s2);
        off1 = hs_b[min(s2, n_steps - 1)];
        loadH(hA, off2);
        process(s1, hB);
        if (s > rk_hi) break;
        s1 = s2;
      }
    }
  }
  __syncthreads();
  TSTAMP0(c, 30);
  // ---------------- sigma^2 (updateSigma, UpdateSigma.h:22-58) ---------------------------------
  if (mask & U_SIGMA) {
    // RSS = YY + sum of the threads' shares (RSS(theta_0) - YY and the steps' increments), fixed-order reduction
    // (covariate-adjusted: YY is replaced by sum_i yy_i - 2 o_i's_i + o_i'G_i o_i, block partials of k_curve_z)
    double acc = isB ? -rss_acc : 0.0;
    if (d.D > 0)
      for (int x = tid; x < c.nblk_curve; x += nthr) acc -= c.yyp_part[x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      double qs = 0.0;
      for (int w = 0; w < nthr / 64; ++w) qs += red[w];
      const double rss = (d.D > 0) ? -qs : (c.YY - qs);
      const bool tempered = (dyn->tt_step != 0);
      const double bb = (tempered ? (beta / 2) * rss : 0.5 * rss) + c.h.beta_0;
      const double s2 = 1.0 / (sig_g * (1.0 / bb));
      dyn->sigma2 = s2;
      dyn->rss = rss;
      c.c_sigma[slot] = s2;
    }
  } else if (tid == 0) {
    c.c_sigma[slot] = dyn->sigma2;
  }
  // ---------------- publish theta and its chain slots -------------------------------------------
  double* s_nu = c.c_nu + (size_t)slot * K * P;
  double* s_phi = c.c_Phi + (size_t)slot * K * P * M;
  if (isB) {
    const int jj = b / MD, mt = b - jj * MD;
    for (int u = 0; u < (two ? 2 : 1); ++u) {
      const int pu = p0 + u;
      const double th_e = th[b * P + pu];
      c.theta[(size_t)fd * P + pu] = th_e;
      if (mt == 0) s_nu[jj + (size_t)K * pu] = th_e;
      else s_phi[jj + (size_t)K * (pu + (size_t)P * (mt - 1))] = th_e;
    }
  }
  if (MD == 1)
    for (int x = tid; x < K * P * M; x += nthr) {
      const int k = x % K, pm = x / K, pp = pm % P, m = pm / P;
      s_phi[x] = c.theta[(size_t)(k * (M + 1) + m + 1) * P + pp];
    }
}

// ---------------------------------------------------------------------------------------------
// k_loglik: calcLikelihood = sum_il dnorm(y_il; mean_il, sqrt(sigma2), log)  and end-of-iteration
// bookkeeping (advance the iteration counter / slot for graph replay).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_loglik(Ctx c0, int use_rss_part, int r_stored) {
  const Ctx c = chain_view(c0);      // chain blockIdx.z of the batch
  TIMELINE(c, 6);
  __shared__ double red[256];
  Dyn* dyn = c.dyn;
  const int tid = threadIdx.x;
  double rss = dyn->rss;
  if (use_rss_part) {
    double acc = 0.0;
    const int per = (c.nblk_curve + 255) / 256;
    for (int b = tid * per; b < min(c.nblk_curve, (tid + 1) * per); ++b) acc += c.rss_part[b];
    rss = block_sum256(acc, red);
  }
  if (tid == 0) {
    const double s2 = dyn->sigma2;
    double ll;
    if (c.d.mv)   // calcLikelihoodMV: (y_obs.n_cols / 2) is an integer division, CalculateLikelihood.h:155
      ll = -(double)c.d.n * ((c.d.P / 2) * log(2 * 3.14159265358979323846 * s2)) - (1 / (s2 * 2)) * rss;
    else
      ll = -(double)c.d.n_obs_total * (0.91893853320467274178 + log(sqrt(s2))) - rss / (2.0 * s2);
    dyn->rss = rss;
    dyn->loglik = ll;
    if (c.mask & U_LOGLIK) c.c_loglik[dyn->slot] = ll;
    dyn->iter += 1;
    dyn->slot = (r_stored > 0) ? ((dyn->iter - dyn->slot_base) % (uint32_t)r_stored) : dyn->iter - dyn->slot_base;
  }
}

// reduces a still-pending log-likelihood (launched once at the end of a run)
// status_out (host-mapped pinned memory, one word per chain; may be null): the chain's status word for bfmmm_run -- written
// from the run's last kernel, it saves the device-to-host copy a run used to queue behind its kernels (about 10 us of a call)
__global__ __launch_bounds__(256) void k_loglik_flush(Ctx c0, uint32_t* status_out) {
  const Ctx c = chain_view(c0);      // chain blockIdx.z of the batch
  __shared__ double red[256];
  if (blockIdx.x == 1) {             // second workgroup: the last iteration's scalar job (Ctx::defer_hyper), beside the log-likelihood
    if (c.dyn->hyper_pending) {      // (dynamic LDS: HYPER_LDS_DOUBLES)
      job_hyper(c, false);
      __syncthreads();
      if (threadIdx.x == 0) c.dyn->hyper_pending = 0u;
    }
    return;
  }
  if (c.dyn->ll_pending) deferred_loglik(c, red);
  if (status_out && threadIdx.x == 0) {
    __hip_atomic_store(&status_out[blockIdx.z], c.dyn->status, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// broadcast the current value of blocks a sweep does not update into chain slots [s0, s1)
__global__ void k_fill_slots(double* chain, const double* cur, size_t len, int s0, int s1, size_t chain_bytes) {
  chain = ptr_shift(chain, blockIdx.z * chain_bytes);      // chain blockIdx.z of the batch
  cur = ptr_shift(cur, blockIdx.z * chain_bytes);
  const size_t total = len * (size_t)(s1 - s0);
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
    chain[(size_t)s0 * len + e] = cur[e % len];
}

// ---- host launchers -------------------------------------------------------------------------
// The one decision of which sweep kernel a run launches (bfmmm_debug_get("sweep_route") reports it).
SweepRoute sweep_route_decide(const Dims& d) {
  SweepRoute r;
  if (d.BW == 0 && d.BWP == 0 && d.A <= 8 * DG_RPL_MAX && d.P <= 64) {        // diagonal model: independent scalar chains per coordinate
    r.kernel = 0;
    r.targ = std::min((d.A + 7) / 8, DG_RPL_MAX);
    r.threads = (8 * d.P + 63) / 64 * 64;
    r.lds = (16 + (size_t)d.A * d.A) * sizeof(double) + ((size_t)d.A * d.A + (size_t)d.K * (d.M + 1) + 8) * sizeof(int) + 16;
    return r;
  }
  const int swc_ph = (d.P + 1) / 2, swc_lrk = swc_ph <= 4 ? 4 : swc_ph <= 8 ? 8 : 16;      // lanes per rank of the row threads
  const size_t swc_lds = (5 * (((size_t)d.A * d.P + 1) & ~(size_t)1) + 32 + (size_t)d.A * (32 + 2 * d.BW + 2) + 16) * sizeof(double) + 2 * ((size_t)d.A + 2) * sizeof(int4) +
                         ((size_t)d.A * d.A + (size_t)d.A + 8) * sizeof(int) + 16;
  if (d.P <= 32 && d.A * swc_lrk <= SWC_THREADS - 64 && d.BW <= 5 && swc_lds <= 160 * 1024) {      // fast path: the chain in one wave
    r.kernel = 1;
    r.targ = d.BW;
    r.threads = 64 + (d.A * swc_lrk + 63) / 64 * 64;
    r.lds = swc_lds;       // beyond 64 KB at small P and many directions (P = 8, A >= 71): opted in by prepare_sweep_kernels
    return r;
  }
  const bool diag = (d.BW == 0 && d.BWP == 0);
  size_t pf_len = (size_t)d.A * d.LG + (diag ? (size_t)d.P : (size_t)d.P * d.P);
  auto lds_for = [&](size_t pf) {
    const size_t doubles = (size_t)d.A * (d.P + 2 * d.BW) + 4 * (size_t)d.A * d.P + PMAX + PMAX + 2 * BWWIDE + 32 + 2 * pf;
    return doubles * sizeof(double) + (size_t)d.A * d.A * sizeof(int) + 16;
  };
  if (pf_len > (size_t)NPF * SW_THREADS || lds_for(pf_len) > 160 * 1024) { r.direct = 1; pf_len = 0; }
  r.lds = lds_for(pf_len);
  r.threads = SW_THREADS;
  if (r.lds <= 160 * 1024) r.kernel = 2;
  return r;
}

int launch_sweep(const Ctx& c, hipStream_t st) {
  const Dims& d = c.d;
  const SweepRoute r = sweep_route_decide(d);
  const dim3 grid(1, 1, c.nch), block(r.threads);
  const size_t lds = r.lds;
  if (r.kernel == 0) {
    switch (r.targ) {
      case 1: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<1, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<1, false>), grid, block, lds, st, c); break;
      case 2: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<2, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<2, false>), grid, block, lds, st, c); break;
      case 3: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<3, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<3, false>), grid, block, lds, st, c); break;
      case 4: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<4, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<4, false>), grid, block, lds, st, c); break;
      case 5: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<5, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<5, false>), grid, block, lds, st, c); break;
      case 6: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<6, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<6, false>), grid, block, lds, st, c); break;
      case 7: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<7, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<7, false>), grid, block, lds, st, c); break;
      default: if (d.mv) hipLaunchKernelGGL((k_sweep_diag<8, true>), grid, block, lds, st, c); else hipLaunchKernelGGL((k_sweep_diag<8, false>), grid, block, lds, st, c); break;
    }
    return 0;
  }
  if (r.kernel == 1) {
    switch (r.targ) {
      case 0: hipLaunchKernelGGL(k_sweep_chain<0>, grid, block, lds, st, c); break;
      case 1: hipLaunchKernelGGL(k_sweep_chain<1>, grid, block, lds, st, c); break;
      case 2: hipLaunchKernelGGL(k_sweep_chain<2>, grid, block, lds, st, c); break;
      case 3: hipLaunchKernelGGL(k_sweep_chain<3>, grid, block, lds, st, c); break;
      case 4: hipLaunchKernelGGL(k_sweep_chain<4>, grid, block, lds, st, c); break;
      default: hipLaunchKernelGGL(k_sweep_chain<5>, grid, block, lds, st, c); break;
    }
    return 0;
  }
  if (r.kernel != 2) return 1;
  hipLaunchKernelGGL(k_sweep, grid, block, lds, st, c, r.direct);
  return 0;
}

void launch_loglik_flush(const Ctx& c, hipStream_t st, uint32_t* status_out) {
  hipLaunchKernelGGL(k_loglik_flush, dim3(c.defer_hyper ? 2 : 1, 1, c.nch), dim3(256), (size_t)HYPER_LDS_DOUBLES * sizeof(double), st, c, status_out);
}

void launch_loglik(const Ctx& c, int use_rss_part, int r_stored, hipStream_t st) {
  hipLaunchKernelGGL(k_loglik, dim3(1, 1, c.nch), dim3(256), 0, st, c, use_rss_part, r_stored);
}

void prepare_sweep_kernels() {
  set_max_lds((const void*)k_sweep);
  set_max_lds((const void*)k_sweep_chain<0>); set_max_lds((const void*)k_sweep_chain<1>); set_max_lds((const void*)k_sweep_chain<2>);
  set_max_lds((const void*)k_sweep_chain<3>); set_max_lds((const void*)k_sweep_chain<4>); set_max_lds((const void*)k_sweep_chain<5>);
}

void launch_fill_slots(const Ctx& c, double* chain, const double* cur, size_t len, int s0, int s1, hipStream_t st) {
  if (s1 <= s0 || len == 0) return;
  hipLaunchKernelGGL(k_fill_slots, dim3(256, 1, c.nch), dim3(256), 0, st, chain, cur, len, s0, s1, c.chain_bytes);
}

}  // namespace bfmmm
