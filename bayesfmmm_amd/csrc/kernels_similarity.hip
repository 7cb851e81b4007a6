// Pooled co-membership of curves from chain slots: for every chain q, slot t and pair of curves (i, j)
//     d_ij(q, t) = sum_k Z_ik(q, t) Z_jk(q, t)        (Z rows on the simplex: 0 <= d <= 1, d_ii = sum_k Z_ik^2),
// a sum over k (label-invariant), so the chains pool as they are.  Of the N = C S draws of slots [first_slot, first_slot + S):
//     mean[r n + j]             the mean of d over the N draws (result row r is curve curves[r], or r; column j every curve),
//     sd[r n + j]               the sample sd (N - 1; NaN for one draw), in a second pass over the draws,
//     chain_mean[(r C + q) n + j]  the mean over the S slots of chain q.
//
//   k_similarity   A workgroup of four waves owns a block of 16 x 16 tiles of the result: 64 x 64 (each wave one row tile
//                  and four column tiles) or, where that gives too few workgroups, 16 x 64 (each wave one tile).  Z_.k of
//                  the block's rows and columns of a run of draws is staged in LDS once (next run's loads in flight while
//                  this one is consumed; zeros for k >= K and for curves past the edge), so Z comes from L2 once per block
//                  and each staged value feeds up to four v_mfma_f64_16x16x4_f64.  A draw's d of a tile is that one
//                  instruction on a zero accumulator (k < 4; a second one chained for k = 4 .. 7): lane l feeds
//                  A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15] and receives D[row (l >> 4) + 4 reg][col l & 15].
// Summation order, fixed per entry whatever the block, the grid, the chunk or the call:  s_q = sum_t d(q, t) in slot order
// from 0, the pooled sum sum_q s_q in chain order from 0, mean = that / N, chain_mean = s_q / S; the sd pass forms d by the
// same instructions and sums (d - mean)^2 in the same order, sd = sqrt(that / (N - 1)).  No atomics, no split over the
// draws, no scratch.  d_ij and d_ji are the same products summed in the same order: the full matrix is symmetric bit for bit.
#include "model.hpp"
#include "launchers.hpp"

#include <string>

// the MFMA fuses internally; the accumulation over the draws must round as the restatement's does
#pragma clang fp contract(off)

namespace bfmmm {

int g_similarity_block = 0;      // bfmmm_set_similarity_block

namespace {

constexpr int SIM_NT = 256;
constexpr int SIM_ROWS = 16;      // staged k-rows of a buffer: (draws of a run) x (k padded to 4 or 8)
constexpr int SIM_BIG_MIN = 512;  // 64 x 64 blocks only where they make at least this many workgroups (two per CU)

struct SimArgs {
  const double* c_Z;              // chain 0's slots; chain q's are q * chain_bytes further
  size_t chain_bytes;
  const int* curves;              // the curve of row r of the chunk, or null: curve r0 + r
  int r0, rows, n, K, C, first_slot, S;
  double *mean, *sd, *chain_mean; // of the chunk: [r n + j], [r n + j], [(r C + q) n + j]; sd, chain_mean may be null
};

// KB: MFMAs per draw (k in blocks of 4); WR x WC waves, CT column tiles each
template <int KB, int WR, int CT>
struct SimGeom {
  static constexpr int WC = 4 / WR, BR = 16 * WR, BC = 16 * CT * WC, NCV = BR + BC;   // block rows, columns; staged curves
  static constexpr int KP = 4 * KB, DR = SIM_ROWS / KP;                               // padded k, draws per run
  // doubles between staged k-rows: = 16 mod 32, so that the four k-rows a wave reads at once fall on distinct LDS banks
  static constexpr int SLD = NCV + (48 - NCV % 32) % 32;
  static constexpr int NE = SIM_ROWS * NCV / SIM_NT;                                  // staged values per thread and run
  static_assert(SIM_ROWS * NCV % SIM_NT == 0, "a run's values divide among the threads");
};

// One pass over the draws for the CT tiles of a wave: tot[ct] = sum_q sum_t f(d), f(d) = d (PASS 0) or (d - mu)^2 (PASS 1).
template <int KB, int WR, int CT, int PASS>
__device__ __forceinline__ void sim_pass(const SimArgs& a, double* sZ, const int (&goff)[SimGeom<KB, WR, CT>::NE], int tid, int aoff,
                                         int boff, int row0, int col0, double4_t (&tot)[CT], const double4_t (&mu)[CT]) {
  using G = SimGeom<KB, WR, CT>;
  constexpr int KP = G::KP, DR = G::DR, SLD = G::SLD, NCV = G::NCV, NE = G::NE;
  const int RPC = (a.S + DR - 1) / DR, NR = a.C * RPC;      // runs per chain, runs
  const size_t slot = (size_t)a.n * a.K;
  const double4_t zero = {0.0, 0.0, 0.0, 0.0};
  double v[NE];
  auto fetch = [&](int g) {
    const int q = g / RPC, s0 = (g - q * RPC) * DR, len = min(DR, a.S - s0);
    const double* base = ptr_shift(a.c_Z, (size_t)q * a.chain_bytes) + (size_t)(a.first_slot + s0) * slot;
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int dd = (tid + SIM_NT * u) / (NCV * KP);
      v[u] = (goff[u] >= 0 && dd < len) ? base[(size_t)dd * slot + goff[u]] : 0.0;
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + SIM_NT * u, row = e / NCV, cl = e - row * NCV;      // row = draw of the run * KP + k
      sZ[(buf * SIM_ROWS + row) * SLD + cl] = v[u];
    }
  };
  double4_t s[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) { s[ct] = zero; tot[ct] = zero; }
  fetch(0);
  put(0);
  __syncthreads();
  for (int g = 0; g < NR; ++g) {
    if (g + 1 < NR) fetch(g + 1);
    const int q = g / RPC, s0 = (g - q * RPC) * DR, len = min(DR, a.S - s0);
    const double* zb = sZ + (g & 1) * SIM_ROWS * SLD;
    for (int dd = 0; dd < len; ++dd) {
      const double* zd = zb + dd * KP * SLD;
      double av[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) av[kb] = zd[kb * 4 * SLD + aoff];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        double4_t d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], zd[boff + ct * 16], zero, 0, 0, 0);
        if (KB > 1) d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[KB - 1], zd[4 * SLD + boff + ct * 16], d, 0, 0, 0);
        if (PASS == 0) s[ct] += d;
        else { const double4_t e = d - mu[ct]; s[ct] += e * e; }
      }
    }
    if (s0 + len == a.S) {      // the chain's last run: s_q is complete
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        tot[ct] += s[ct];
        if (PASS == 0 && a.chain_mean) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = row0 + 4 * r, col = col0 + ct * 16;
            if (row < a.rows && col < a.n) a.chain_mean[((size_t)row * a.C + q) * a.n + col] = s[ct][r] / (double)a.S;
          }
        }
        s[ct] = zero;
      }
    }
    if (g + 1 < NR) put((g + 1) & 1);      // the buffer run g - 1 was read from, before the barrier that ended run g - 1's turn
    __syncthreads();
  }
}

template <int KB, int WR, int CT>
__global__ __launch_bounds__(SIM_NT) void k_similarity(SimArgs a, int ncb) {
  using G = SimGeom<KB, WR, CT>;
  constexpr int BR = G::BR, BC = G::BC, NCV = G::NCV, KP = G::KP, SLD = G::SLD, NE = G::NE;
  __shared__ double sZ[2 * SIM_ROWS * SLD];
  __shared__ int sIdx[BR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / G::WC, wc = wave % G::WC;
  const int rb = (int)(blockIdx.x / (unsigned)ncb), cb = (int)(blockIdx.x - (unsigned)rb * ncb);
  if (tid < BR) {
    const int row = rb * BR + tid;
    sIdx[tid] = row < a.rows ? (a.curves ? a.curves[row] : a.r0 + row) : -1;
  }
  __syncthreads();
  // what this thread stages of every run: Z_.k of one curve of the block's rows or columns (-1: a zero)
  int goff[NE];
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = tid + SIM_NT * u, cl = e % NCV, kk = (e / NCV) % KP;
    const int j = cb * BC + cl - BR;
    const int curve = cl < BR ? sIdx[cl] : (j < a.n ? j : -1);
    goff[u] = (curve >= 0 && kk < a.K) ? kk * a.n + curve : -1;
  }
  const int aoff = (lane >> 4) * SLD + wr * 16 + (lane & 15);
  const int boff = (lane >> 4) * SLD + BR + wc * CT * 16 + (lane & 15);
  const int row0 = rb * BR + wr * 16 + (lane >> 4), col0 = cb * BC + wc * CT * 16 + (lane & 15);   // D layout: row0 + 4 reg
  const double N = (double)a.C * (double)a.S;
  double4_t tot[CT], mu[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) mu[ct] = double4_t{0.0, 0.0, 0.0, 0.0};
  sim_pass<KB, WR, CT, 0>(a, sZ, goff, tid, aoff, boff, row0, col0, tot, mu);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    mu[ct] = tot[ct] / N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * r, col = col0 + ct * 16;
      if (row < a.rows && col < a.n) a.mean[(size_t)row * a.n + col] = mu[ct][r];
    }
  }
  if (!a.sd) return;
  sim_pass<KB, WR, CT, 1>(a, sZ, goff, tid, aoff, boff, row0, col0, tot, mu);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * r, col = col0 + ct * 16;
      if (row < a.rows && col < a.n) a.sd[(size_t)row * a.n + col] = sqrt(tot[ct][r] / (N - 1.0));      // one draw: 0 / 0
    }
  }
}

template <int KB, int WR, int CT>
std::string sim_launch(const SimArgs& a, hipStream_t st) {
  using G = SimGeom<KB, WR, CT>;
  const long long nrb = (a.rows + G::BR - 1) / G::BR, ncb = (a.n + G::BC - 1) / G::BC;
  if (nrb * ncb > 0x7fffffffLL) return "k_similarity: too many workgroups in one chunk";
  hipLaunchKernelGGL((k_similarity<KB, WR, CT>), dim3((unsigned)(nrb * ncb)), dim3(SIM_NT), 0, st, a, (int)ncb);
  if (hipGetLastError() != hipSuccess) return "k_similarity: launch failed";
  return "";
}

// ---- the least-squares loss of every draw against the pooled mean -------------------------------------------
//     loss(q, t) = sum_i sum_j (d_ij(q, t) - m_ij)^2,    m = the mean k_similarity writes, bit for bit
// over the 64 x 64 blocks (rb, cb), rb <= cb, of the full matrix in the order rb first, then cb.
//   k_similarity_loss         block b0 + blockIdx.x: pass 0 is sim_pass<., 4, 4, 0>, the mean pass of k_similarity's 64 x 64 block,
//                             which leaves m in registers; pass 1 forms d again and reduces (d - m)^2 over the block to
//                             partial[blockIdx.x N + q S + t].  Entries past n were fed zeros and have m = 0: they add exactly 0.
//   k_similarity_loss_reduce  one thread per draw: loss += w partial over the chunk's blocks in order, w = 1 on the diagonal of
//                             blocks and 2 above it (d_ij and d_ji are the same bits), from the value the chunk before left.
// Summation order of a block's 4096 squares, by position in the block alone: a lane's 16 (column tile, then register) in order;
// the 256 lanes' sums of a draw parked in LDS, read back by 64 lanes as 4 sequential sums each, which a butterfly joins.
constexpr int LOSS_BATCH = 4;      // draws parked per buffer: 2 x 8 KiB beside the staging leave three workgroups a CU

template <int KB>
__device__ __forceinline__ void sim_loss_pass(const SimArgs& a, double* sZ, double* sP, const int (&goff)[SimGeom<KB, 4, 4>::NE], int tid,
                                              int aoff, int boff, const double4_t (&mu)[4], double* part) {
  using G = SimGeom<KB, 4, 4>;
  constexpr int KP = G::KP, DR = G::DR, SLD = G::SLD, NCV = G::NCV, NE = G::NE, CT = 4;
  const int RPC = (a.S + DR - 1) / DR, NR = a.C * RPC;      // runs per chain, runs
  const size_t slot = (size_t)a.n * a.K;
  const double4_t zero = {0.0, 0.0, 0.0, 0.0};
  double v[NE];
  auto fetch = [&](int g) {
    const int q = g / RPC, s0 = (g - q * RPC) * DR, len = min(DR, a.S - s0);
    const double* base = ptr_shift(a.c_Z, (size_t)q * a.chain_bytes) + (size_t)(a.first_slot + s0) * slot;
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int dd = (tid + SIM_NT * u) / (NCV * KP);
      v[u] = (goff[u] >= 0 && dd < len) ? base[(size_t)dd * slot + goff[u]] : 0.0;
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int e = tid + SIM_NT * u, row = e / NCV, cl = e - row * NCV;
      sZ[(buf * SIM_ROWS + row) * SLD + cl] = v[u];
    }
  };
  constexpr int RB = LOSS_BATCH / DR;      // runs per parked batch
  constexpr int LPD = SIM_NT / LOSS_BATCH;  // lanes that share a draw's 256 parked sums
  static_assert(LOSS_BATCH % DR == 0 && LPD <= 64 && LPD >= 32, "whole runs per batch; a draw's lanes within a wave");
  // the draws of the batch that began with run g0, parked in buffer buf.  A last batch that is not full (a short last run of a
  // chain, fewer runs than a batch holds) leaves places of the buffer stale or never written: they are read and summed like the
  // others, and the store below leaves them out (g < NR, s < S), so nothing of them reaches memory.
  auto reduce = [&](int g0, int buf) {
    const int j = tid / LPD, sub = tid % LPD;
    const double* w = sP + (buf * LOSS_BATCH + j) * SIM_NT + sub;
    double x = w[0];
#pragma unroll
    for (int i = 1; i < LOSS_BATCH; ++i) x += w[LPD * i];
#pragma unroll
    for (int m = LPD / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    const int g = g0 + j / DR, q = g / RPC, s = (g - q * RPC) * DR + j % DR;
    if (sub == 0 && g < NR && s < a.S) part[(long long)q * a.S + s] = x;
  };
  fetch(0);
  put(0);
  __syncthreads();
  for (int g = 0; g < NR; ++g) {
    if (g + 1 < NR) fetch(g + 1);
    const int len = min(DR, a.S - g % RPC * DR);
    if (g > 0 && g % RB == 0) reduce(g - RB, (g / RB - 1) & 1);
    const double* zb = sZ + (g & 1) * SIM_ROWS * SLD;
    for (int dd = 0; dd < len; ++dd) {
      const double* zd = zb + dd * KP * SLD;
      double av[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) av[kb] = zd[kb * 4 * SLD + aoff];
      double p = 0.0;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        double4_t d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], zd[boff + ct * 16], zero, 0, 0, 0);
        if (KB > 1) d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[KB - 1], zd[4 * SLD + boff + ct * 16], d, 0, 0, 0);
        const double4_t e = d - mu[ct];
#pragma unroll
        for (int r = 0; r < 4; ++r) p += e[r] * e[r];
      }
      sP[((((g / RB) & 1) * RB + g % RB) * DR + dd) * SIM_NT + tid] = p;
    }
    if (g + 1 < NR) put((g + 1) & 1);
    __syncthreads();
  }
  reduce((NR - 1) / RB * RB, ((NR - 1) / RB) & 1);
}

template <int KB>
__global__ __launch_bounds__(SIM_NT) void k_similarity_loss(SimArgs a, double* partial, int b0, int nbk) {
  using G = SimGeom<KB, 4, 4>;
  constexpr int BR = G::BR, BC = G::BC, NCV = G::NCV, KP = G::KP, SLD = G::SLD, NE = G::NE;
  __shared__ double sZ[2 * SIM_ROWS * SLD];
  __shared__ double sP[2 * LOSS_BATCH * SIM_NT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // block b0 + blockIdx.x of the upper triangle, rows first
  int rb = 0, cb = b0 + (int)blockIdx.x;
  while (rb < nbk - 1 && cb >= nbk - rb) { cb -= nbk - rb; ++rb; }
  cb += rb;
  int goff[NE];
#pragma unroll
  for (int u = 0; u < NE; ++u) {
    const int e = tid + SIM_NT * u, cl = e % NCV, kk = (e / NCV) % KP;
    const int curve = cl < BR ? rb * BR + cl : cb * BC + cl - BR;
    goff[u] = (curve < a.n && kk < a.K) ? kk * a.n + curve : -1;
  }
  const int aoff = (lane >> 4) * SLD + wave * 16 + (lane & 15);
  const int boff = (lane >> 4) * SLD + BR + (lane & 15);
  const double N = (double)a.C * (double)a.S;
  double4_t tot[4], mu[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) mu[ct] = double4_t{0.0, 0.0, 0.0, 0.0};
  sim_pass<KB, 4, 4, 0>(a, sZ, goff, tid, aoff, boff, 0, 0, tot, mu);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) mu[ct] = tot[ct] / N;
  sim_loss_pass<KB>(a, sZ, sP, goff, tid, aoff, boff, mu, partial + (size_t)blockIdx.x * ((size_t)a.C * a.S));
}

__global__ __launch_bounds__(256) void k_similarity_loss_reduce(const double* partial, long long N, int b0, int nb, int nbk, double* loss) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= N) return;
  int rb = 0, cb = b0;
  while (rb < nbk - 1 && cb >= nbk - rb) { cb -= nbk - rb; ++rb; }
  cb += rb;
  double acc = b0 ? loss[o] : 0.0;
  for (int b = 0; b < nb; ++b) {
    acc += (rb == cb ? 1.0 : 2.0) * partial[(size_t)b * N + o];
    if (++cb == nbk) { ++rb; cb = rb; }
  }
  loss[o] = acc;
}

}  // namespace

long long similarity_loss_blocks(int n) {
  const long long nbk = (n + 63) / 64;
  return nbk * (nbk + 1) / 2;
}

// what both launchers check, reported under the kernel's name
static std::string loss_check(const char* kernel, const Ctx& c, int first_slot, int n_slots, long long b0, long long nb) {
  const Dims& d = c.d;
  const std::string k = std::string(kernel) + ": ";
  if (d.K < 1 || d.K > KMAX) return k + "K outside 1 .. 8";
  if (n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return k + "range outside the chain storage";
  if ((long long)c.nch * n_slots > (1LL << 22)) return k + "more than 2^22 draws";
  if ((long long)d.n * KMAX > 0x7fffffffLL) return k + "n K above 2^31 - 1";
  if (b0 < 0 || nb < 1 || b0 + nb > similarity_loss_blocks(d.n) || b0 + nb > 0x7fffffffLL) return k + "blocks outside the upper triangle";
  return "";
}

// partial[b N + q S + t] of blocks [b0, b0 + nb) of the upper triangle of 64 x 64 blocks (rows first), N = C n_slots
std::string launch_similarity_loss(const Ctx& c, int first_slot, int n_slots, long long b0, long long nb, double* partial, hipStream_t st) {
  const std::string bad = loss_check("k_similarity_loss", c, first_slot, n_slots, b0, nb);
  if (!bad.empty()) return bad;
  if (!partial) return "k_similarity_loss: 'partial' is null";
  const Dims& d = c.d;
  SimArgs a;
  a.c_Z = c.c_Z; a.chain_bytes = c.chain_bytes; a.curves = nullptr;
  a.r0 = 0; a.rows = d.n; a.n = d.n; a.K = d.K; a.C = c.nch; a.first_slot = first_slot; a.S = n_slots;
  a.mean = nullptr; a.sd = nullptr; a.chain_mean = nullptr;
  const int nbk = (d.n + 63) / 64;
  if (d.K <= 4) hipLaunchKernelGGL((k_similarity_loss<1>), dim3((unsigned)nb), dim3(SIM_NT), 0, st, a, partial, (int)b0, nbk);
  else hipLaunchKernelGGL((k_similarity_loss<2>), dim3((unsigned)nb), dim3(SIM_NT), 0, st, a, partial, (int)b0, nbk);
  if (hipGetLastError() != hipSuccess) return "k_similarity_loss: launch failed";
  return "";
}

// loss[q S + t] (+)= sum over those blocks of w partial, from 0 where b0 = 0 and from what the chunk before left otherwise
std::string launch_similarity_loss_reduce(const Ctx& c, int first_slot, int n_slots, long long b0, long long nb, const double* partial,
                                          double* loss, hipStream_t st) {
  const std::string bad = loss_check("k_similarity_loss_reduce", c, first_slot, n_slots, b0, nb);
  if (!bad.empty()) return bad;
  if (!partial || !loss) return "k_similarity_loss_reduce: 'partial' or 'loss' is null";
  const long long N = (long long)c.nch * n_slots;
  hipLaunchKernelGGL(k_similarity_loss_reduce, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, partial, N, (int)b0, (int)nb,
                     (c.d.n + 63) / 64, loss);
  if (hipGetLastError() != hipSuccess) return "k_similarity_loss_reduce: launch failed";
  return "";
}

// mean, sd (or null) and chain_mean (or null) of result rows [r0, r0 + rows) against all n curves into the chunk's buffers
// (row r0 first); curves: the chunk's curve list on the device (row r0 first), or null: result row r is curve r
std::string launch_similarity(const Ctx& c, int first_slot, int n_slots, const int* curves, int r0, int rows, double* mean, double* sd,
                              double* chain_mean, hipStream_t st) {
  const Dims& d = c.d;
  if (d.K < 1 || d.K > KMAX) return "k_similarity: K outside 1 .. 8";
  if (n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return "k_similarity: range outside the chain storage";
  if ((long long)c.nch * n_slots > (1LL << 22)) return "k_similarity: more than 2^22 draws";
  if (rows < 1 || r0 < 0 || !mean || (!curves && r0 + rows > d.n)) return "k_similarity: bad arguments";
  if ((long long)d.n * KMAX > 0x7fffffffLL) return "k_similarity: n K above 2^31 - 1";
  SimArgs a;
  a.c_Z = c.c_Z; a.chain_bytes = c.chain_bytes; a.curves = curves;
  a.r0 = r0; a.rows = rows; a.n = d.n; a.K = d.K; a.C = c.nch; a.first_slot = first_slot; a.S = n_slots;
  a.mean = mean; a.sd = sd; a.chain_mean = chain_mean;
  const long long big_blocks = (long long)((rows + 63) / 64) * ((d.n + 63) / 64);
  const bool big = g_similarity_block ? g_similarity_block == 1 : big_blocks >= SIM_BIG_MIN;
  if (d.K <= 4) return big ? sim_launch<1, 4, 4>(a, st) : sim_launch<1, 1, 1>(a, st);
  return big ? sim_launch<2, 4, 4>(a, st) : sim_launch<2, 1, 1>(a, st);
}

}  // namespace bfmmm
