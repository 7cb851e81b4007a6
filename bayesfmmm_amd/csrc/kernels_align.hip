// Label alignment of chain slots against a pivot membership matrix (the pivot method of Marin, Mengersen &
// Robert 2005).  Labels only: signs and rotations of the eigenfunctions are not touched.
//
//   k_align_gram     One workgroup of 256 threads per draw (q, t).  A[c][l] = sum_i Z_ic(q, t) Zref_il: a thread walks
//                    i = tid, tid + 256, .. down the columns (Z slots are i-fastest: the reads coalesce; Zref comes from L2)
//                    with its KP x KP partial sums in registers, KP = 4 (K <= 4) or 8; components at or past K are never
//                    loaded and never assignable.  Then perm(q, t), the exact maximiser over all K! permutations of
//                    sum_l A[perm(l)][l], by a subset recursion over the 2^K masks in LDS:
//                        g[l][mask] = max over c in mask of A[c][l] + g[l + 1][mask \ c]     (|mask| = K - l, l = K - 1 .. 0)
//                    one thread per mask and level; thread 0 reads the permutation off from l = 0, taking the smallest c that
//                    attains g[l][mask] exactly: the lexicographically smallest maximiser of the right-nested sum
//                    A[p0][0] + (A[p1][1] + (..)), which is score(q, t).
//   k_align_gather   k_diag_gather with the component index of the source element relabelled per draw: element
//                    e = a + inner (k + K b) of the row is read from a + inner (perm[k] + K b) of the same slot.
//   k_align_project  v[(k + K g)][q S + s] = sum_p E_gp nu_{perm[k], p}(q, s), draw fastest, p = 0 .. P - 1 in order.
// Summation order of A, fixed by (thread, wave, workgroup) alone whatever the grid or the call: a thread's terms in the order
// of i; the 64 lanes of a wave by a butterfly (offsets 32 .. 1); the four waves' sums in wave order from LDS.  No atomics.
#include "model.hpp"
#include "launchers.hpp"

#include <string>

// the products and sums must round as the restatement's bound assumes: one rounding each
#pragma clang fp contract(off)

namespace bfmmm {

namespace {

constexpr int AL_NT = 256;
constexpr int AL_WAVES = AL_NT / 64;

template <int KP>
__global__ __launch_bounds__(AL_NT) void k_align_gram(const double* c_Z, size_t chain_bytes, const double* Zref, int n, int K,
                                                      int first_slot, int S, int32_t* perm, double* score) {
  __shared__ double sW[AL_WAVES][KP * KP];      // the waves' sums
  __shared__ double sA[KP * KP];                // A[c][l] at c KP + l
  __shared__ double sG[KP + 1][1 << KP];        // g[l][mask]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = (int)(blockIdx.x / (unsigned)S), s = (int)(blockIdx.x - (unsigned)q * (unsigned)S);
  const double* Z = ptr_shift(c_Z, (size_t)q * chain_bytes) + (size_t)(first_slot + s) * ((size_t)n * K);
  double acc[KP][KP];
#pragma unroll
  for (int c = 0; c < KP; ++c)
#pragma unroll
    for (int l = 0; l < KP; ++l) acc[c][l] = 0.0;
  for (int i = tid; i < n; i += AL_NT) {
    double z[KP], r[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
      z[c] = c < K ? Z[(size_t)c * n + i] : 0.0;
      r[c] = c < K ? Zref[(size_t)c * n + i] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < KP; ++c)
#pragma unroll
      for (int l = 0; l < KP; ++l) acc[c][l] += z[c] * r[l];
  }
#pragma unroll
  for (int c = 0; c < KP; ++c)
#pragma unroll
    for (int l = 0; l < KP; ++l) {
      double v = acc[c][l];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) sW[wave][c * KP + l] = v;
    }
  __syncthreads();
  if (tid < KP * KP) {
    double v = sW[0][tid];
    for (int w = 1; w < AL_WAVES; ++w) v += sW[w][tid];
    sA[tid] = v;
  }
  if (tid == 0) sG[K][0] = 0.0;
  __syncthreads();
  // the subset recursion over the K real components: level l assigns column l to a component of the mask
  const unsigned full = (1u << K) - 1u;
  for (int l = K - 1; l >= 0; --l) {
    const unsigned mask = (unsigned)tid;
    if (mask <= full && __popc(mask) == K - l) {
      double best = 0.0;
      bool any = false;
      for (int c = 0; c < K; ++c)
        if (mask >> c & 1u) {
          const double v = sA[c * KP + l] + sG[l + 1][mask ^ (1u << c)];
          if (!any || v > best) { best = v; any = true; }
        }
      sG[l][mask] = best;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int32_t* out = perm + (size_t)blockIdx.x * K;
    unsigned mask = full;
    for (int l = 0; l < K; ++l) {
      const double want = sG[l][mask];
      int pick = -1, low = -1;
      for (int c = K - 1; c >= 0; --c)
        if (mask >> c & 1u) {
          low = c;
          if (sA[c * KP + l] + sG[l + 1][mask ^ (1u << c)] == want) pick = c;
        }
      if (pick < 0) pick = low;      // a non-finite sum attains nothing: the permutation stays one
      out[l] = pick;
      mask ^= 1u << pick;
    }
    if (score) score[blockIdx.x] = sG[0][full];
  }
}

// ws[s + S (c + C p)] = chain c's slot (first + s), element p0 + p with its component index relabelled by the draw's row of
// perm[(c S + s) K + .]; inner = 0: the array has no component axis and is gathered as it is.  Tiles as in k_diag_gather.
__global__ __launch_bounds__(256) void k_align_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first,
                                                      int S, int C, int p0, int P, const int32_t* perm, int K, long long inner, double* ws) {
  __shared__ double tile[32][33];
  const int tiles_s = (S + 31) / 32;
  const int ts = (int)(blockIdx.x % (unsigned)tiles_s), tp = (int)(blockIdx.x / (unsigned)tiles_s), c = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double* src = (const double*)((const char*)base + (size_t)c * chain_bytes);
  for (int r = ty; r < 32; r += 8) {
    const int s = ts * 32 + r, p = tp * 32 + tx;
    if (s < S && p < P) {
      long long e = (long long)p0 + p;
      if (inner > 0) {
        const long long a = e % inner, kb = e / inner, k = kb % K, b = kb / K;
        e = a + inner * ((long long)perm[((size_t)c * S + s) * K + k] + (long long)K * b);
      }
      tile[r][tx] = src[(long long)(first + s) * ss + e * ps];
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int p = tp * 32 + r, s = ts * 32 + tx;
    if (s < S && p < P) ws[(size_t)s + (size_t)S * ((size_t)c + (size_t)C * (size_t)p)] = tile[tx][r];
  }
}

// rows [r0, r0 + gridDim.y) of the table, row = k + K g: V[cs + CS (row - r0)], cs = q S + s
__global__ __launch_bounds__(256) void k_align_project(const double* c_nu, size_t chain_bytes, const double* E, const int32_t* perm, int K,
                                                       int P, int first_slot, int S, long long CS, int r0, double* V) {
  const long long cs = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cs >= CS) return;
  const int row = r0 + (int)blockIdx.y, g = row / K, k = row - g * K;
  const int q = (int)(cs / S), s = (int)(cs - (long long)q * S);
  const double* nu = ptr_shift(c_nu, (size_t)q * chain_bytes) + (size_t)(first_slot + s) * ((size_t)K * P) + perm[(size_t)cs * K + k];
  const double* e = E + (size_t)g * P;
  double v = 0.0;
  for (int p = 0; p < P; ++p) v += e[p] * nu[(size_t)K * p];
  V[(size_t)cs + (size_t)CS * blockIdx.y] = v;
}

std::string align_range(const char* kernel, const Ctx& c, int first_slot, int n_slots) {
  const std::string k = std::string(kernel) + ": ";
  if (c.d.K < 1 || c.d.K > KMAX) return k + "K outside 1 .. 8";
  if (n_slots < 1 || first_slot < 0 || first_slot + n_slots > c.T) return k + "range outside the chain storage";
  if ((long long)c.nch * n_slots > (1LL << 22)) return k + "more than 2^22 draws";
  return "";
}

}  // namespace

std::string launch_align_gram(const Ctx& c, const double* Zref, int first_slot, int n_slots, int32_t* perm, double* score, hipStream_t st) {
  const std::string bad = align_range("k_align_gram", c, first_slot, n_slots);
  if (!bad.empty()) return bad;
  if (!Zref || !perm) return "k_align_gram: 'Zref' or 'perm' is null";
  const Dims& d = c.d;
  const unsigned grid = (unsigned)((long long)c.nch * n_slots);
  if (d.K <= 4) hipLaunchKernelGGL((k_align_gram<4>), dim3(grid), dim3(AL_NT), 0, st, c.c_Z, c.chain_bytes, Zref, d.n, d.K, first_slot, n_slots, perm, score);
  else hipLaunchKernelGGL((k_align_gram<8>), dim3(grid), dim3(AL_NT), 0, st, c.c_Z, c.chain_bytes, Zref, d.n, d.K, first_slot, n_slots, perm, score);
  if (hipGetLastError() != hipSuccess) return "k_align_gram: launch failed";
  return "";
}

std::string launch_align_gather(const double* base, size_t chain_bytes, long long ss, long long ps, int first, int S, int C, int p0, int P,
                                const int32_t* perm, int K, long long inner, double* ws, hipStream_t st) {
  const long long tiles = (long long)((S + 31) / 32) * ((P + 31) / 32);
  if (tiles > 0x7fffffffLL || C > 65535) return "k_align_gather: grid too large";
  if (!base || !perm || !ws || K < 1 || K > KMAX || inner < 0) return "k_align_gather: bad arguments";
  hipLaunchKernelGGL(k_align_gather, dim3((unsigned)tiles, 1, (unsigned)C), dim3(256), 0, st, base, chain_bytes, ss, ps, first, S, C, p0, P, perm, K,
                     inner, ws);
  if (hipGetLastError() != hipSuccess) return "k_align_gather: launch failed";
  return "";
}

std::string launch_align_project(const Ctx& c, const double* E, int G, const int32_t* perm, int first_slot, int n_slots, int r0, int rows,
                                 double* V, hipStream_t st) {
  const std::string bad = align_range("k_align_project", c, first_slot, n_slots);
  if (!bad.empty()) return bad;
  const Dims& d = c.d;
  if (!E || !perm || !V || G < 1 || r0 < 0 || rows < 1 || rows > 65535 || (long long)r0 + rows > (long long)d.K * G) return "k_align_project: bad arguments";
  const long long CS = (long long)c.nch * n_slots;
  hipLaunchKernelGGL(k_align_project, dim3((unsigned)((CS + 255) / 256), (unsigned)rows), dim3(256), 0, st, c.c_nu, c.chain_bytes, E, perm, d.K, d.P,
                     first_slot, n_slots, CS, r0, V);
  if (hipGetLastError() != hipSuccess) return "k_align_project: launch failed";
  return "";
}

}  // namespace bfmmm
