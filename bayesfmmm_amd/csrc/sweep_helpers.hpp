// Small device helpers shared by the three kernel files of the Phi / nu block: kernels_pair_gram.hip (the pair-Gram
// contraction and its reductions), kernels_factor.hip (k_factor) and kernels_sweep.hip (the sweep kernels): the LDS-only
// barrier, the layout of the H2 band blocks, and the index maps between directions, pair rows and sweep steps.
#pragma once
#include "model.hpp"

namespace bfmmm {

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory
// counter (vmcnt(0)), which would serialise the global prefetches the sweep keeps in flight
// across its barriers.
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// H2: the band blocks as k_factor and the sweep read them.  Block r holds, for every row p, the 2 BW + 2 entries
// e(p, k) = G(p, p + k - BW) (k = 2 BW + 1: a zero pad) PIECE-major: the 16-byte piece (e(p, 2 q), e(p, 2 q + 1)) of row p sits at
// v2d index q P + p of the block, so that threads owning consecutive rows read consecutive 16-byte pieces (a row-major block
// made every lane of a wave-wide load touch a cache line of its own: the loads of the sweep's row threads were bound by the
// number of lines per instruction, not by bytes).
__host__ __device__ inline int h2_index(int P, int p, int k) { return (((k >> 1) * P + p) << 1) + (k & 1); }

__device__ inline int hrow(const Dims& d, int a, int b) {   // a, b: active direction indices
  const int ja = a / d.MD, ma = a - ja * d.MD, jb = b / d.MD, mb = b - jb * d.MD;
  const int zz = tri_index(d.K, min(ja, jb), max(ja, jb));
  const int cc = tri_index(d.MD, min(ma, mb), max(ma, mb));
  return zz * d.NCC + cc;
}

__device__ inline int full_dir(const Dims& d, int a) {   // active direction -> row of c.theta
  const int j = a / d.MD, mt = a - j * d.MD;
  return j * (d.M + 1) + mt;
}

// (H_block * v)[p] for a band-packed symmetric block
__device__ inline double band_mv(const double* __restrict__ Hb, const double* v, int P, int BW, int p) {
  double s = Hb[p] * v[p];
  for (int dd = 1; dd <= BW; ++dd) {
    if (p + dd < P) s += Hb[dd * P + p] * v[p + dd];
    if (p - dd >= 0) s += Hb[dd * P + p - dd] * v[p - dd];
  }
  return s;
}

__device__ inline int step_dir(const Dims& d, int s, int n_phi) {
  if (s < n_phi) {
    const int j = s / d.M, m = s - j * d.M;
    return j * d.MD + m + 1;
  }
  return (s - n_phi) * d.MD;
}

}  // namespace bfmmm
