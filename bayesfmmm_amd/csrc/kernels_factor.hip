// k_factor: the per-direction covariance factorisation of the Phi / nu block, between the pair-Gram contraction
// (kernels_pair_gram.hip) and the sweep (kernels_sweep.hip).
//
// Every Gaussian full conditional of the reference (updateNu UpdateNu.h:24-74, updatePhi UpdatePhi.h:23-89 and their
// Tempered variants) has the form
//     Prec_a = (beta/sigma^2) H_aa + Prior_a
//     rhs_a  = (beta/sigma^2) ( t_a - sum_{b != a} H_ab theta_b )
//     theta_a ~ N( C_a rhs_a, C_a ),  C_a = Prec_a^-1,   drawn as  C_a rhs_a + chol_lower(C_a) z
//
//   k_factor : per direction a, one workgroup for the reverse Cholesky of Prec_a -> chol_lower(C_a), C_a, L_a z_a and one for
//              r_a = t_a - sum_b H_ab theta_b; spare workgroups draw job_hyper's variates and prepare the next iteration's
//              Z proposals, chi normals and pi / alpha_3 tables (16 instances: PP = 32 / 64 x eight band widths)
#include "model.hpp"
#include "rng.hpp"
#include "scalar_jobs.hpp"
#include "factor_core.hpp"
#include "z_proposal.hpp"
#include "sweep_helpers.hpp"
#include "launchers.hpp"

namespace bfmmm {

#ifdef BFMMM_TIMELINE
void fetch_fct(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fct), sizeof(unsigned long long) * 8); }
#endif

// ---------------------------------------------------------------------------------------------
// k_factor: one workgroup per active direction a.
//   r_a  = t_a - sum_b H_ab theta_b,  hq_a = H_aa theta_a      (always: the sweep starts from these)
//   Prec = (beta/sigma^2) H_aa + Prior_a                        (banded: half-width BWP)
//   Prec = U U'  with U UPPER triangular ("reverse" Cholesky, processed from the last row up).
//   Then  C = Prec^-1 = U^-T U^-1  and, because U^-T is lower triangular with positive diagonal,
//   chol_lower(C) = U^-T  exactly -- the factor arma::mvnrnd(C b, C) multiplies z by
//   (UpdateNu.h:67-69, UpdatePhi.h:79-82).  So one banded factorisation + one triangular inverse
//   give both the reference's covariance C and its Cholesky factor L; no dense inverse is formed
//   by elimination.  The direction's normal variates z and L z are produced here as well, so the
//   sequential sweep only has to apply C.
// A pivot below 1e-12 of the largest diagonal entry sends the direction down the reference's arma::pinv / eigen-decomposition
// route instead (factor_pinv, factor_core.hpp).
// ---------------------------------------------------------------------------------------------
template <int PP, int BW>
// (three workgroups per CU: at four the 128-register cap spilled 62 registers of the factorisation path to scratch -- one chain
//  64.7 us per iteration against 65.6, 8 Nu_Z chains 103 k iterations/s against 100 k; the spare jobs of a batch still overlap)
__global__ __launch_bounds__(256, (BW <= 5) ? 3 : 1) void k_factor(Ctx c0) {
  // one-dimensional grid of chains x jobs with the chain index running FASTEST, so that the long factorisation workgroups
  // of every chain of a batch are dispatched before any of the short spare jobs (workgroups start in index order)
  const int nch_ = c0.nch;
  const Ctx c = chain_ctx(c0, blockIdx.x % nch_);
  const int bx = blockIdx.x / nch_;      // job index
  TIMELINE(c, 3);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Dims& d = c.d;
  const int P = d.P, MD = d.MD, K = d.K, A = d.A, M = d.M;
  constexpr int W = 2 * BW + 2;     // doubles per row of an H2 block: G(p, p - BW .. p + BW), 0
  const int tid = threadIdx.x;
  // Two workgroups per direction (round 4; not for the diagonal model, which has no factorisation): workgroup a < A runs the
  // factorisation of Prec_a -- it needs only H_aa and the prior -- and workgroup A + a forms r_a = t_a - sum_b H_ab theta_b and
  // H_aa theta_a, which the factorisation does not need: side by side on two CUs instead of one after the other (the r phase
  // was 2.2 us of the factorisation workgroup's 13).
  const bool split = !((BW == 0) && d.BWP == 0);
  const int nF0 = split ? 2 * A : A;       // first spare job
  if (c.pi_in_factor && bx == nF0) {
    // The iteration's pi / alpha_3 job (normally an extra workgroup of k_pair_gram; on the packed pair-Gram path of chain
    // batches it would cost k_pair_gram_pack or its reduction their register budget -- it needs 177 VGPRs, they 88 and 46).  The
    // one spare job that reads pi / alpha_3 of THIS iteration (job_pi_prepare, one workgroup) waits for it (wait_pi below); the
    // pi job is dispatched before it (lower workgroup index), so the wait cannot deadlock, and it is bounded anyway.
    job_pi_alpha(c, true, c0.zrec != nullptr);
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      __hip_atomic_store(&c.dyn->pi_done, c.dyn->iter + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  const int nF = nF0 + (c.pi_in_factor ? 1 : 0);
  auto wait_pi = [&]() {
    if (!c.pi_in_factor) return;
    if (tid == 0) {
      const uint32_t want = c.dyn->iter + 1u;
      int spins = 0;
      // (relaxed polls -- an acquire per poll invalidates the XCD's L2 every time, and four hundred waiting workgroups doing that
      //  made the kernel four times longer -- and ONE acquire fence once the flag is up)
      while (__hip_atomic_load(&c.dyn->pi_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
        __builtin_amdgcn_s_sleep(64);
        if (++spins > (1 << 20)) { atomicOr(&c.dyn->status, 8u); break; }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
  };
  if (bx >= nF) {       // spare workgroups: the state-independent variates of job_hyper, then next iteration's Z proposals
    const int ndraw = (hyper_gstd_count(d) + 1 + 8 * d.K + 255) / 256;
    const int zcw = zprep_curves_per_wg(d.K);
    const int nzp = (c.mask & U_Z) ? (d.n + zcw - 1) / zcw : 0;
    // Order: draws, then the ONE job that waits (next iteration's pi / alpha_3 tables: it needs this iteration's pi job, which has
    // a lower workgroup index and is therefore running by the time this one is dispatched -- no deadlock), then the short ones.  It
    // used to be the LAST workgroup of the grid: in a batch it then started when everything else had been dispatched (21 us into
    // the kernel for eight chains) and its 5.5 us were the kernel's tail.
    const int npi = (c.mask & (U_PI | U_ALPHA3)) ? 1 : 0;
    const int sb = bx - nF;
#ifdef BFMMM_TIMELINE
    // one workgroup of each kind of spare job: start / end stamps 56 .. 63
    const int kind_ = sb < ndraw ? 0 : sb < ndraw + npi ? 2 : sb < ndraw + npi + nzp ? 1 : 3;
    const bool first_ = (sb == 0) || kind_ == 2 || (sb == ndraw + npi && nzp > 0) || (kind_ == 3 && sb == ndraw + npi + nzp);
    if (first_ && threadIdx.x == 0) c.dyn->stamps[56 + 2 * kind_] = wall_clock64();
#endif
    if (sb < ndraw) job_hyper_draws(c, sb * 256);
    else if (sb < ndraw + npi) { wait_pi(); job_pi_prepare(c); }
    else if (sb < ndraw + npi + nzp) job_z_prepare(c, sb - ndraw - npi);      // (does not read pi / alpha_3: z_proposal.hpp)
    else job_chi_normals(c, sb - ndraw - npi - nzp);
#ifdef BFMMM_TIMELINE
    if (first_ && threadIdx.x == 0) c.dyn->stamps[57 + 2 * kind_] = wall_clock64();
#endif
    return;
  }
  const bool role_r = split && bx >= A;      // this workgroup forms r_a, H_aa theta_a (and, without the split, everything)
  const bool role_f = !role_r;               // this workgroup factorises
  const bool do_r = role_r || !split;
  const int a = role_r ? bx - A : bx;
  const int j = a / MD, mt = a - j * MD;
#ifdef BFMMM_TIMELINE
#define FST(i) do { if (bx == 1 && threadIdx.x == 0) c.dyn->stamps[48 + (i)] = wall_clock64(); } while (0)
#else
#define FST(i) do { } while (0)
#endif
  FST(0);
  const int AP = A * P, PS = P + 2 * BW + 1;
  // diagonal model (multivariate: G_i = I, prior (1 / tau) I or diag(gamma)): the precision is a diagonal, no P x P work
  // areas -- the launch then asks for 10 KB of LDS instead of 75, and the spare jobs of this kernel (which need none of it) fit
  // five to a CU instead of two
  const bool diag = (BW == 0) && d.BWP == 0;
  double* S = smem;                 // PP x PP : Prec (col-major, S[i + PP*k])
  double* X = S + PP * PP;          // PP x PP : U^-1, row-major X[i*PP + c]
  double* thp = diag ? smem : X + PP * PP;        // A x PS : theta_b with BW zero pads before and BW + 1 after
  double* part = thp + A * PS;      // A x P  : (H_ab theta_b)[p]
  double* zv = part + AP;           // PP
  double* hb2 = zv + PP;            // P x W  : rows of H_aa
  double* dsc = hb2 + P * W;        // 16     : delta(j, .)
  const bool upd_nu = (mt == 0) && (c.mask & U_NU);
  const bool upd_phi = (mt > 0) && (c.mask & U_PHI);
  const bool upd = upd_nu || upd_phi;
  const Dyn* dyn = c.dyn;
  // ---- everything this workgroup needs from global memory is requested up front, in one batch ----
  constexpr int MAXI = (BW > 5) ? 1 : 4;          // (b, p) items per thread and pass (wide band: a row is 64 doubles)
  v2d hreg[MAXI][BW + 1];
  double tval[MAXI];
  const bool upd_nu0 = (mt == 0) && (c.mask & U_NU), upd_phi0 = (mt > 0) && (c.mask & U_PHI);
  if (split && role_f && !(upd_nu0 || upd_phi0)) return;      // (a direction that is not sampled needs only its r workgroup)
  if (do_r) {
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
      const int e = min(tid + 256 * it, AP - 1);
      const int b = e / P, p = e - b * P;
      tval[it] = c.theta[(size_t)full_dir(d, b) * P + p];
      const v2d* blk = (const v2d*)(c.H2 + (size_t)hrow(d, a, b) * P * W);
#pragma unroll
      for (int k = 0; k <= BW; ++k) hreg[it][k] = blk[k * P + p];
    }
  } else {
    // factorisation workgroup: row p = tid of H_aa only
    const v2d* blk = (const v2d*)(c.H2 + (size_t)hrow(d, a, a) * P * W);
    const int p = min(tid, P - 1);
#pragma unroll
    for (int k = 0; k <= BW; ++k) hreg[0][k] = blk[k * P + p];
  }
  const double tv0 = do_r ? c.tvec[a * P + min(tid >> 3, P - 1)] : 0.0;      // t_a[p] of the r-reduction's first pass
  // prior entries of the band of Prec this thread will build: element (p, p + t), t <= BWP (two per thread at most)
  constexpr int NPRI = (BW > 5) ? ((BWWIDE + 1) * PP + 255) / 256 : 2;
  double pri[NPRI];
#pragma unroll
  for (int u = 0; u < NPRI; ++u) {
    const int e = tid + 256 * u, t = e / PP, p = e - t * PP, q = p + t;
    const bool in = t <= d.BWP && q < P;
    const int pc = min(p, P - 1), qc = min(q, P - 1);
    double v = 0.0;
    if (mt == 0) v = d.mv ? 0.0 : c.Pmat[pc + (size_t)P * qc];
    else v = c.gamma[j + (size_t)K * (pc + (size_t)P * (mt - 1))];
    pri[u] = (in && (mt == 0 || t == 0)) ? v : 0.0;
  }
  const double dlt = (mt > 0 && tid < M) ? c.delta[j + (size_t)K * tid] : 1.0;
  const double f = dyn->beta / dyn->sigma2;
  const double tau_j = dyn->tau[j];
  if (do_r) for (int x = tid; x < A * PS; x += 256) thp[x] = 0.0;
  if (role_f && upd && tid >= 64 && tid < 64 + P) {     // the direction's normal variates, while the loads are in flight
    const RngKey key = make_key(c.seed, c.chain, dyn->iter, dyn->tt_step);
    const uint32_t idx0 = (mt == 0) ? (uint32_t)(j * P) : (uint32_t)((j * M + (mt - 1)) * P);
    zv[tid - 64] = rnorm(key, (mt == 0) ? UPD_NU : UPD_PHI, idx0 + (uint32_t)(tid - 64));
  }
  FST(1);
  __syncthreads();
  FST(2);
  if (!do_r) {
    // factorisation workgroup of a split launch: the rows of H_aa straight to the precision's work area
    if (tid < P) {
#pragma unroll
      for (int k = 0; k <= BW; ++k) { hb2[tid * W + 2 * k] = hreg[0][k].x; hb2[tid * W + 2 * k + 1] = hreg[0][k].y; }
    }
    if (tid < 16) dsc[tid] = dlt;
    __syncthreads();
  }
  if (do_r) {
#pragma unroll
  for (int it = 0; it < MAXI; ++it) {
    const int e = tid + 256 * it;
    if (e < AP) { const int b = e / P, p = e - b * P; thp[b * PS + BW + p] = tval[it]; }
  }
  for (int e = tid + 256 * MAXI; e < AP; e += 256) {     // beyond the batched part (more than 1024 elements)
    const int b = e / P, p = e - b * P;
    thp[b * PS + BW + p] = c.theta[(size_t)full_dir(d, b) * P + p];
  }
  if (tid < 16) dsc[tid] = dlt;
  __syncthreads();
  // ---- (H_ab theta_b)[p] for every b; the rows of H_aa are kept for the precision matrix ----
  for (int base = 0; base < AP; base += 256 * MAXI) {
    if (base > 0) {                 // more than 1024 elements: further passes reload their rows (rare)
#pragma unroll
      for (int it = 0; it < MAXI; ++it) {
        const int e = min(base + tid + 256 * it, AP - 1);
        const int b = e / P, p = e - b * P;
        const v2d* blk = (const v2d*)(c.H2 + (size_t)hrow(d, a, b) * P * W);
#pragma unroll
        for (int k = 0; k <= BW; ++k) hreg[it][k] = blk[k * P + p];
      }
    }
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
      const int e = base + tid + 256 * it;
      if (e < AP) {
        const int b = e / P, p = e - b * P;
        const double* tb = thp + b * PS + p;        // tb[k] = theta_b[p + k - BW]
        double v = 0.0;
#pragma unroll
        for (int k = 0; k <= BW; ++k) v += hreg[it][k].x * tb[2 * k] + hreg[it][k].y * tb[2 * k + 1];
        part[e] = v;
        if (b == a) {
#pragma unroll
          for (int k = 0; k <= BW; ++k) { hb2[p * W + 2 * k] = hreg[it][k].x; hb2[p * W + 2 * k + 1] = hreg[it][k].y; }
        }
      }
    }
  }
  __syncthreads();
  FST(3);
  // ---- r_a = t_a - sum_b H_ab theta_b : 8 lanes per p, fixed summation order ----
  for (int p0 = 0; p0 < P; p0 += 32) {
    const int p = p0 + (tid >> 3), g = tid & 7;
    double acc = 0.0;
    if (p < P)
      for (int b = g; b < A; b += 8) acc += part[b * P + p];
    acc = dpp_add<0xB1>(acc);
    acc = dpp_add<0x4E>(acc);
    acc = dpp_add<0x141>(acc);
    const double tvp = (p0 == 0) ? tv0 : c.tvec[a * P + min(p, P - 1)];
    if (p < P && g == 0) {
      c.rvec[a * P + p] = tvp - acc;
      c.hq[a * P + p] = part[a * P + p];
    }
  }
  FST(4);
  }      // do_r
  if (role_r || !upd) return;
  // prior scale: tau_j (nu) or tilde_tau(j, m) = prod_{m' <= m} delta(j, m') (BFMMM.h:1514-1519)
  double tt = 1.0;
  for (int m2 = 0; m2 < mt; ++m2) tt *= dsc[m2];
  if (diag) {
    // C = diag(1 / d_p), chol_lower(C) = diag(1 / sqrt(d_p)), L z likewise (the same estimate + two Newton steps as
    // factor_core's diagonal branch, so the factor is the same function of the pivot).  d_p > 0 always: the prior term is.
    double* Cg = c.Cmat + (size_t)a * P * P;
    for (int e = tid; e < P * P; e += 256) {
      const int p = e % P, q = e / P;
      double cv = 0.0;
      if (p == q) {
        double dk = f * hb2[p * W + BW];
        if (mt == 0) dk += d.mv ? 1.0 / tau_j : tau_j * c.Pmat[p + (size_t)P * p];     // UpdateNu.h:197 (MV) / :66
        else dk += tt * c.gamma[j + (size_t)K * (p + (size_t)P * (mt - 1))];            // UpdatePhi.h:76-78
        double rk = __builtin_amdgcn_rsq(dk);
        rk = rk * (1.5 - (0.5 * dk) * (rk * rk));
        rk = rk * (1.5 - (0.5 * dk) * (rk * rk));
        if (!(dk > 0.0)) atomicOr(&c.dyn->status, 1u);
        cv = rk * rk;
        c.Lz[(size_t)a * P + p] = rk * zv[p];
      }
      Cg[q + (size_t)P * p] = cv;
    }
    FST(6);
    return;
  }
  // only the band of Prec is read by the factorisation (factor_core): (BWP + 1) x P entries
  auto build_prec = [&](bool full) {     // full: the whole symmetric matrix (pseudo-inverse route)
    for (int e = tid; e < PP * PP; e += 256) X[e] = 0.0;
    if (BW > 5 || full) {             // the dense factorisation / the Jacobi rotations read all of S
      for (int e = tid; e < PP * PP; e += 256) S[e] = (!full && e % PP == e / PP) ? 1.0 : 0.0;
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NPRI; ++u) {
      const int e = tid + 256 * u, t = e / PP, p = e - t * PP, q = p + t;
      if (t <= d.BWP && q < P) {
        double v = (t <= BW) ? f * hb2[p * W + BW + t] : 0.0;
        if (mt == 0) v += d.mv ? ((t == 0) ? 1.0 / tau_j : 0.0) : tau_j * pri[u];    // UpdateNu.h:197 (MV) / :66
        else v += tt * pri[u];                                                       // UpdatePhi.h:76-78 (diagonal)
        S[p + PP * q] = v;
        if (BW > 5 || full) S[q + PP * p] = v;
      }
    }
    __syncthreads();
  };
  build_prec(false);
  FST(5);
  double* wkp = dsc + 16;             // 4 PP + 2 doubles: scratch of the pseudo-inverse route
  // (the factor L itself is not stored: the sweep needs only C_a and L_a z_a, and the store sat at the end of this kernel's
  //  critical path)
  if (factor_core<PP>(S, X, zv, P, d.BWP, c.Cmat + (size_t)a * P * P, nullptr, c.Lz + (size_t)a * P, tid, nullptr)) {
    // singular to working accuracy (e.g. a cluster without members: Prec = tau P_mat): arma::pinv + the eigen route of
    // arma::mvnrnd in the reference (UpdateNu.h:67-69), factor_pinv here
    build_prec(true);
    factor_pinv<PP>(S, X, zv, P, c.Cmat + (size_t)a * P * P, nullptr, c.Lz + (size_t)a * P, tid, wkp);
  }
  FST(6);
}

template <int PP>
static void launch_factor_pp(const Ctx& c, int grid, size_t lds, hipStream_t st) {
  switch (c.d.BW) {
    case 0: hipLaunchKernelGGL((k_factor<PP, 0>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    case 1: hipLaunchKernelGGL((k_factor<PP, 1>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    case 2: hipLaunchKernelGGL((k_factor<PP, 2>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    case 3: hipLaunchKernelGGL((k_factor<PP, 3>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    case 4: hipLaunchKernelGGL((k_factor<PP, 4>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    case 5: hipLaunchKernelGGL((k_factor<PP, 5>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    case BWMID: hipLaunchKernelGGL((k_factor<PP, BWMID>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
    default: hipLaunchKernelGGL((k_factor<PP, BWWIDE>), dim3(c.nch * grid), dim3(256), lds, st, c); break;
  }
}

void launch_factor(const Ctx& c, hipStream_t st) {
  const int PP = (c.d.P <= 32) ? 32 : 64;
  const int W = 2 * c.d.BW + 2, PS = c.d.P + 2 * c.d.BW + 1;
  const bool diag = c.d.BW == 0 && c.d.BWP == 0;       // no P x P work areas (k_factor)
  const size_t lds = ((diag ? 0 : 2 * (size_t)PP * PP) + (size_t)c.d.A * PS + (size_t)c.d.A * c.d.P + PP + (size_t)c.d.P * W + 16 + 4 * PP + 2) * sizeof(double);
  const int n_draw = c.d.K * c.d.P * c.d.M + c.d.K * c.d.M + c.d.K + 4 * c.d.K + 1 + 8 * c.d.K;   // + sigma^2's gamma variate, A terms
  const int zcw = zprep_curves_per_wg(c.d.K);       // curves per workgroup of job_z_prepare (z_proposal.hpp)
  const int n_zprep = (c.mask & U_Z) ? (c.d.n + zcw - 1) / zcw : 0;      // (covariate-adjusted models too: the proposal does not see the data)
  const int n_znorm = ((c.mask & U_CHI) && c.d.MD > 1) ? (c.d.n * c.d.M + 255) / 256 : 0;
  const int n_pi = (c.mask & (U_PI | U_ALPHA3)) ? 1 : 0;          // next iteration's pi / alpha_3 tables (right behind the draws)
  const int grid = (diag ? 1 : 2) * c.d.A + (c.pi_in_factor ? 1 : 0) + (n_draw + 255) / 256 + n_zprep + n_znorm + n_pi;      // (k_factor: two workgroups per direction)
  if (PP == 32) launch_factor_pp<32>(c, grid, lds, st);
  else launch_factor_pp<64>(c, grid, lds, st);
}

void prepare_factor_kernels() {
  set_max_lds((const void*)k_factor<32, 0>); set_max_lds((const void*)k_factor<64, 0>);
  set_max_lds((const void*)k_factor<32, 1>); set_max_lds((const void*)k_factor<64, 1>);
  set_max_lds((const void*)k_factor<32, 2>); set_max_lds((const void*)k_factor<64, 2>);
  set_max_lds((const void*)k_factor<32, 3>); set_max_lds((const void*)k_factor<64, 3>);
  set_max_lds((const void*)k_factor<32, 4>); set_max_lds((const void*)k_factor<64, 4>);
  set_max_lds((const void*)k_factor<32, 5>); set_max_lds((const void*)k_factor<64, 5>);
  set_max_lds((const void*)k_factor<32, BWMID>); set_max_lds((const void*)k_factor<64, BWMID>);
  set_max_lds((const void*)k_factor<32, BWWIDE>); set_max_lds((const void*)k_factor<64, BWWIDE>);
}

}  // namespace bfmmm
