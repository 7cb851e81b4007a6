"""High-precision restatement of the per-curve updates (csrc/kernels_curve.hip: k_curve_chi, k_curve_z, its lean form and the Z
update fused into k_curve_chi), their per-entry checks, bounds, two float64 emulations and the case list shared by
tests/test_curve_update_ref.py (CPU) and tests/test_gpu_curve_update.py (device).  (Test infrastructure.)

Inputs are the DEVICE's own records rec_i = [G_i band rows | s_i | yy_i] (bfmmm_debug_get "rec"), so the record builder's rounding
stays out of this test, with the pushed state or the chain slots the judged update started from.  Everything below is
np.longdouble.  Curve i sees row r = (k, mt) of the parameters as th_r = theta_r + sum_d x_id thetaX_{r,d} (no covariates: theta_r);
mt = 0 is nu_k, mt = m + 1 is phi_km.  u = 2^-53.

chi (UpdateChi.h:19-64 in Gram form), per curve:
    u_m = sum_k Z_k th_{k,m+1},   c0 = sum_k Z_k th_{k,0} + sum_m chi_m u_m,   A = U'GU,   b = U'(s - G c0)
    step m:  r_m = b_m - sum_{m2 < m} A_{m2,m} dl_m2,   W_m = 1 / (1 + A_mm f),   f = beta / sigma^2,
             chi_ref,m = W_m f (r_m + chi_m A_mm) + sqrt(W_m) z_m
Each step is judged ALONE: dl_m2 = chi_new,m2 - chi_old,m2 of the DEVICE's earlier steps (exact in longdouble), z_m is "chi_norm"
as the device holds it.  Bound per entry (check_chi), G_CHI times

    W f E_r + W f |chi_m| c_A u Sa_mm + |f (r_m + chi_m A_mm) + z_m / (2 sqrt W)| W^2 f c_A u Sa_mm
      + 8 u (W f (|r_m| + |chi_m| A_mm) + |chi_m| + sqrt(W) |z_m|) + u |chi_ref,m|
    E_r = (c_b + m + 1) u Sb_m + sum_{m2 < m} ((c_A + m + 1) u Sa_{m2,m} |dl_m2| + u Sa_{m2,m} |chi_new,m2|)

with the sums of absolute terms  ua_m = sum_k |Z_k| |th|_{k,m+1}  (|th| = |theta| + sum_d |x_d| |thetaX|),  c0a = sum_k |Z_k| |th|_{k,0} +
sum_m |chi_m| ua_m,  Sb_m = ua_m'(|s| + |G| c0a),  Sa = Ua'|G|Ua  and the term counts (roundings a term passes at most)
    n_u = K (1 + D) + 2      a term Z_k x_d thetaX of u_m: two products, K (1 + D) additions
    n_c = n_u + M + 2        a term of c0: through u_m, one product, M + 1 additions
    c_b = n_u + n_c + (2 BW + 3) + LPC + 1     u_m'(s - G c0): the band product (2 BW + 1 additions, a product), the subtraction,
                                               LPC additions of the dot product in any order and its product
    c_A = 2 n_u + (2 BW + 2) + LPC + 1         u_m2'G u_m
First line: the error of r_m through W f; the error of A_mm where it multiplies chi_m; the error of A_mm through W (dW = -W^2 f dA).
Second line: the CANCELLATION the kernel's folded constant c3 = c1 chi A_mm + (sqrt(W) z - chi) carries (c1 = W f: in the stiff
regime c1 A_mm is 1 - 1e-3 and the two terms of size |chi| cancel), eight roundings for f, the reciprocal, the rsqrt, the
normal variate and the sums, on every term by its modulus; u |chi_ref|: chi_new = fl(chi_old + dl).  The rounding of dl recovered
as a difference is the last term of E_r.  Nothing is scaled by a global maximum.

Residual sums.  rss_part[b] against sum_{i in b} (yy - 2 c's + c'Gc) at the final chi, c = c0 + sum_m dl_m u_m, under G_RSS times
c_R u S_abs, S_abs = sum_i max(form 1, form 2): form 1 = |yy| + 2 ca'|s| + ca'|G|ca (ca = c0a + sum |dl_m| ua_m), form 2 (the kernel's:
rss at c0, then the update) = |yy| + c0a'|s| + c0a'(|s| + |G| c0a) + sum_m |dl_m| (2 Sb_m + sum_m2 |dl_m2| Sa_{m,m2});
c_R = n_c + (2 BW + 3) + LPC + 2 M + 6 + GPB.  An idle group (curve index >= n) must add nothing.  Dyn::rss against the sum of the
parts under (nblk + 10) u sum |part|; the log-likelihood (CalculateLikelihood.h:19-44, :140-160) from that RSS:
    functional    -N (0.918938533204672742 + log sqrt(sigma^2)) - RSS / (2 sigma^2)
    multivariate  -n ((P / 2) log(2 pi sigma^2)) - RSS / (2 sigma^2)        (P / 2: integer division)
under 8 u (|first term| + |second term|): a log, a square root, a division, three products and the sum.

Z (UpdateMixedMembership.h:131-185).  u_k = th_{k,0} + sum_m chi_m th_{k,m+1},  a_k = u_k's,  Q = U'GU,
    q(Z) = yy + sum_k Z_k (-2 a_k + sum_k2 Z_k2 Q_{k,k2}),
    acc_ref = (pr_new - pr_old + lpo - lpn) - beta (q(Z_new) - q(Z_old)) / (2 sigma^2)
with pr_*, lp*, Z_new from the device's record ("z_record", bfmmm_set_curve_record): the acceptance value itself is recorded, so
NO curve is left undecided.  Bound (check_z), G_ACC times
    f/2 c_q u (Sq(Z_old) + Sq(Z_new)) + 4 u (|pr_new| + |pr_old| + |lpo| + |lpn| + |acc_ref|)
    Sq(Z) = |yy| + sum_k |Z_k| (2 aa_k + sum_k2 |Z_k2| Qa_{k,k2}),   aa = Ua'|s|,  Qa = Ua'|G|Ua,  ua_k = |th|_{k,0} + sum_m |chi_m| |th|_{k,m+1}
    c_q = 2 n_z + (2 BW + 2) + LPC + 1 + 2 K + 4,   n_z = (M + 1)(1 + D) + 2
(the kernel forms q_old and q_new WITH yy, scales each by beta / 2 sigma^2 and subtracts: |yy| is in Sq twice on purpose).
Decision and outputs: Z_out is bit-equal to the recorded Z_new where log_uu < acceptance (the device's value) and to Z_old
otherwise; a curve with a Z_old,k <= 0 has acceptance == 1 exactly and takes the proposal; logz_part[b, k] against
sum_{i in b} log Z_out,ik under (GPB + 4) u sum |log Z_out,ik|.  pr_old and pr_new against sum_k (alpha_3 pi_k - 1) log Z_k with the pi
and alpha_3 the update must use (check_prior_terms).  log_uu against the log of the oracle's keyed uniform (UPD_Z_ACC,
index i) under 4 u |log u| + 2 u: the same uniform through two log implementations of at most 2 ulp each.

Constants.  G_CHI, G_ACC, G_RSS are 4 x the largest error / (bound with G = 1) that two float64 emulations show over every case:
`kernel` follows the kernels' order of operations (zrow's k-then-d sums, the band product diagonal first, four-accumulator dot
products, the two-lane half dots of z_forms, one chain per k in q_old / q_new, the lane-owned Gauss-Seidel recursion with folded
c1 / c3, the 16-lane butterfly of the residual update), `plain` a plainly different valid order (BLAS products, the textbook
recursion, the residual at the final coefficient).  They come from the emulations, never from a device run
(tests/test_curve_update_ref.py recomputes them and asserts they have not grown):

    chi step:   kernel 0.0236 (mv_P7_K2M4-benign),       plain 0.0289 (cubic_P30_K2M1-benign)    ->  G_CHI = 0.12
    acceptance: kernel 0.0194 (lin_P6-benign),           plain 0.00841 (mv_P7_K2M3-benign)       ->  G_ACC = 0.08
    rss_part:   kernel 0.00944 (cubic_P40_K2M1-benign),  plain 0.011 (mv_P40_K3M1-benign)        ->  G_RSS = 0.045
    stil:       kernel 0.148, plain 0.148 (cubic_P30_K3M2_D2-benign)                            ->  G_STIL = 0.6
    yyp_part:   kernel 0.0151 (cubic_P30_K2M7_D2-benign), plain 0.0128 (cubic_P30_K2M6_D2-benign) ->  G_YYP = 0.065
    cfull:      kernel 0.151 (cubic_P30_K3M1_D2-benign), plain 0.111 (cubic_P30_K2M1_D2-benign)  ->  G_CF = 0.61
    gfull:      kernel 0.0423, plain 0.0452 (cubic_P30_K2M2_D2-benign)                          ->  G_GF = 0.185

Every bound must stay below 1e-3 of the change it judges (|dl_m|; |q_new - q_old| f / 2): asserted on the CPU for every case
and reported by the device test.

Covariate models: stil and yyp_part, which only k_curve_z writes, are checked by check_stil, and cfull / gfull, which k_curve_chi
writes, by check_cfull (bounds in their docstrings).  launch_cov_block stores to cfull / gfull only behind an eta / Xi step, so
after a run whose mask has neither U_ETA nor U_XI k_curve_chi's values are still there; it rewrites rss_part in every iteration,
which is why the rss_part check is for D = 0 only.

The data-independent half of the proposal (check_proposal): Z_new against the oracle's K keyed gamma variates (UPD_Z_PROP, shape
a_Z_PM Z_old,k, 10 where that is <= 0) normalised in longdouble; lpn and lpo against longdouble log / lgamma densities at the
recorded Z_new; pr_old / pr_new and log_uu as above.  These tolerances cannot be derived (two gamma rejection samplers through
different log / pow): they are MEASURED, the oracle's float64 arithmetic against the longdouble restatement over every case, in
units of u -- Z_new 2.94 (relative), lpn 2.01, lpo 2.3 (of their sums of absolute terms) -- and the device's own libm gets 4 x
that.  reference_z is the whole update from the oracle's variates; tests/test_curve_update_ref.py holds it to the oracle's
updateZ_PM (1e-9).  The functions that fetch keyed variates take tt (the sweep of a tempered-transition block, counter word
tt_step; 0: a plain iteration): tests/test_gpu_tempered_steps.py runs them on the in-place branches of tempered sweeps.  Not restated
here: kernels_cov.hip (tests/cov_ref.py), the scalar jobs (tests/scalar_jobs_ref.py).
"""
import zlib

import numpy as np

import factor_ref as F
import sweep_ref as S

U, LD = F.U, F.LD
SEED = F.SEED
UPD_Z_PROP, UPD_Z_ACC, UPD_CHI = 1, 2, 15          # update ids of the keyed generator (oracle/oracle.h, csrc/rng.hpp)
N_CURVES = 21                       # idle groups at both 8 and 4 curves per workgroup
LOG_SQRT_2PI = LD("0.918938533204672741780329736406")

# measured by tests/test_curve_update_ref.py::test_emulations_pass_and_constants_hold (largest error / bound at G = 1)
MEASURED_CHI = {"kernel": 0.0236, "plain": 0.0289}
MEASURED_ACC = {"kernel": 0.0194, "plain": 0.00841}
MEASURED_RSS = {"kernel": 0.00944, "plain": 0.011}
MEASURED_STIL = {"kernel": 0.148, "plain": 0.148}
MEASURED_YYP = {"kernel": 0.0151, "plain": 0.0128}
G_CHI, G_ACC, G_RSS, G_STIL, G_YYP = 0.12, 0.08, 0.045, 0.6, 0.065
MEASURED_CF = {"kernel": 0.151, "plain": 0.111}
MEASURED_GF = {"kernel": 0.0423, "plain": 0.0452}
G_CF, G_GF = 0.61, 0.185
# measured by tests/test_curve_update_ref.py::test_proposal_tolerances_have_not_grown: the oracle's float64 arithmetic against the
# longdouble restatement over every case, in units of u (of Z_new; of the sums of absolute terms of lpn, lpo); the device's own
# libm gets PROP_MARGIN x that
MEASURED_PROP = {"Znew": 2.94, "lpn": 2.01, "lpo": 2.3}
PROP_MARGIN = 4.0
EMU_LIMIT = 0.25
NONVACUOUS = 1e-3

# update mask bits (bayesfmmm_amd.sampler's; asserted in tests/test_gpu_curve_update.py)
U_Z, U_PI, U_ALPHA3, U_NU, U_TAU, U_SIGMA, U_CHI, U_LOGLIK = 1, 2, 4, 1 << 7, 1 << 8, 1 << 9, 1 << 10, 1 << 17
MASK_CHI = U_CHI | U_LOGLIK
MASK_LOGZ = U_PI | U_ALPHA3          # k_curve_z with do_update == 0: only the block sums of log Z
MASK_LEAN = U_Z | U_PI | U_ALPHA3 | U_NU | U_TAU | U_SIGMA
KMAX, MMAX = 8, 16
CHI_EXACT_COMBOS = ((3, 32, False), (3, 64, False), (3, 32, True), (0, 32, False), (0, 64, False))      # BFMMM_CHI_EXACT_COMBOS


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class CurveCase(F.Case):
    """factor_ref.Case at n = 21 curves, with D covariates and the special states of the Z update"""
    def __init__(self, name, D=0, zero=False, **kw):
        super().__init__(name=name, **kw)
        self.n, self.D, self.zero = N_CURVES, D, zero
        self.LPC = 32 if self.P <= 32 else 64
        self.GPB = 256 // self.LPC
        self.nblk = -(-self.n // self.GPB)

    @property
    def data_key(self):
        return ("curve", self.n) + super().data_key

    def exact_built(self):
        return (self.BW, self.LPC, self.D > 0) in CHI_EXACT_COMBOS


def _case(name, regime="benign", special=None, **kw):
    return CurveCase(name=f"{name}-{special or regime}", regime=regime, special=special, **kw)


_INST = {d["name"]: d for d in F._INST}


def _inst(name, regime="benign", special=None, suffix="", **kw):
    d = dict(_INST[name])
    d.update(kw)
    d["name"] = name + suffix
    return _case(regime=regime, special=special, **d)


def _cases():
    out = [_inst(i) for i in _INST]                                   # every band class at both LPC: P = 32, 33, 64, 6 among them
    out += [_inst("cubic_P30", "stiff"), _inst("mv_P7", "stiff")]
    sp = dict(kind="spline", deg=3)
    # K / M edges, 32 lanes: K = 5 and 7 one lane per form, K = 8 a second trip of q += LPC; odd M (the sChi[M] pad); M = 9 past SMALL;
    # K (M + 1) P = 1200 > 1024 (the copy_to_lds tail); 64 lanes: K = 7, 8 one lane per form
    out += [_case("cubic_P30_K2M1", P=30, K=2, M=1, **sp), _case("cubic_P30_K4M8", P=30, K=4, M=8, **sp),
            _case("cubic_P30_K3M7", P=30, K=3, M=7, **sp), _case("cubic_P30_K5M7", P=30, K=5, M=7, **sp),
            _case("cubic_P30_K7M9", P=30, K=7, M=9, **sp), _case("cubic_P30_K8M3", P=30, K=8, M=3, **sp),
            _case("cubic_P30_K2M15", P=30, K=2, M=15, **sp), _case("cubic_P30_K2M16", P=30, K=2, M=16, **sp),
            _case("cubic_P40_K6M2", P=40, K=6, M=2, **sp), _case("cubic_P40_K7M1", P=40, K=7, M=1, **sp),
            _case("cubic_P40_K8M2", P=40, K=8, M=2, **sp), _case("cubic_P40_K3M7", P=40, K=3, M=7, **sp)]
    # exact instances: all 24 (K, M) pairs on each of the five built combinations (BW, LPC, COV)
    have = {c.name for c in out}
    for K in (2, 3, 4):
        for M in range(1, 9):
            for cs in (_case(f"cubic_P30_K{K}M{M}", P=30, K=K, M=M, **sp), _case(f"cubic_P40_K{K}M{M}", P=40, K=K, M=M, **sp),
                       _case(f"cubic_P30_K{K}M{M}_D2", P=30, K=K, M=M, D=2, **sp), _case(f"mv_P7_K{K}M{M}", kind="mv", P=7, K=K, M=M),
                       _case(f"mv_P40_K{K}M{M}", kind="mv", P=40, K=K, M=M)):
                if cs.name not in have:
                    out.append(cs)
    # covariates: exact (P <= 32) and general (P > 32)
    out += [_case("cubic_P30_D1", P=30, K=3, M=2, D=1, **sp), _case("cubic_P30_D5", P=30, K=3, M=2, D=5, **sp),
            _case("cubic_P40_D8", P=40, K=3, M=2, D=8, **sp)]
    # special states
    out += [_inst("cubic_P30", special="prior"), _inst("cubic_P30", suffix="_zero", zero=True),
            _inst("cubic_P30", suffix="_4chains", nch=4)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), [c.name for c in CASES]
BETA_CASE = "cubic_P30-benign"      # also run at beta = 0.37


def case_X(c):
    rng = np.random.default_rng(zlib.crc32(("X" + c.name).encode()))
    return rng.standard_normal((c.n, c.D)) if c.D else None


def case_state(c, q=0):
    """factor_ref.case_state, a Z with exact zeros (one per curve on a third of the curves) for the `zero` cases, and eta / xi"""
    st = F.case_state(c, q)
    rng = np.random.default_rng(zlib.crc32(("cu" + c.name).encode()) + 31 * q)
    if c.zero:
        Z = st["Z"]
        for i in range(0, c.n, 3):
            Z[i, i % c.K] = 0.0
            Z[i] /= Z[i].sum()
    if c.D:
        st["eta"] = 0.4 * rng.standard_normal((c.P, c.D, c.K))
        st["xi"] = 0.1 * rng.standard_normal((c.P, c.D, c.M, c.K))
    return st


def host_rec(c):
    """the records computed on the host in float64 from the basis rows (CPU tests; the device's differ by rounding):
    (n, LREC) with LREC = (BW + 1) P + P + 1 padded to even"""
    d = F.case_data(c)
    n, P, BW = c.n, c.P, c.BW
    LG = (BW + 1) * P
    rec = np.zeros((n, (LG + P + 2) // 2 * 2))
    for i in range(n):
        if c.kind == "mv":
            G, s, yy = np.eye(P), d["Y"][i], float(d["Y"][i] @ d["Y"][i])
        else:
            B, y = d["B"][i], d["y"][i]
            G, s, yy = B.T @ B, B.T @ y, float(y @ y)
        for t in range(min(BW, P - 1) + 1):
            rec[i, t * P:t * P + P - t] = np.diagonal(G, t)
        rec[i, LG:LG + P], rec[i, LG + P] = s, yy
    return rec


def split_rec(c, rec):
    """(G band rows (n, BW + 1, P), s (n, P), yy (n)) of the records, float64"""
    rec = np.asarray(rec, dtype=np.float64).reshape(c.n, -1)
    LG = (c.BW + 1) * c.P
    return rec[:, :LG].reshape(c.n, c.BW + 1, c.P), rec[:, LG:LG + c.P], rec[:, LG + c.P]


def expected_route(c, kind, exact=True, pcz=False):
    """what "curve_route" must report after a run of `kind` ("chi", "z", "logz", "lean", "fused", "prepared")"""
    cov = c.D > 0
    ex = exact and c.exact_built()
    M = c.M
    kex = ex and c.K in (2, 3, 4)
    small = c.K <= 4 and M <= 8
    mx = ex and c.K in (2, 3, 4) and 1 <= M <= 8
    z = dict(form=None, BW=-1, LPC=0, COV=False, KT=0, KEX=False)
    zs = dict(form="standalone", BW=c.BW, LPC=c.LPC, COV=cov, KT=c.K if kex else (4 if c.K <= 4 else KMAX), KEX=kex)
    chi = dict(BW=c.BW, LPC=c.LPC, COV=cov, SMALL=small, KX=c.K if mx else 0, MX=M if mx else 0, mode=0, fuse=False)
    if kind == "chi":
        chi["mode"] = 2
        return dict(z=zs if cov else z, chi=chi)      # (covariate models run k_curve_z in every iteration: s~_i)
    if kind in ("z", "prepared", "logz"):
        chi["mode"] = 1 if cov else 0
        return dict(z=zs, chi=chi)
    if kind == "lean":
        chi["mode"] = 1 if cov else 0
        if not cov and c.K <= 4 and c.BW <= 5:
            zs["form"] = "lean"
        return dict(z=zs, chi=chi)
    assert kind == "fused"
    chi["mode"] = 2 if not pcz else 1
    if cov:
        return dict(z=zs, chi=chi)
    chi["fuse"] = True
    return dict(z=dict(form="fused", BW=c.BW, LPC=c.LPC, COV=False, KT=c.K if mx else (4 if small else KMAX), KEX=mx), chi=chi)


# ---------------------------------------------------------------------------------------------------------------------
# the longdouble restatement
# ---------------------------------------------------------------------------------------------------------------------
def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def theta_rows(c, st, X, M, dtype=LD):
    """th[i, k, mt, p] as curve i sees it and its sum of absolute terms, mt = 0 .. M"""
    K, P, n = c.K, c.P, c.n
    th = np.zeros((K, M + 1, P), dtype=dtype)
    th[:, 0] = np.asarray(st["nu"], dtype=np.float64).astype(dtype)
    for m in range(M):
        th[:, m + 1] = np.asarray(st["Phi"], dtype=np.float64)[:, :, m].astype(dtype)
    tha = np.abs(th)
    th, tha = np.broadcast_to(th, (n,) + th.shape).copy(), np.broadcast_to(tha, (n,) + tha.shape).copy()
    if c.D:
        tx = np.zeros((K, M + 1, c.D, P), dtype=dtype)
        tx[:, 0] = np.transpose(np.asarray(st["eta"], dtype=np.float64), (2, 1, 0)).astype(dtype)
        for m in range(M):
            tx[:, m + 1] = np.transpose(np.asarray(st["xi"], dtype=np.float64)[:, :, m, :], (2, 1, 0)).astype(dtype)
        Xl = np.asarray(X, dtype=np.float64).astype(dtype)
        th = th + np.einsum("id,kmdp->ikmp", Xl, tx)
        tha = tha + np.einsum("id,kmdp->ikmp", np.abs(Xl), np.abs(tx))
    return th, tha


def counts(c, M):
    n_u = c.K * (1 + c.D) + 2
    n_c = n_u + M + 2
    return dict(n_u=n_u, n_c=n_c, c_b=n_u + n_c + 2 * c.BW + 3 + c.LPC + 1, c_A=2 * n_u + 2 * c.BW + 2 + c.LPC + 1,
                c_R=n_c + 2 * c.BW + 3 + c.LPC + 2 * M + 6 + c.GPB,
                c_q=2 * ((M + 1) * (1 + c.D) + 2) + 2 * c.BW + 2 + c.LPC + 1 + 2 * c.K + 4)


def _ratio(err, bound):
    err, bound = float(err), float(bound)
    if not np.isfinite(err):
        return np.inf
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


def chi_forms(c, G, s, th, tha, Z, chi):
    """of ONE curve in longdouble: dict(u, ua, c0, c0a, A, Sa, b, Sb, d, da)"""
    M = chi.shape[0]
    u = np.einsum("k,kmp->mp", Z, th[:, 1:])
    ua = np.einsum("k,kmp->mp", np.abs(Z), tha[:, 1:])
    c0 = Z @ th[:, 0] + chi @ u
    c0a = np.abs(Z) @ tha[:, 0] + np.abs(chi) @ ua
    d = s - S.band_mv(G, c0)
    da = np.abs(s) + S.band_mv(G, c0a, absolute=True)
    Gu = np.stack([S.band_mv(G, u[m]) for m in range(M)]) if M else np.zeros((0, c.P), dtype=LD)
    Gua = np.stack([S.band_mv(G, ua[m], absolute=True) for m in range(M)]) if M else np.zeros((0, c.P), dtype=LD)
    return dict(u=u, ua=ua, c0=c0, c0a=c0a, A=u @ Gu.T, Sa=ua @ Gua.T, b=u @ d, Sb=ua @ da, d=d, da=da)


def check_chi(c, rec, st, chi_new, znorm, beta, X=None, ztol=None):
    """every Gauss-Seidel step of every curve against longdouble, each judged alone (module docstring).  st: the state the update
    started from (Z, chi, nu, Phi, sigma_sq, eta / xi); chi_new (n, M): the device's; znorm (n, M): its normals.  ztol (n, M):
    the absolute allowance of znorm where it is the oracle's keyed normal and not the device's own (an iteration judged from chain
    slots alone; check_chi_norm has the figure): it enters the bound through sqrt(W).
    Returns dict(ok, worst, where (i, m), fails [messages], vacuous (largest bound / |dl|))."""
    M, n = c.M, c.n
    Gb, sv, _ = split_rec(c, rec)
    th, tha = theta_rows(c, st, X, M)
    Z, chi0, chi1, zn = _ld(st["Z"]), _ld(st["chi"]), _ld(chi_new).reshape(n, M), _ld(znorm).reshape(n, M)
    f = LD(beta) / LD(float(np.ravel(st["sigma_sq"])[0]))
    cn = counts(c, M)
    worst, where, fails, vac = 0.0, None, [], 0.0
    for i in range(n):
        fm = chi_forms(c, _ld(Gb[i]), _ld(sv[i]), th[i], tha[i], Z[i], chi0[i])
        dl = chi1[i] - chi0[i]
        for m in range(M):
            A, Sa = fm["A"], fm["Sa"]
            r = fm["b"][m] - sum((A[m2, m] * dl[m2] for m2 in range(m)), LD(0))
            W = 1 / (1 + A[m, m] * f)
            sq = np.sqrt(W)
            ref = W * f * (r + chi0[i, m] * A[m, m]) + sq * zn[i, m]
            E_r = (cn["c_b"] + m + 1) * U * fm["Sb"][m] + sum(((cn["c_A"] + m + 1) * U * Sa[m2, m] * abs(dl[m2]) + U * Sa[m2, m] * abs(chi1[i, m2])
                                                               for m2 in range(m)), LD(0))
            dA = cn["c_A"] * U * Sa[m, m]
            bound = G_CHI * (W * f * E_r + W * f * abs(chi0[i, m]) * dA + abs(f * (r + chi0[i, m] * A[m, m]) + zn[i, m] / (2 * sq)) * W * W * f * dA
                             + 8 * U * (W * f * (abs(r) + abs(chi0[i, m]) * A[m, m]) + abs(chi0[i, m]) + sq * abs(zn[i, m])) + U * abs(ref))
            if ztol is not None:
                bound = bound + sq * LD(float(np.asarray(ztol).reshape(n, M)[i, m]))
            err = abs(chi1[i, m] - ref)
            ratio = _ratio(err, bound)
            step = abs(ref - chi0[i, m])
            vac = max(vac, _ratio(bound, step))
            if ratio > worst:
                worst, where = ratio, (i, m)
            if not ratio <= 1.0:
                fails.append(f"{c.name}: curve {i}, step m {m}: chi {float(chi1[i, m])!r}, reference {float(ref)!r}, error {float(err):.3g}, "
                             f"bound {float(bound):.3g}, error / bound {ratio:.3g} (r_m {float(r):.6g}, A_mm {float(A[m, m]):.6g}, W {float(W):.6g}, "
                             f"z {float(zn[i, m]):.6g}, chi_old {float(chi0[i, m]):.6g})")
    return dict(ok=not fails, worst=worst, where=where, fails=fails, vacuous=vac)


def check_rss(c, rec, st, chi_new, rss_part, X=None, M=None):
    """rss_part[b] against sum_{i in b} (yy - 2 c's + c'Gc) at the final chi (module docstring); M = 0: phi_chi_zero (c = sum_k Z_k nu_k)
    Returns dict(ok, worst, fails, rss (the longdouble total), parts_ref)."""
    M = c.M if M is None else M
    n = c.n
    Gb, sv, yy = split_rec(c, rec)
    th, tha = theta_rows(c, st, X, M)
    Z, chi0, chi1 = _ld(st["Z"]), _ld(st["chi"])[:, :M], _ld(chi_new).reshape(n, -1)[:, :M]
    cn = counts(c, M)
    part, Sabs = np.zeros(c.nblk, dtype=LD), np.zeros(c.nblk, dtype=LD)
    for i in range(n):
        G, s = _ld(Gb[i]), _ld(sv[i])
        fm = chi_forms(c, G, s, th[i], tha[i], Z[i], chi0[i])
        dl = chi1[i] - chi0[i]
        cf = fm["c0"] + dl @ fm["u"]
        ca = fm["c0a"] + np.abs(dl) @ fm["ua"]
        val = LD(yy[i]) - 2 * (cf @ s) + cf @ S.band_mv(G, cf)
        f1 = abs(LD(yy[i])) + 2 * (ca @ np.abs(s)) + ca @ S.band_mv(G, ca, absolute=True)
        f2 = (abs(LD(yy[i])) + fm["c0a"] @ np.abs(s) + fm["c0a"] @ fm["da"]
              + sum((abs(dl[m]) * (2 * fm["Sb"][m] + np.abs(dl) @ fm["Sa"][m]) for m in range(M)), LD(0)))
        part[i // c.GPB] += val
        Sabs[i // c.GPB] += max(f1, f2)
    got = _ld(rss_part).reshape(-1)
    fails, worst = [], 0.0
    if got.shape[0] != c.nblk:
        return dict(ok=False, worst=np.inf, fails=[f"{c.name}: {got.shape[0]} residual partial sums for {c.nblk} curve workgroups"], rss=part.sum(), parts_ref=part)
    for b in range(c.nblk):
        bound = G_RSS * cn["c_R"] * U * Sabs[b]
        ratio = _ratio(abs(got[b] - part[b]), bound)
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            fails.append(f"{c.name}: rss_part[{b}] (curves {b * c.GPB} .. {min(n, (b + 1) * c.GPB) - 1}) {float(got[b])!r}, reference {float(part[b])!r}, "
                         f"error / bound {ratio:.3g} (bound {float(bound):.3g})")
    return dict(ok=not fails, worst=worst, fails=fails, rss=part.sum(), parts_ref=part)


def check_total_and_loglik(c, rss_part, rss, loglik, sigma2, n_obs_total):
    """Dyn::rss against the sum of the parts, and the log-likelihood from that RSS (module docstring): list of failures"""
    parts = _ld(rss_part).reshape(-1)
    fails = []
    bound = (c.nblk + 10) * U * np.abs(parts).sum()
    if not abs(LD(rss) - parts.sum()) <= bound:
        fails.append(f"{c.name}: RSS {rss!r}, the sum of rss_part {float(parts.sum())!r} (bound {float(bound):.3g})")
    s2 = LD(sigma2)
    if c.kind == "mv":
        t1 = -LD(c.n) * ((c.P // 2) * np.log(2 * LD(np.pi) * s2))      # (np.pi rounded: 1e-16 relative, inside the bound)
    else:
        t1 = -LD(n_obs_total) * (LOG_SQRT_2PI + np.log(np.sqrt(s2)))
    t2 = -LD(rss) / (2 * s2)
    ref = t1 + t2
    bound = 8 * U * (abs(t1) + abs(t2))
    if not abs(LD(loglik) - ref) <= bound:
        fails.append(f"{c.name}: log-likelihood {loglik!r}, CalculateLikelihood.h from the device's RSS gives {float(ref)!r} "
                     f"(difference {float(abs(LD(loglik) - ref)):.3g}, bound {float(bound):.3g})")
    return fails


def check_cfull(c, rec, st, chi_new, X, cfull, gfull):
    """covariate models, what k_curve_chi leaves for the eta / Xi steps: c_i = c0 + sum_m dl_m u_m and g_i = G_i c_i at the new chi
    (chi_new = st's chi: the residual-only pass, c_i = c0), entry by entry.  launch_cov_block stores to cfull / gfull only
    behind an eta / Xi step, so after a run whose mask has neither these are k_curve_chi's values.  Bounds, with
    ca = c0a + sum_m |dl_m| ua_m and the counts of the module docstring:
        cfull   G_CF (n_c + M + 1) u ca + sum_m u |chi_new,m| ua_m + u |c_ref|
        gfull   G_GF (n_c + 2 BW + M + 5) u (2 |s| + |G| ca) + sum_m u |chi_new,m| |G| ua_m + u |g_ref|
    (the kernel forms g_i as s - (s - G c0) + sum_m dl_m G u_m: |s| enters twice; the middle terms are the rounding of the
    device's dl against the difference the reference recovers).  Returns dict(ok, worst, worst_g, fails)."""
    n, P, M = c.n, c.P, c.M
    Gb, sv, _ = split_rec(c, rec)
    th, tha = theta_rows(c, st, X, M)
    Z, chi0, chi1 = _ld(st["Z"]), _ld(st["chi"]), _ld(chi_new).reshape(n, M)
    gc, gg = _ld(cfull).reshape(n, P), _ld(gfull).reshape(n, P)
    cn = counts(c, M)
    worst, worst_g, fails = 0.0, 0.0, []
    for i in range(n):
        G, s = _ld(Gb[i]), _ld(sv[i])
        fm = chi_forms(c, G, s, th[i], tha[i], Z[i], chi0[i])
        dl = chi1[i] - chi0[i]
        cref = fm["c0"] + dl @ fm["u"]
        ca = fm["c0a"] + np.abs(dl) @ fm["ua"]
        dle = np.abs(chi1[i]) @ fm["ua"]
        gref = S.band_mv(G, cref)
        bc = G_CF * (cn["n_c"] + M + 1) * U * ca + U * dle + U * np.abs(cref)
        bg = (G_GF * (cn["n_c"] + 2 * c.BW + M + 5) * U * (2 * np.abs(s) + S.band_mv(G, ca, absolute=True))
              + U * S.band_mv(G, dle, absolute=True) + U * np.abs(gref))
        for nm, got, ref, b in (("cfull", gc[i], cref, bc), ("gfull", gg[i], gref, bg)):
            for p in range(P):
                ratio = _ratio(abs(got[p] - ref[p]), b[p])
                if nm == "cfull":
                    worst = max(worst, ratio)
                else:
                    worst_g = max(worst_g, ratio)
                if not ratio <= 1.0:
                    fails.append(f"{c.name}: curve {i}, row p {p}: {nm} {float(got[p])!r}, reference {float(ref[p])!r}, error / bound {ratio:.3g}")
    return dict(ok=not fails, worst=worst, worst_g=worst_g, fails=fails)


def lgamma_ld(x):
    """log Gamma(x), x > 0, in longdouble: upward recurrence to x >= 25, then the Stirling series through x^-13 (the next term is
    below 1e-22 there)"""
    x = LD(x)
    shift = LD(0)
    while x < 25:
        shift += np.log(x)
        x += 1
    r = 1 / x
    r2 = r * r
    ser = r * (LD(1) / 12 - r2 * (LD(1) / 360 - r2 * (LD(1) / 1260 - r2 * (LD(1) / 1680 - r2 * (LD(1) / 1188 - r2 * (LD(691) / 360360 - r2 / 156))))))
    return (x - LD(0.5)) * np.log(x) - x + LOG_SQRT_2PI + ser - shift


def oracle_gammas(c, Z_old, a_Z_PM, chain_id, it, tt=0):
    """the K keyed gamma variates per curve of the Dirichlet proposal (UPD_Z_PROP, index i K + k, shape a_Z_PM Z_old,k, or 10 where
    that is <= 0: Distributions.h:24-28) from the oracle, without touching it: fill(.., idx + 1, ..)[-1] is the variate of index idx"""
    import oracle_lib as O
    Z0 = np.asarray(Z_old, dtype=np.float64).reshape(c.n, c.K)
    g = np.zeros((c.n, c.K))
    for i in range(c.n):
        for k in range(c.K):
            a = a_Z_PM * Z0[i, k]
            g[i, k] = O.fill(2, i * c.K + k + 1, seed=SEED, chain=chain_id, it=it, upd=UPD_Z_PROP, p1=float(10.0 if a <= 0 else a), p2=1.0, tt=tt)[-1]
    return g


def proposal_fields(Z_old, gam, a_Z_PM, dtype=LD, Znew=None):
    """of ONE curve without a zero: Z_new = g / sum g and the proposal densities of UpdateMixedMembership.h:102-113 with calc_lB
    (Distributions.h:40-60), in `dtype` (longdouble: the restatement; float64 with libm's log / lgamma: what the oracle's own
    arithmetic gives).  Znew: evaluate the densities at this Z_new instead (the device's recorded one).
    Returns dict(Znew, lpn, lpo, S_lpn, S_lpo): S_* the sums of absolute terms."""
    from math import lgamma
    T = dtype
    lg = lgamma_ld if T is LD else (lambda v: T(lgamma(float(v))))
    z0, g = np.asarray(Z_old, dtype=np.float64).astype(T), np.asarray(gam, dtype=np.float64).astype(T)
    zn = g / g.sum() if Znew is None else np.asarray(Znew, dtype=np.float64).astype(T)
    ao, an = T(a_Z_PM) * z0, T(a_Z_PM) * zn
    lo, ln = np.log(z0), np.log(zn)
    lgo, lgn = np.array([lg(v) for v in ao], dtype=T), np.array([lg(v) for v in an], dtype=T)
    lso, lsn = lg(ao.sum()), lg(an.sum())
    return dict(Znew=zn, lpn=((ao - 1) * ln).sum() - (lgo.sum() - lso), lpo=((an - 1) * lo).sum() - (lgn.sum() - lsn),
                S_lpn=(np.abs(ao - 1) * np.abs(ln)).sum() + np.abs(lgo).sum() + abs(lso),
                S_lpo=(np.abs(an - 1) * np.abs(lo)).sum() + np.abs(lgn).sum() + abs(lsn))


def measure_proposal(c, q=0, it=0, a_Z_PM=10000.0):
    """the oracle's arithmetic (float64, libm) against the longdouble restatement over the curves of a case, in units of u: the
    largest |Z_new - ref| / Z_new,  |lpn - ref| / S_lpn,  |lpo - ref| / S_lpo"""
    st = case_state(c, q)
    gam = oracle_gammas(c, st["Z"], a_Z_PM, q, it)
    out = dict(Znew=0.0, lpn=0.0, lpo=0.0)
    for i in range(c.n):
        if (st["Z"][i] <= 0).any():
            continue
        r, f = proposal_fields(st["Z"][i], gam[i], a_Z_PM, LD), proposal_fields(st["Z"][i], gam[i], a_Z_PM, np.float64)
        out["Znew"] = max(out["Znew"], float((np.abs(f["Znew"].astype(LD) - r["Znew"]) / r["Znew"]).max() / U))
        for k in ("lpn", "lpo"):
            out[k] = max(out[k], float(abs(LD(f[k]) - r[k]) / r["S_" + k] / U))
    return out


def check_proposal(c, Z_old, zrec, a_Z_PM, chain_id, it, tt=0):
    """the data-independent half of the recorded proposal against the restatement: Z_new against the oracle's keyed gamma
    variates, normalised in longdouble, under PROP_MARGIN MEASURED_PROP["Znew"] u Z_new; lpn and lpo against the longdouble
    densities AT the recorded Z_new under PROP_MARGIN MEASURED_PROP[.] u S (the sums of absolute terms).  A curve with a zero only
    has its Z_new checked (its densities are infinite and unused).  Returns dict(fails, worst: {field: error / tolerance})."""
    zr = split_zrec(c, zrec)
    Z0 = np.asarray(Z_old, dtype=np.float64).reshape(c.n, c.K)
    gam = oracle_gammas(c, Z0, a_Z_PM, chain_id, it, tt)
    fails, worst = [], dict(Znew=0.0, lpn=0.0, lpo=0.0)
    for i in range(c.n):
        g = gam[i].astype(LD)
        ref = g / g.sum()
        tol = PROP_MARGIN * MEASURED_PROP["Znew"] * U * ref
        rz = float((np.abs(_ld(zr["Znew"][i]) - ref) / tol).max())
        worst["Znew"] = max(worst["Znew"], rz)
        if not rz <= 1.0:
            fails.append(f"{c.name}: curve {i}: Z_new {zr['Znew'][i]} against the oracle's keyed gamma variates normalised "
                         f"{np.asarray(ref, dtype=np.float64)}: error / tolerance {rz:.3g} (iteration {it}, chain id {chain_id})")
        if (Z0[i] <= 0).any():
            continue
        r = proposal_fields(Z0[i], gam[i], a_Z_PM, LD, Znew=zr["Znew"][i])
        for k in ("lpn", "lpo"):
            ratio = _ratio(abs(LD(zr[k][i]) - r[k]), PROP_MARGIN * MEASURED_PROP[k] * U * r["S_" + k])
            worst[k] = max(worst[k], ratio)
            if not ratio <= 1.0:
                fails.append(f"{c.name}: curve {i}: {k} {zr[k][i]!r}, restated {float(r[k])!r}: error / tolerance {ratio:.3g}")
    return dict(fails=fails, worst=worst)


def reference_z(c, rec, st, beta, a_Z_PM, chain_id, it, X=None, tt=0):
    """the whole Z update in longdouble from the oracle's keyed variates (gamma: UPD_Z_PROP, uniform: UPD_Z_ACC): Z_out (n, K) float64
    and the acceptance values"""
    import oracle_lib as O
    n, K, M = c.n, c.K, c.M
    Gb, sv, yy = split_rec(c, rec)
    th, tha = theta_rows(c, st, X, M)
    chi, Z0 = _ld(st["chi"]), np.asarray(st["Z"], dtype=np.float64)
    gam = oracle_gammas(c, Z0, a_Z_PM, chain_id, it, tt)
    luu = np.log(O.fill(0, n, seed=SEED, chain=chain_id, it=it, upd=UPD_Z_ACC, tt=tt).astype(LD))
    coef = LD(float(np.ravel(st["alpha_3"])[0])) * _ld(np.ravel(st["pi"])) - 1
    f2 = LD(beta) / (2 * LD(float(np.ravel(st["sigma_sq"])[0])))
    Z1, acc = Z0.copy(), np.zeros(n)
    for i in range(n):
        r = proposal_fields(Z0[i], gam[i], a_Z_PM, LD)
        fm = z_forms(c, _ld(Gb[i]), _ld(sv[i]), th[i], tha[i], chi[i])
        zo, zn = _ld(Z0[i]), r["Znew"]
        a = ((coef * np.log(zn)).sum() - (coef * np.log(zo)).sum() + r["lpo"] - r["lpn"]) - f2 * (_q(zn, fm["a"], fm["Q"]) - _q(zo, fm["a"], fm["Q"]))
        if (Z0[i] <= 0).any():
            a = LD(1)
        acc[i] = float(a)
        if luu[i] < a:
            Z1[i] = np.asarray(zn, dtype=np.float64)
    return Z1, acc


def _cov_rows(c, st, X, M, dtype=LD):
    """e[i, k, mt, p] = sum_d x_id thetaX_{(k, mt), d}[p] and its sum of absolute terms"""
    tx = np.zeros((c.K, M + 1, c.D, c.P), dtype=dtype)
    tx[:, 0] = np.transpose(np.asarray(st["eta"], dtype=np.float64), (2, 1, 0)).astype(dtype)
    for m in range(M):
        tx[:, m + 1] = np.transpose(np.asarray(st["xi"], dtype=np.float64)[:, :, m, :], (2, 1, 0)).astype(dtype)
    Xl = np.asarray(X, dtype=np.float64).astype(dtype)
    return np.einsum("id,kmdp->ikmp", Xl, tx), np.einsum("id,kmdp->ikmp", np.abs(Xl), np.abs(tx))


def check_stil(c, rec, st, Z_out, X, stil, yyp_part):
    """covariate models, what k_curve_z leaves for the Phi / nu block: o_i = sum_k Z_out,k ucov_k with ucov_k the covariate part of
    u_k (sum_d x_d (eta_{k,d} + sum_m chi_m xi_{k,m,d})), stil_i = s_i - G_i o_i entry by entry under
        G_STIL (c_o + 2 BW + 3) u (|s| + |G| oa) + u |stil_ref|,      c_o = D + M + 1 + K + 3
    (a term x_d chi_m Z_k xi passes D + (M + 1) + K additions and three products, then the band product and the subtraction),
    and yyp_part[b] = sum_{i in b} (yy - 2 o's + o'Go) under G_YYP (2 c_o + 2 BW + 2 + P + 4 + GPB) u sum_i (|yy| + 2 oa'|s| + oa'|G|oa).
    st: the state the update saw (chi, eta, xi); Z_out: the Z it left.  Returns dict(ok, worst, worst_yyp, fails)."""
    n, P, M = c.n, c.P, c.M
    Gb, sv, yy = split_rec(c, rec)
    e, ea = _cov_rows(c, st, X, M)
    chi, Z1 = _ld(st["chi"]), _ld(Z_out).reshape(n, c.K)
    got = _ld(stil).reshape(n, P)
    c_o = c.D + M + 1 + c.K + 3
    part, Sabs = np.zeros(c.nblk, dtype=LD), np.zeros(c.nblk, dtype=LD)
    worst, fails = 0.0, []
    for i in range(n):
        G, s = _ld(Gb[i]), _ld(sv[i])
        uc = e[i][:, 0] + np.einsum("m,kmp->kp", chi[i], e[i][:, 1:])
        uca = ea[i][:, 0] + np.einsum("m,kmp->kp", np.abs(chi[i]), ea[i][:, 1:])
        o, oa = Z1[i] @ uc, np.abs(Z1[i]) @ uca
        Go, Goa = S.band_mv(G, o), S.band_mv(G, oa, absolute=True)
        ref = s - Go
        bound = G_STIL * (c_o + 2 * c.BW + 3) * U * (np.abs(s) + Goa) + U * np.abs(ref)
        err = np.abs(got[i] - ref)
        for p in range(P):
            ratio = _ratio(err[p], bound[p])
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                fails.append(f"{c.name}: curve {i}, row p {p}: stil {float(got[i, p])!r}, reference {float(ref[p])!r}, error / bound {ratio:.3g}")
        part[i // c.GPB] += LD(yy[i]) - 2 * (o @ s) + o @ Go
        Sabs[i // c.GPB] += abs(LD(yy[i])) + 2 * (oa @ np.abs(s)) + oa @ Goa
    gy = _ld(yyp_part).reshape(-1)
    wy = 0.0
    for b in range(c.nblk):
        bound = G_YYP * (2 * c_o + 2 * c.BW + 2 + P + 4 + c.GPB) * U * Sabs[b]
        ratio = _ratio(abs(gy[b] - part[b]), bound)
        wy = max(wy, ratio)
        if not ratio <= 1.0:
            fails.append(f"{c.name}: yyp_part[{b}] {float(gy[b])!r}, reference {float(part[b])!r}, error / bound {ratio:.3g}")
    return dict(ok=not fails, worst=worst, worst_yyp=wy, fails=fails)


def emulate_stil(c, rec, st, Z_out, X, variant="kernel", mut=None):
    """k_curve_z's covariate offsets in float64: (stil (n, P), yyp_part (nblk))"""
    n, K, P, M, D = c.n, c.K, c.P, c.M, c.D
    Gb, sv, yy = split_rec(c, rec)
    chi, Z1, Xd = np.asarray(st["chi"], dtype=np.float64), np.asarray(Z_out, dtype=np.float64), np.asarray(X, dtype=np.float64)
    eta, xi = np.asarray(st["eta"], dtype=np.float64), np.asarray(st["xi"], dtype=np.float64)
    if variant == "plain":
        e, _ = _cov_rows(c, st, X, M, np.float64)
        uc = e[:, :, 0] + np.einsum("im,ikmp->ikp", chi, e[:, :, 1:])
        o = np.einsum("ik,ikp->ip", Z1, uc)
        Go = np.stack([np.asarray(S.band_mv(Gb[i], o[i]), dtype=np.float64) for i in range(n)])
        yyp = yy - 2.0 * np.einsum("ip,ip->i", o, sv) + np.einsum("ip,ip->i", o, Go)
    else:
        uc = np.zeros((n, K, P))
        for d in range(D):
            uc = uc + Xd[:, d][:, None, None] * eta[:, d, :].T[None]
        sch = np.concatenate([chi, np.zeros((n, 1))], axis=1)
        for m in range(0, M if mut != "cov_left_out" else 0, 2):      # mutation: the chi-weighted covariate part never enters o_i
            e0, e1 = np.zeros((n, K, P)), np.zeros((n, K, P))
            for d in range(D):
                e0 = e0 + Xd[:, d][:, None, None] * xi[:, d, m, :].T[None]
                e1 = e1 + Xd[:, d][:, None, None] * xi[:, d, min(m + 1, M - 1), :].T[None]
            uc = uc + (sch[:, m][:, None, None] * e0 + sch[:, m + 1][:, None, None] * e1)
        o = np.zeros((n, P))
        for k in range(K):
            o = o + Z1[:, k][:, None] * uc[:, k]
        Go = _matvec64(Gb, o)
        d1, d2 = np.zeros(n), np.zeros(n)
        for p in range(P):
            d1, d2 = d1 + o[:, p] * sv[:, p], d2 + o[:, p] * Go[:, p]
        yyp = yy - 2.0 * d1 + d2
    part = np.zeros(c.nblk)
    for i in range(n):
        part[i // c.GPB] = part[i // c.GPB] + yyp[i]
    return sv - Go, part


ZREC_FIELDS = ("acceptance", "log_uu", "pr_old", "pr_new", "lpo", "lpn")


def split_zrec(c, zrec):
    z = np.asarray(zrec, dtype=np.float64).reshape(6 + c.K, c.n)
    out = {k: z[j] for j, k in enumerate(ZREC_FIELDS)}
    out["Znew"] = z[6:].T.copy()
    return out


def z_forms(c, G, s, th, tha, chi):
    """of ONE curve in longdouble: a (K), Q (K, K) and their sums of absolute terms"""
    u = th[:, 0] + np.einsum("m,kmp->kp", chi, th[:, 1:])
    ua = tha[:, 0] + np.einsum("m,kmp->kp", np.abs(chi), tha[:, 1:])
    Gu = np.stack([S.band_mv(G, u[k]) for k in range(c.K)])
    Gua = np.stack([S.band_mv(G, ua[k], absolute=True) for k in range(c.K)])
    return dict(a=u @ s, aa=ua @ np.abs(s), Q=u @ Gu.T, Qa=ua @ Gua.T)


def _q(Z, a, Q):
    return Z @ (-2 * a + Q @ Z)


def check_z(c, rec, st, zrec, Z_out, beta, X=None, M=None, logz_part=None):
    """the recorded acceptance of every curve against longdouble, the decision and the outputs (module docstring).  st: the state
    the update started from (chi: the values the update SAW); zrec: "z_record"; Z_out (n, K): the Z after the update.
    Returns dict(ok, worst, where, fails, vacuous, accepted (count), forced (curves with a zero))."""
    M = c.M if M is None else M
    n, K = c.n, c.K
    Gb, sv, yy = split_rec(c, rec)
    th, tha = theta_rows(c, st, X, M)
    chi = _ld(st["chi"])[:, :M]
    Z0 = np.asarray(st["Z"], dtype=np.float64)
    Z1 = np.asarray(Z_out, dtype=np.float64).reshape(n, K)
    zr = split_zrec(c, zrec)
    f2 = LD(beta) / (2 * LD(float(np.ravel(st["sigma_sq"])[0])))
    cn = counts(c, M)
    worst, where, fails, vac, nacc, forced = 0.0, None, [], 0.0, 0, 0
    for i in range(n):
        acc, luu, Zn = zr["acceptance"][i], zr["log_uu"][i], zr["Znew"][i]
        took = bool(luu < acc)
        nacc += took
        want = Zn if took else Z0[i]
        if not np.array_equal(Z1[i].view(np.uint64), want.view(np.uint64)):
            fails.append(f"{c.name}: curve {i}: log_uu {luu!r} {'<' if took else '>='} acceptance {acc!r} but Z_out {Z1[i]} is not "
                         f"{'the recorded proposal' if took else 'Z_old'} {want}")
        if (Z0[i] <= 0).any():
            forced += 1
            if acc != 1.0 or not took:
                fails.append(f"{c.name}: curve {i} has a Z_old,k = 0: acceptance {acc!r} (must be exactly 1), proposal taken: {took}")
            continue
        fm = z_forms(c, _ld(Gb[i]), _ld(sv[i]), th[i], tha[i], chi[i])
        zo, zn = _ld(Z0[i]), _ld(Zn)
        qo, qn = _q(zo, fm["a"], fm["Q"]), _q(zn, fm["a"], fm["Q"])
        Sq = sum((abs(LD(yy[i])) + np.abs(z) @ (2 * fm["aa"] + fm["Qa"] @ np.abs(z)) for z in (zo, zn)), LD(0))
        pn, po, lpo, lpn = (LD(zr[k][i]) for k in ("pr_new", "pr_old", "lpo", "lpn"))
        prop = pn - po + lpo - lpn
        lik = f2 * (qn - qo)
        ref = prop - lik
        bound = G_ACC * (f2 * cn["c_q"] * U * Sq + 4 * U * (abs(pn) + abs(po) + abs(lpo) + abs(lpn) + abs(ref)))
        err = abs(LD(acc) - ref)
        ratio = _ratio(err, bound)
        vac = max(vac, _ratio(bound, abs(lik)))
        if ratio > worst:
            worst, where = ratio, i
        if not ratio <= 1.0:
            k, k2 = np.unravel_index(int(np.argmax(np.abs(np.outer(zn, zn) - np.outer(zo, zo)) * np.abs(fm["Q"]))), (K, K))
            fails.append(f"{c.name}: curve {i}: acceptance {acc!r}, reference {float(ref)!r} = proposal part {float(prop)!r} (pr_new {float(pn)!r} - pr_old "
                         f"{float(po)!r} + lpo {float(lpo)!r} - lpn {float(lpn)!r}) - likelihood part {float(lik)!r} (beta / 2 sigma^2 {float(f2):.6g}, q_new "
                         f"{float(qn)!r}, q_old {float(qo)!r}); error {float(err):.3g}, bound {float(bound):.3g}, error / bound {ratio:.3g}; the largest "
                         f"form of the difference is (k, k2) = ({k}, {k2}), Q {float(fm['Q'][k, k2])!r}")
    if logz_part is not None:
        fails += check_logz(c, Z1, logz_part)
    return dict(ok=not fails, worst=worst, where=where, fails=fails, vacuous=vac, accepted=nacc, forced=forced)


def check_logz(c, Z_out, logz_part):
    """logz_part[b, k] against sum_{i in b} log Z_out,ik"""
    lz = np.log(_ld(Z_out).reshape(c.n, c.K))
    got = _ld(logz_part).reshape(-1)
    if got.shape[0] != c.nblk * c.K:
        return [f"{c.name}: {got.shape[0]} partial sums of log Z for {c.nblk} x {c.K}"]
    fails = []
    for b in range(c.nblk):
        blk = lz[b * c.GPB:(b + 1) * c.GPB]
        ref, bound = blk.sum(axis=0), (c.GPB + 4) * U * np.abs(blk).sum(axis=0)
        for k in range(c.K):
            if not abs(got[b * c.K + k] - ref[k]) <= bound[k]:
                fails.append(f"{c.name}: logz_part[{b}, {k}] {float(got[b * c.K + k])!r}, reference {float(ref[k])!r} (bound {float(bound[k]):.3g})")
    return fails


def check_prior_terms(c, Z_old, zrec, pi, alpha3):
    """the recorded pr_old = sum_k (alpha_3 pi_k - 1) log Z_old,k and pr_new (the same at the recorded Z_new) against longdouble,
    with the pi and alpha_3 the update must use (a fused or lean update of iteration t + 1: those of chain slot t).  Bound
    (K + 5) u sum_k |alpha_3 pi_k - 1| |log Z_k|: a log of at most 2 ulp, the two products and the difference of each coefficient, K
    additions.  A stale pi or alpha_3 (the previous iteration's) moves the terms by the size of the pi / alpha_3 step."""
    zr = split_zrec(c, zrec)
    coef = LD(float(np.ravel(alpha3)[0])) * _ld(np.ravel(pi)) - 1
    Z0 = np.asarray(Z_old, dtype=np.float64).reshape(c.n, c.K)
    fails = []
    for i in range(c.n):
        if (Z0[i] <= 0).any():
            continue
        for nm, Zv in (("pr_old", Z0[i]), ("pr_new", zr["Znew"][i])):
            l = np.log(_ld(Zv))
            ref, bound = (coef * l).sum(), (c.K + 5) * U * (np.abs(coef) * np.abs(l)).sum()
            if not abs(LD(zr[nm][i]) - ref) <= bound:
                fails.append(f"{c.name}: curve {i}: {nm} {zr[nm][i]!r}, sum_k (alpha_3 pi_k - 1) log Z_k gives {float(ref)!r} "
                             f"(difference {float(abs(LD(zr[nm][i]) - ref)):.3g}, bound {float(bound):.3g})")
    return fails


def check_log_uu(c, zrec, chain_id, it, tt=0):
    """the recorded log_uu against the log of the oracle's keyed uniform (UPD_Z_ACC, index i)"""
    import oracle_lib as O
    uu = O.fill(0, c.n, seed=SEED, chain=chain_id, it=it, upd=UPD_Z_ACC, tt=tt)
    ref = np.log(uu.astype(LD))
    got = split_zrec(c, zrec)["log_uu"]
    bad = [i for i in range(c.n) if not abs(LD(got[i]) - ref[i]) <= 4 * U * abs(ref[i]) + 2 * U]
    return [f"{c.name}: log_uu of curves {bad} differs from log(runif(UPD_Z_ACC, i)) of iteration {it}: {got[bad]} against {np.asarray(ref[bad], dtype=np.float64)}"] if bad else []


def check_chi_norm(c, znorm, chain_id, it, tt=0):
    """chi_norm against the oracle's keyed rnorm (UPD_CHI, index i M + m).  Both are AS241 (PPND16) of the same uniform: a ratio
    of two degree-7 polynomials, each Horner step one rounding (16 u relative at most on the ratio, usually 3), and in the tails
    r = sqrt(-log(min(p, 1 - p))) through two libm paths of <= 2 ulp each, which the polynomials (condition below 4 in r) carry
    to <= 16 u: 32 u |z| + 4 u (q = p - 1/2 near zero: absolute)."""
    import oracle_lib as O
    ref = O.fill(1, c.n * c.M, seed=SEED, chain=chain_id, it=it, upd=UPD_CHI, tt=tt).reshape(c.n, c.M)
    got = np.asarray(znorm, dtype=np.float64).reshape(c.M, c.n).T      # the device holds it curve-fastest
    bad = np.argwhere(~(np.abs(got - ref) <= 32 * U * np.abs(ref) + 4 * U))
    return [f"{c.name}: chi_norm differs from rnorm(UPD_CHI, i M + m) of iteration {it} at (i, m) {bad[:4].tolist()}: {got[tuple(bad[0])]!r} against {ref[tuple(bad[0])]!r}"] if len(bad) else []


def reference_chi(c, rec, st, znorm, beta, X=None):
    """the whole chi update in longdouble, every step from the reference's own earlier steps: chi_new (n, M) longdouble"""
    M, n = c.M, c.n
    Gb, sv, _ = split_rec(c, rec)
    th, tha = theta_rows(c, st, X, M)
    Z, chi0, zn = _ld(st["Z"]), _ld(st["chi"]), _ld(znorm).reshape(n, M)
    f = LD(beta) / LD(float(np.ravel(st["sigma_sq"])[0]))
    out = chi0.copy()
    for i in range(n):
        fm = chi_forms(c, _ld(Gb[i]), _ld(sv[i]), th[i], tha[i], Z[i], chi0[i])
        dl = np.zeros(M, dtype=LD)
        for m in range(M):
            r = fm["b"][m] - sum((fm["A"][m2, m] * dl[m2] for m2 in range(m)), LD(0))
            W = 1 / (1 + fm["A"][m, m] * f)
            out[i, m] = W * f * (r + chi0[i, m] * fm["A"][m, m]) + np.sqrt(W) * zn[i, m]
            dl[m] = out[i, m] - chi0[i, m]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulations
# ---------------------------------------------------------------------------------------------------------------------
CHI_MUTATIONS = ("stale_dl", "small_at_9", "sqrtW_as_W", "rss_no_cross", "idle_rss")
COV_MUTATIONS = ("cov_left_out", "cfull_last_step")
Z_MUTATIONS = ("q_transposed", "half_dot_dropped", "a_vs_resid", "no_beta", "lp_swapped", "inv_s2", "pad_nonzero")


def _rows64(c, st, X, M):
    """theta rows in the kernel's order: e = theta + x_0 thetaX_0 + x_1 thetaX_1 + ..., float64: (n, K, M + 1, LPC), zero beyond P"""
    K, P, n, L = c.K, c.P, c.n, c.LPC
    th = np.zeros((n, K, M + 1, L))
    th[:, :, 0, :P] = np.asarray(st["nu"], dtype=np.float64)
    for m in range(M):
        th[:, :, m + 1, :P] = np.asarray(st["Phi"], dtype=np.float64)[:, :, m]
    if c.D:
        eta, xi = np.asarray(st["eta"], dtype=np.float64), np.asarray(st["xi"], dtype=np.float64)
        for d in range(c.D):
            x = np.asarray(X, dtype=np.float64)[:, d][:, None, None]
            th[:, :, 0, :P] = th[:, :, 0, :P] + x * eta[:, d, :].T[None]
            for m in range(M):
                th[:, :, m + 1, :P] = th[:, :, m + 1, :P] + x * xi[:, d, m, :].T[None]
    return th


def _matvec64(Gb, v):
    """Curve::matvec: g[0] v[p], then for d = 1 .. BW: + g[d] v[p + d] + gl[d] v[p - d]; Gb (n, BW + 1, P), v (n, ..., L)"""
    n, nb, P = Gb.shape
    L = v.shape[-1]
    g = np.zeros((n, nb, L))
    g[:, :, :P] = Gb
    ex = (slice(None),) + (None,) * (v.ndim - 2)
    out = g[:, 0][ex] * v
    for d in range(1, min(nb - 1, P - 1) + 1):
        up, lo = np.zeros_like(v), np.zeros_like(v)
        up[..., :L - d] = g[:, d][ex][..., :L - d] * v[..., d:]
        lo[..., d:] = g[:, d][ex][..., :L - d] * v[..., :L - d]
        out = out + (up + lo)
    return out


def _dot4(a, b, lo=0, hi=None):
    """dot_lds: four accumulators over the entries lo .. hi of the last axis, (s0 + s1) + (s2 + s3)"""
    hi = a.shape[-1] if hi is None else hi
    acc = [np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape) for _ in range(4)]
    for e in range(lo, hi):
        acc[(e - lo) & 3] = acc[(e - lo) & 3] + a[..., e] * b[..., e]
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def _butterfly(v, width):
    """xor butterfly over the last axis (length `width`, a power of two): every lane's sum, lane 0 returned"""
    x = np.asarray(v, dtype=np.float64).copy()
    lanes = np.arange(width)
    o = 1
    while o < width:
        x = x + x[..., lanes ^ o]
        o *= 2
    return x[..., 0]


def emulate_chi(c, rec, st, znorm, beta, X=None, variant="kernel", mut=None, full=False):
    """k_curve_chi's update in float64: (chi_new (n, M), rss_part (nblk)); full: also (cfull, gfull) (n, P) each"""
    M, n, K, P, L = c.M, c.n, c.K, c.P, c.LPC
    Gb, sv, yy = split_rec(c, rec)
    Z, chi0, zn = np.asarray(st["Z"], dtype=np.float64), np.asarray(st["chi"], dtype=np.float64), np.asarray(znorm, dtype=np.float64).reshape(n, M)
    s2 = float(np.ravel(st["sigma_sq"])[0])
    s = np.zeros((n, L))
    s[:, :P] = sv
    th = _rows64(c, st, X, M)
    if variant == "plain":
        u = np.einsum("ik,ikmp->imp", Z, th[:, :, 1:])
        c0 = np.einsum("ik,ikp->ip", Z, th[:, :, 0]) + np.einsum("im,imp->ip", chi0, u)
        Gd = np.zeros((n, L, L))
        for t in range(min(c.BW, P - 1) + 1):
            for p in range(P - t):
                Gd[:, p, p + t] = Gd[:, p + t, p] = Gb[:, t, p]
        A = np.einsum("imp,ipq,ilq->iml", u, Gd, u)
        b = np.einsum("imp,ip->im", u, s - np.einsum("ipq,iq->ip", Gd, c0))
        f = beta / s2
        chi1 = chi0.copy()
        for m in range(M):
            r = b[:, m] - np.einsum("il,il->i", A[:, :m, m], chi1[:, :m] - chi0[:, :m])
            W = 1.0 / (1.0 + f * A[:, m, m])
            chi1[:, m] = W * (f * (r + chi0[:, m] * A[:, m, m])) + np.sqrt(W) * zn[:, m]
        cf = np.einsum("ik,ikp->ip", Z, th[:, :, 0]) + np.einsum("im,imp->ip", chi1, u)
        rss = yy - 2.0 * np.einsum("ip,ip->i", cf, s) + np.einsum("ip,ipq,iq->i", cf, Gd, cf)
        part = np.array([rss[b0 * c.GPB:(b0 + 1) * c.GPB].sum() for b0 in range(c.nblk)])
        return (chi1, part, cf[:, :P], np.einsum("ipq,iq->ip", Gd, cf)[:, :P]) if full else (chi1, part)

    def zrow(mt):
        v = np.zeros((n, L))
        for k in range(K):
            v = v + Z[:, k][:, None] * th[:, k, mt]
        return v
    cf = zrow(0)
    u = np.zeros((n, M, L))
    for m in range(M):
        u[:, m] = zrow(m + 1)
        cf = cf + chi0[:, m][:, None] * u[:, m]
    c0s = _butterfly(cf * s, L)
    d = s - _matvec64(Gb, cf)
    Gu = _matvec64(Gb, u)
    A = np.zeros((n, M, M))
    for a in range(M):
        for b2 in range(a, M):
            A[:, a, b2] = A[:, b2, a] = _dot4(u[:, a], Gu[:, b2])
    b = np.stack([_dot4(u[:, m], d) for m in range(M)], axis=1)
    rss = yy - c0s - _dot4(cf, d)
    inv_s2 = 1.0 / s2
    col = A.copy()                                         # col[:, m2, ml] = A_{m2, ml}
    if mut == "small_at_9":                                # the SMALL bound (MT = 8) applied past it: column entries and steps m >= 8 are gone
        col[:, 8:, :] = 0.0
    W0 = np.stack([A[:, m, m] for m in range(M)], axis=1)
    den = 1.0 + (W0 * beta) * inv_s2
    Wl, sq = 1.0 / den, 1.0 / np.sqrt(den)
    if mut == "sqrtW_as_W":
        sq = Wl
    c1 = Wl * (beta * inv_s2)
    c3 = (c1 * chi0) * W0 + (sq * zn - chi0)
    r = b.copy()
    dl = np.zeros((n, M))
    for m in range(M if mut != "small_at_9" else min(M, 8)):
        dl[:, m] = c1[:, m] * r[:, m] + c3[:, m]
        use = dl[:, m - 1] if (mut == "stale_dl" and m >= 1) else dl[:, m]      # the lanes behind m read last step's broadcast
        r = r - col[:, m, :] * use[:, None]
    chi1 = chi0 + dl
    tm = -2.0 * b
    for m2 in range(M):
        if mut == "rss_no_cross":
            tm[:, m2] = tm[:, m2] + dl[:, m2] * col[:, m2, m2]
        else:
            tm = tm + dl[:, m2][:, None] * col[:, m2, :]
    lane = np.zeros((n, 16))
    lane[:, :M] = dl * tm
    rss = rss + _butterfly(lane, 16)
    part = np.zeros(c.nblk)
    for g in range(c.nblk * c.GPB):                        # sRss[grp] in group order; an idle group holds 0
        if g < n:
            part[g // c.GPB] = part[g // c.GPB] + rss[g]
        elif mut == "idle_rss":                            # the clamped curve n - 1 counted again
            part[g // c.GPB] = part[g // c.GPB] + rss[n - 1]
    if not full:
        return chi1, part
    cfin, gfin = cf.copy(), s - d                          # the eta / Xi steps start from c_i and g_i = G_i c_i at the NEW chi
    for m in range(M - 1 if mut == "cfull_last_step" else M):      # mutation: the last step's dl never reaches c_i, g_i
        cfin, gfin = cfin + dl[:, m][:, None] * u[:, m], gfin + dl[:, m][:, None] * Gu[:, m]
    return chi1, part, cfin[:, :P], gfin[:, :P]


def synthetic_proposal(c, st, a_Z_PM=10000.0, alpha3=None, pi=None, q=0):
    """a Dirichlet(a Z_old) proposal per curve with the densities and prior terms of UpdateMixedMembership.h in float64 and a
    log-uniform: the fields of "z_record" but the acceptance (CPU tests: the data-dependent half is what is emulated)"""
    from math import lgamma
    rng = np.random.default_rng(zlib.crc32(("prop" + c.name).encode()) + q)
    Z0 = np.asarray(st["Z"], dtype=np.float64)
    n, K = c.n, c.K
    pi = np.asarray(st["pi"], dtype=np.float64) if pi is None else pi
    a3 = float(np.ravel(st["alpha_3"])[0]) if alpha3 is None else alpha3
    out = {k: np.zeros(n) for k in ZREC_FIELDS}
    out["Znew"] = np.zeros((n, K))
    for i in range(n):
        ao = a_Z_PM * Z0[i]
        g = rng.gamma(np.where(ao <= 0, 10.0, ao))
        zn = g / g.sum()
        out["Znew"][i] = zn
        out["log_uu"][i] = np.log(rng.uniform())
        if (Z0[i] <= 0).any():
            out["pr_old"][i], out["lpo"][i] = -np.inf, -np.inf
            continue
        an = a_Z_PM * zn
        lo, ln = np.log(Z0[i]), np.log(zn)
        out["pr_old"][i], out["pr_new"][i] = ((a3 * pi - 1.0) * lo).sum(), ((a3 * pi - 1.0) * ln).sum()
        out["lpn"][i] = ((ao - 1.0) * ln).sum() - (sum(lgamma(x) for x in ao) - lgamma(ao.sum()))
        out["lpo"][i] = ((an - 1.0) * lo).sum() - (sum(lgamma(x) for x in an) - lgamma(an.sum()))
    return out


def pack_zrec(c, prop, acceptance):
    z = np.zeros((6 + c.K, c.n))
    for j, k in enumerate(ZREC_FIELDS):
        z[j] = acceptance if k == "acceptance" else prop[k]
    z[6:] = prop["Znew"].T
    return z


def emulate_z(c, rec, st, prop, beta, X=None, M=None, variant="kernel", mut=None):
    """the data-dependent half of the Z update in float64: (acceptance (n), Z_out (n, K), logz_part (nblk K))"""
    M = c.M if M is None else M
    n, K, P, L = c.n, c.K, c.P, c.LPC
    Gb, sv, yy = split_rec(c, rec)
    Z0, chi = np.asarray(st["Z"], dtype=np.float64), np.asarray(st["chi"], dtype=np.float64)[:, :M]
    Zn = prop["Znew"]
    s2 = float(np.ravel(st["sigma_sq"])[0])
    s = np.zeros((n, L))
    s[:, :P] = sv
    th = _rows64(c, st, X, M)
    if variant == "plain":
        u = th[:, :, 0] + np.einsum("im,ikmp->ikp", chi, th[:, :, 1:])
        Gd = np.zeros((n, L, L))
        for t in range(min(c.BW, P - 1) + 1):
            for p in range(P - t):
                Gd[:, p, p + t] = Gd[:, p + t, p] = Gb[:, t, p]
        a = np.einsum("ikp,ip->ik", u, s)
        Q = np.einsum("ikp,ipq,ilq->ikl", u, Gd, u)
        qo = np.einsum("ik,ikl,il->i", Z0, Q, Z0) - 2.0 * np.einsum("ik,ik->i", Z0, a)
        qn = np.einsum("ik,ikl,il->i", Zn, Q, Zn) - 2.0 * np.einsum("ik,ik->i", Zn, a)
        with np.errstate(invalid="ignore"):      # (a curve with a zero has infinite proposal terms: its acceptance is forced below)
            acc = (prop["pr_new"] - prop["pr_old"]) + (prop["lpo"] - prop["lpn"]) - (beta / (2.0 * s2)) * (qn - qo)
    else:
        pad = 1.0 if mut == "pad_nonzero" else 0.0         # sChi[M]: the pad of the 2-unrolled loop
        sch = np.concatenate([chi, np.full((n, 1), pad)], axis=1)
        u = th[:, :, 0].copy()
        for m in range(0, M, 2):
            r0, r1 = m + 1, min(m + 2, M)
            u = u + (sch[:, m][:, None, None] * th[:, :, r0] + sch[:, m + 1][:, None, None] * th[:, :, r1])
        Gu = _matvec64(Gb, u)
        rhs = s
        if mut == "a_vs_resid":                            # a_k against s - G c0, the row the chi part leaves behind
            c0 = np.einsum("ik,ikp->ip", Z0, u)
            rhs = s - _matvec64(Gb, c0)
        ntask = K + K * (K + 1) // 2
        two = 2 * ntask <= L

        def form(x, y, drop=False):
            if two:
                lo = _dot4(x, y, 0, L // 2)
                return lo if drop else lo + _dot4(x, y, L // 2, L)
            return _dot4(x, y)
        a = np.stack([form(u[:, k], rhs) for k in range(K)], axis=1)
        tri = np.zeros((n, K * (K + 1) // 2))
        for k in range(K):
            for k2 in range(k, K):
                tri[:, F.tri(K, k, k2)] = form(u[:, k], Gu[:, k2], drop=(mut == "half_dot_dropped" and (k, k2) == (0, K - 1)))

        def Qat(k, k2):
            lo, hi = min(k, k2), max(k, k2)
            if mut == "q_transposed" and (k, k2) == (K - 1, 0):      # tri_index(K, a, b) with a > b: another entry of the triangle
                return tri[:, min(k * K - k * (k - 1) // 2 + (k2 - k), tri.shape[1] - 1)]
            return tri[:, F.tri(K, lo, hi)]
        qo, qn = np.zeros(n), np.zeros(n)
        for k in range(K):
            to, tn = -2.0 * a[:, k], -2.0 * a[:, k]
            for k2 in range(K):
                qq = Qat(k, k2)
                to, tn = to + Z0[:, k2] * qq, tn + Zn[:, k2] * qq
            qo, qn = qo + Z0[:, k] * to, qn + Zn[:, k] * tn
        q_old, q_new = yy + qo, yy + qn
        inv = 1.0 / s2 if mut == "inv_s2" else 1.0 / (2.0 * s2)
        bt = 1.0 if mut == "no_beta" else beta
        lpo, lpn = (prop["lpn"], prop["lpo"]) if mut == "lp_swapped" else (prop["lpo"], prop["lpn"])
        with np.errstate(invalid="ignore"):
            acc = (prop["pr_new"] - bt * (q_new * inv)) - (prop["pr_old"] - bt * (q_old * inv)) + lpo - lpn
    acc = np.where((Z0 <= 0).any(axis=1), 1.0, acc)
    took = prop["log_uu"] < acc
    Z1 = np.where(took[:, None], Zn, Z0)
    lz = np.log(Z1)
    logz = np.zeros((c.nblk, K))
    for i in range(n):
        logz[i // c.GPB] = logz[i // c.GPB] + lz[i]
    return acc, Z1, logz.ravel()
