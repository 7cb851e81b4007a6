"""High-precision restatement of the Gauss-Seidel sweep (csrc/kernels_sweep.hip: k_sweep, k_sweep_diag, k_sweep_chain), its
per-step check, its bounds, two float64 emulations of the kernels' orders of operations and the case list shared by
tests/test_sweep_ref.py (CPU) and tests/test_gpu_sweep.py (device).  (Test infrastructure.)

What the sweep computes (updatePhi: j outer, m inner, UpdatePhi.h:40-84; then updateNu, UpdateNu.h:39-70; updateSigma,
UpdateSigma.h:22-58).  Inputs, as the device holds them after k_factor of the iteration: the pair blocks H_ab (band-packed,
every block symmetric), t_a, C_a, L_a z_a, r0_a = t_a - sum_b H_ab theta0_b over ALL active b, hq0_a = H_aa theta0_a, the state
theta0 before the iteration, f = beta / sigma^2 with the sigma^2 of before the iteration, and YY = sum y^2.  Steps s = 0 .. S - 1
update the directions a_s: the Phi sweep (j outer, m inner) if U_PHI is set and MD > 1, then the nu sweep if U_NU is set;
directions outside the mask keep theta0.  Step s, a = a_s:

    r_a^(s) = r0_a - sum_{u < s} H_{a, a_u} delta_u,   rhs = f (r_a^(s) + hq0_a),   theta1_a = C_a rhs + L_a z_a,
    delta_s = theta1_a - theta0_a

and after the last step  RSS = YY - sum_a theta1_a'(t_a + r1_a),  r1_a = r0_a - sum_{all u} H_{a, a_u} delta_u.
sigma^2 is then 1 / Gamma(a, 1 / b) with b = RSS / 2 + beta_0 in every plain run: bfmmm_run passes tt_step = 0 whatever beta
is, and the kernels' `tempered` form (b = (beta / 2) RSS + beta_0, UpdateSigma.h:75-113) is taken for tt_step != 0 only; beta
enters a plain run through f alone; the tempered form is judged by tests/tempered_ref.py on runs of Sampler.run_tt, with check_steps
and check_rss of this file at f = beta / sigma^2.  (sigma^2 itself needs the gamma variate: tests/test_gpu_sweep.py::check_sigma
takes the oracle's, tests/scalar_jobs_ref.py the device's "gstd".)

Step check (check_steps).  Step s is judged ALONE: r_a^(s) is formed in np.longdouble from the device's own theta1 of the
earlier steps (delta_u = theta1_{a_u} - theta0_{a_u} is exact in longdouble), so an error of step 3 is not charged to step 7.
theta_ref = Cbar_a rhs + Lz_a with Cbar = (C + C') / 2, compared with theta1_a entry by entry under

    bound_p = sum_q |Cbar_pq| ( f c_r(s) u S_q + (P + 3) u |rhs_q| ) + sum_q |C_pq - C_qp| |rhs_q| + 2 u (|Lz_p| + |theta_ref,p|)
    S_q     = |r0_a[q]| + |hq0_a[q]| + sum_{u < s} sum_{|d| <= BW} |H_{a, a_u}[q, q + d]| (|theta1| + |theta0|)_{a_u}[q + d]
    c_r(s)  = (s + 1)(2 BW + 2) + 4,        u = 2^-53.

Derivation.  (i) The device's delta_u is fl(theta1 - theta0): a relative error u of a number of modulus <= |theta1| + |theta0|.
(ii) r_a^(s)[q] is r0_a[q] less s band products of at most 2 BW + 1 terms each, each product rounded once, each entering at
most 2 BW + 2 additions of its band sum in whatever order (general kernel: diagonal first, then pairs; chain wave: even and odd
pieces; row threads: upper and lower halves) and then the s subtractions: an entry of the sum of absolute terms S_q is carried
through at most s (2 BW + 2) + (2 BW + 2) roundings including (i), which is (s + 1)(2 BW + 2); the + 4 are r + hq, the product
with f, f = beta / sigma^2 itself and one spare.  First-order bound: |rhs^_q - rhs_q| <= f c_r(s) u S_q.  (iii) The mat-vec
sums P products in some tree (eight segments and a butterfly, or four column groups of eight in two accumulators): every
product passes at most P - 1 additions, is rounded once itself, the sum takes Lz (one more) and the result is stored: (P + 3) u
per term on |Cbar_pq| |rhs_q|, and the error of rhs passes through |Cbar_pq|.  (iv) The kernels read ONE triangle of the stored
C_a (row p of the draw is the stored column p), the reference the mean of both: on the pseudo-inverse route the two triangles
differ by rounding and sum_q |C_pq - C_qp| |rhs_q| covers either choice; on the Cholesky route and the diagonal model the term
is exactly 0.  (v) 2 u (|Lz_p| + |theta_ref,p|): the final addition and the reference's own rounding to the double it is
compared in.  Nothing is scaled by a global maximum; a direction outside the mask must come back BIT-EQUAL to theta0.

RSS check (check_rss).  RSS_ref is formed in longdouble from the device's theta1 and compared under  c_R u S_abs + E_r:
  S_abs = the larger of the sums of absolute terms of the two forms the kernels use,
            k_sweep / k_sweep_diag : YY + sum |theta1| (|t| + |r1|)
            k_sweep_chain          : YY + sum |theta0| (|t| + |r0|) + sum_s |delta_s|'(|H_aa| |delta_s| + 2 |r^(s)|)
  E_r   = sum_a |theta1_a|' c_r(S) u S(a) : the kernel's own r1 (and r^(s)) carries the rounding of part (ii) above, S steps
  c_R   = A P + 6 + 16 + 4 : a term passes at most A P - 1 additions of the per-thread and cross-thread sums in any order
          (A P terms in all; the chain's 2 A P + S P terms sit on at most A 16 + 64 threads, fewer additions per term), 6 levels
          of the wave butterfly and at most 16 wave partials are counted again on top for a layout that splits the sum
          differently, and 4 for the products of a term (theta (t + r): one addition, one product; delta (H delta - 2 r): the
          band sum is in S_abs term by term, the product by 2 is exact) and YY - q.
The bound is loose by design (the kernels' actual depth is ceil(A P / 1024) + 6 + 16): it is there to catch a dropped or
stale term, which is of the order of S_abs itself.

Emulations (float64, the same inputs): `emulate_general` -- the 8-segment mat-vec with its butterfly, r -= H delta per element
(diagonal, then upper + lower pairs), hq and the next rhs in phase B, the RSS per thread of 1024, wave butterfly, 16 partials;
`emulate_chain` -- the quad-split mat-vec (four column groups of eight, even and odd columns in two accumulators), r of rank
rk updated by the row threads for the deltas of the steps <= rk - 3 (upper half, lower half) and by the chain wave for the last
two (even / odd pieces of the H2 row), the incremental RSS  -theta0'(t + r0) + sum_s delta_s'(H_aa delta_s - 2 r^(s))  in the
row threads' layout.  They generate theta1 on the CPU; tests/test_sweep_ref.py holds both to a quarter of either bound on every
case and mask and shows that each mutation of them is rejected.  Largest error / bound of the emulations (recomputed and
asserted there):

    step bound : general 0.1423, chain 0.15 (both on cubic_P30-prior)      RSS bound : general 0.004686 (lin_P6-benign), chain 0.004846
    (quint_P27-stiff, phi_chi_zero)

CPU inputs (cpu_inputs): H and t from the basis rows in float64 (host_H_md), C_a and L_a z_a from factor_ref's longdouble
inverse rounded to float64 (the pseudo-inverse directions from factor_ref.emulate_pinv, whose C is asymmetric by rounding as
the device's is), r0 and hq0 in longdouble, rounded.

Safe masks for bfmmm_debug_get("rss"): the value is the sweep's after a run whose mask has U_SIGMA and causes no chi pass --
no U_CHI (with n_eigen > 0), no U_LOGLIK without U_SIGMA, no covariates; the deferred log-likelihood then rewrites Dyn::rss
with the value it read.  Every mask used here is a subset of U_NU | U_PHI | U_SIGMA.
"""
import copy

import numpy as np

import factor_ref as F

U, LD = F.U, F.LD
U_PHI, U_NU, U_SIGMA = 1 << 3, 1 << 7, 1 << 9      # bayesfmmm_amd.sampler's bits (asserted in tests/test_gpu_sweep.py)

# measured by tests/test_sweep_ref.py::test_emulations_pass_both_bounds (largest error / bound over every run of RUNS)
MEASURED_STEP_GENERAL, MEASURED_STEP_CHAIN = 0.1423, 0.15
MEASURED_RSS_GENERAL, MEASURED_RSS_CHAIN = 0.004686, 0.004846
EMU_LIMIT = 0.25


# ---------------------------------------------------------------------------------------------------------------------
# cases and runs
# ---------------------------------------------------------------------------------------------------------------------
def _case(name, regime="benign", **kw):
    return F.Case(name=f"{name}-{regime}", regime=regime, **kw)


# the instances the sweep's routes need beside factor_ref.CASES
SWEEP_CASES = [
    _case("cubic_P13", kind="spline", deg=3, P=13),                         # chain<3>, 8 lanes per rank, odd P
    _case("step_P10_pen1", kind="step", P=10, pen_band=1),                  # chain<0> with a banded penalty
    _case("cubic_P30_K4M5", kind="spline", deg=3, P=30, K=4, M=5),          # A = 24: 384 row threads, the chain's limit
    _case("cubic_P30_K5M4", kind="spline", deg=3, P=30, K=5, M=4),          # A = 25: k_sweep
    _case("cubic_P64_K3M2", kind="spline", deg=3, P=64, K=3, M=2),          # A LG + P^2 = 6400 > 6144: k_sweep direct
    _case("mv_P5_K8M7", kind="mv", P=5, K=8, M=7),                          # A = 64: k_sweep_diag<8, true>
    _case("step_P12_pen0", kind="step", P=12, pen_band=0),                  # functional diagonal model: k_sweep_diag<1, false>
    _case("mv_P7_K8M8", kind="mv", P=7, K=8, M=8),                          # A = 72 > 64: chain<0>
    _case("mv_P40_K8M8", kind="mv", P=40, K=8, M=8),                        # A = 72, P > 32: k_sweep's diagonal branch
    _case("cubic_P30_K2M1", kind="spline", deg=3, P=30, K=2, M=1),          # U_PHI alone: a 2-step sweep
    _case("quint_P27_K2M1", kind="spline", deg=5, P=27, K=2, M=1),
    _case("cubic_P30_4chains", kind="spline", deg=3, P=30, K=3, nch=4),     # two half-batches on two streams
]
ALL_CASES = F.CASES + SWEEP_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# the route every instance was written for: (kernel, template argument, mv, direct, lanes per rank of the chain's row threads)
EXPECTED_ROUTE = {
    "lin_P6": ("chain", 1, False, False, 4), "lin_P33": ("general", 0, False, False, 0),
    "quad_P29": ("chain", 2, False, False, 16), "quad_P64": ("general", 0, False, False, 0),
    "cubic_P30": ("chain", 3, False, False, 16), "cubic_P40": ("general", 0, False, False, 0),
    "quart_P32": ("chain", 4, False, False, 16), "quart_P50": ("general", 0, False, False, 0),
    "quint_P27": ("chain", 5, False, False, 16), "quint_P47": ("general", 0, False, False, 0),
    "mid_5x5": ("general", 0, False, False, 0), "mid_6x6": ("general", 0, False, False, 0),
    "wide_5x6": ("general", 0, False, True, 0), "wide_7x7": ("general", 0, False, True, 0),
    "mv_P7": ("diag", 2, True, False, 0), "mv_P64": ("diag", 1, True, False, 0),
    "cubic_P13": ("chain", 3, False, False, 8), "step_P10_pen1": ("chain", 0, False, False, 8),
    "cubic_P30_K4M5": ("chain", 3, False, False, 16), "cubic_P30_K5M4": ("general", 0, False, False, 0),
    "cubic_P64_K3M2": ("general", 0, False, True, 0), "mv_P5_K8M7": ("diag", 8, True, False, 0),
    "step_P12_pen0": ("diag", 1, False, False, 0), "mv_P7_K8M8": ("chain", 0, True, False, 4),
    "mv_P40_K8M8": ("general", 0, True, True, 0),
    "cubic_P30_K2M1": ("chain", 3, False, False, 16), "quint_P27_K2M1": ("chain", 5, False, False, 16),
    "cubic_P30_4chains": ("chain", 3, False, False, 16),
}


def expected_route(c, MD=None):
    """(kernel, template argument, mv, direct, block threads) the case was written for (MD = 1: phi_chi_zero, A = K)"""
    kern, targ, mv, direct, lrk = EXPECTED_ROUTE[c.name.split("-")[0]]
    A = c.K * (c.MD if MD is None else MD)
    if kern == "diag":
        return kern, (A + 7) // 8, mv, direct, (8 * c.P + 63) // 64 * 64
    if kern == "chain":
        return kern, targ, mv, direct, 64 + (A * lrk + 63) // 64 * 64
    return kern, targ, mv, direct, 1024


class Run:
    """one device run of a case: the mask, phi_chi_zero (MD = 1) and beta"""
    def __init__(self, case, mask, pcz=False, beta=1.0):
        self.case, self.mask, self.pcz, self.beta = case, mask, pcz, beta
        self.MD = 1 if pcz else case.MD
        bits = "+".join(n for n, b in (("nu", U_NU), ("phi", U_PHI), ("sigma", U_SIGMA)) if mask & b)
        self.id = f"{case.name}:{bits}" + (":pcz" if pcz else "") + (f":beta{beta}" if beta != 1.0 else "")


def _runs():
    full = U_NU | U_PHI
    out = [Run(c, full | U_SIGMA) for c in ALL_CASES]
    for inst, inst1 in (("cubic_P30", "cubic_P30_K2M1"), ("quint_P27", "quint_P27_K2M1")):
        for reg in ("benign", "stiff"):
            c = BY_NAME[f"{inst}-{reg}"]
            out += [Run(c, full), Run(c, U_NU), Run(c, U_NU | U_SIGMA), Run(c, U_PHI), Run(c, U_PHI | U_SIGMA),
                    Run(c, full, pcz=True), Run(c, full | U_SIGMA, pcz=True)]
        c1 = BY_NAME[f"{inst1}-benign"]
        out += [Run(c1, U_PHI), Run(c1, U_PHI | U_SIGMA), Run(c1, full)]
    out.append(Run(BY_NAME["cubic_P30-benign"], full | U_SIGMA, beta=0.37))
    out.append(Run(BY_NAME["quint_P27-stiff"], full | U_SIGMA, beta=0.37))
    return out


RUNS = _runs()
RUN_BY_ID = {r.id: r for r in RUNS}
assert len(RUN_BY_ID) == len(RUNS)


# ---------------------------------------------------------------------------------------------------------------------
# index maps (restated from the model, not from the kernels: UpdatePhi.h loops j then m, UpdateNu.h loops j)
# ---------------------------------------------------------------------------------------------------------------------
def sweep_steps(c, mask, MD=None, order=None):
    """the directions a_s = j MD + mt of the steps.  order: a mutation ("nu_first", "m_outer")"""
    MD = c.MD if MD is None else MD
    M = MD - 1
    phi = [j * MD + m + 1 for j in range(c.K) for m in range(M)] if (mask & U_PHI) and MD > 1 else []
    if order == "m_outer":
        phi = [j * MD + m + 1 for m in range(M) for j in range(c.K)] if phi else []
    nu = [j * MD for j in range(c.K)] if mask & U_NU else []
    return nu + phi if order == "nu_first" else phi + nu


def hrow_md(K, MD, a, b):
    ncc = MD * (MD + 1) // 2
    return F.tri(K, a // MD, b // MD) * ncc + F.tri(MD, a % MD, b % MD)


def view(c, MD=None):
    """the case as a run with MD active components per cluster sees it (MD = 1: phi_chi_zero)"""
    v = copy.copy(c)
    if MD is not None and MD != c.MD:
        v.MD, v.A = MD, c.K * MD
    return v


def theta_of(c, st, MD=None):
    """(A, P) active directions from a state's nu (K, P) and Phi (K, P, M)"""
    MD = c.MD if MD is None else MD
    th = np.zeros((c.K * MD, c.P))
    for j in range(c.K):
        th[j * MD] = st["nu"][j]
        for mt in range(1, MD):
            th[j * MD + mt] = st["Phi"][j, :, mt - 1]
    return th


def band_mv(Hb, v, lower=True, upper=True, absolute=False):
    """(H_block v)[p] of a band-packed symmetric block Hb[t, p] = G(p, p + t) in the dtype of its arguments"""
    nb, P = Hb.shape
    if absolute:
        Hb, v = np.abs(Hb), np.abs(v)
    out = Hb[0] * v
    for t in range(1, min(nb - 1, P - 1) + 1):
        g = Hb[t, :P - t]
        if upper:
            out[:P - t] = out[:P - t] + g * v[t:]
        if lower:
            out[t:] = out[t:] + g * v[:P - t]
    return out


class Blocks:
    """H (R x LG, band-packed) as blocks of active directions"""
    def __init__(self, c, H, MD, dtype):
        self.K, self.MD, self.P = c.K, MD, c.P
        self.H = np.asarray(H, dtype=np.float64).reshape(-1, c.BW + 1, c.P).astype(dtype)

    def __call__(self, a, b):
        return self.H[hrow_md(self.K, self.MD, a, b)]


# ---------------------------------------------------------------------------------------------------------------------
# the step check
# ---------------------------------------------------------------------------------------------------------------------
def c_r(s, BW):
    return (s + 1) * (2 * BW + 2) + 4


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def _r_at(HL, steps, a, s, r0a, hq0a, dl, dabs):
    """r_a with the deltas of the steps u < s applied, and S (the sum of absolute terms), in longdouble"""
    r, S = r0a.copy(), np.abs(r0a) + np.abs(hq0a)
    for u in range(s):
        Hb = HL(a, steps[u])
        r -= band_mv(Hb, dl[u])
        S += band_mv(Hb, dabs[u], absolute=True)
    return r, S


def check_steps(case, mask, theta0, theta1, H, Cmat, Lz, rvec, hq, f, MD=None):
    """every step of the sweep against longdouble, each judged alone (module docstring).  theta0, theta1, Lz, rvec, hq: (A, P) of
    the active directions; H: the device's band-packed blocks; Cmat: (A, P, P); f: beta / sigma^2 as a double.
    Returns dict(ok, worst (the largest error / bound), steps: [dict(s, a, j, mt, p, value, ref, err, bound, ratio, dmax, bmax)],
    frozen_ok (directions outside the mask bit-equal to theta0), msg)."""
    c = case
    MD = c.MD if MD is None else MD
    A, P, BW = c.K * MD, c.P, c.BW
    steps = sweep_steps(c, mask, MD)
    th0, th1 = _ld(theta0).reshape(A, P), _ld(theta1).reshape(A, P)
    HL = Blocks(c, H, MD, LD)
    C, lz, r0, hq0 = _ld(Cmat).reshape(A, P, P), _ld(Lz).reshape(A, P), _ld(rvec).reshape(A, P), _ld(hq).reshape(A, P)
    fL = LD(f)
    dl = [th1[a] - th0[a] for a in steps]
    dabs = [np.abs(th1[a]) + np.abs(th0[a]) for a in steps]
    res, worst = [], 0.0
    finite = bool(np.isfinite(np.asarray(theta1, dtype=np.float64)).all())
    for s, a in enumerate(steps):
        r, S = _r_at(HL, steps, a, s, r0[a], hq0[a], dl, dabs)
        rhs = fL * (r + hq0[a])
        Cb = (C[a] + C[a].T) / 2
        ref = Cb @ rhs + lz[a]
        bound = (np.abs(Cb) @ (fL * c_r(s, BW) * U * S + (P + 3) * U * np.abs(rhs)) + np.abs(C[a] - C[a].T) @ np.abs(rhs)
                 + 2 * U * (np.abs(lz[a]) + np.abs(ref)))
        err = np.abs(th1[a] - ref)
        b64, e64 = np.asarray(bound, dtype=np.float64), np.asarray(err, dtype=np.float64)
        ratio = np.where(b64 > 0, e64 / np.where(b64 > 0, b64, 1.0), np.where(e64 == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)
        p = int(np.argmax(ratio))
        res.append(dict(s=s, a=a, j=a // MD, mt=a % MD, p=p, value=float(th1[a][p]), ref=float(ref[p]), err=float(e64[p]),
                        bound=float(b64[p]), ratio=float(ratio[p]), dmax=float(np.abs(ref - th0[a]).max()), bmax=float(b64.max())))
        worst = max(worst, float(ratio[p]))
    frozen = [a for a in range(A) if a not in steps]
    t0, t1 = np.asarray(theta0, dtype=np.float64).reshape(A, P), np.asarray(theta1, dtype=np.float64).reshape(A, P)
    bad_frozen = [a for a in frozen if not np.array_equal(t0[a].view(np.uint64), t1[a].view(np.uint64))]
    ok = finite and worst <= 1.0 and not bad_frozen
    msg = ""
    if not ok:
        w = max(res, key=lambda x: x["ratio"]) if res else None
        msg = f"{c.name}: " + ("theta1 not finite; " if not finite else "")
        if w is not None and w["ratio"] > 1.0:
            msg += (f"step {w['s']}, direction a {w['a']} = (j {w['j']}, mt {w['mt']}), row p {w['p']}: value {w['value']!r}, reference "
                    f"{w['ref']!r}, error {w['err']:.3g}, bound {w['bound']:.3g}, error / bound {w['ratio']:.3g}; ")
        if bad_frozen:
            msg += f"directions outside the mask changed: {bad_frozen}"
    return dict(ok=ok, worst=worst, steps=res, frozen_ok=not bad_frozen, msg=msg)


def c_R(A, P):
    return A * P + 6 + 16 + 4


def check_rss(case, mask, theta0, theta1, H, tvec, rvec, hq, YY, rss, MD=None):
    """the device's RSS against YY - sum_a theta1_a'(t_a + r1_a) in longdouble from the device's theta1 (module docstring).
    Returns dict(ok, ratio, rss_ref, err, bound, msg)."""
    c = case
    MD = c.MD if MD is None else MD
    A, P, BW = c.K * MD, c.P, c.BW
    steps = sweep_steps(c, mask, MD)
    S = len(steps)
    th0, th1 = _ld(theta0).reshape(A, P), _ld(theta1).reshape(A, P)
    HL = Blocks(c, H, MD, LD)
    tv, r0, hq0 = _ld(tvec).reshape(A, P), _ld(rvec).reshape(A, P), _ld(hq).reshape(A, P)
    dl = [th1[a] - th0[a] for a in steps]
    dabs = [np.abs(th1[a]) + np.abs(th0[a]) for a in steps]
    q, form1, e_r = LD(0), LD(YY), LD(0)
    for a in range(A):
        r1, Sa = _r_at(HL, steps, a, S, r0[a], hq0[a], dl, dabs)
        q += (th1[a] * (tv[a] + r1)).sum()
        form1 += (np.abs(th1[a]) * (np.abs(tv[a]) + np.abs(r1))).sum()
        e_r += (np.abs(th1[a]) * (c_r(S, BW) * U * Sa)).sum()
    form2 = LD(YY) + (np.abs(th0) * (np.abs(tv) + np.abs(r0))).sum()
    for s, a in enumerate(steps):
        rs, _ = _r_at(HL, steps, a, s, r0[a], hq0[a], dl, dabs)
        form2 += (np.abs(dl[s]) * (band_mv(HL(a, a), dl[s], absolute=True) + 2 * np.abs(rs))).sum()
    ref = LD(YY) - q
    bound = float(c_R(A, P) * U * max(form1, form2) + e_r)
    err = float(abs(LD(rss) - ref)) if np.isfinite(rss) else np.inf
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
    return dict(ok=ratio <= 1.0, ratio=ratio, rss_ref=float(ref), err=err, bound=bound,
                msg=f"{c.name}: RSS {rss!r}, reference {float(ref)!r}, error {err:.3g}, bound {bound:.3g} = (c_R {c_R(A, P)}) u S_abs + E_r, "
                    f"error / bound {ratio:.3g}")


def reference_sweep(case, mask, theta0, H, Cmat, Lz, rvec, hq, f, MD=None):
    """the whole sweep in longdouble, every step from the reference's own earlier steps: theta1 (A, P) longdouble"""
    c = case
    MD = c.MD if MD is None else MD
    A, P = c.K * MD, c.P
    steps = sweep_steps(c, mask, MD)
    HL = Blocks(c, H, MD, LD)
    th = _ld(theta0).reshape(A, P).copy()
    C, lz, r0, hq0 = np.asarray(Cmat, dtype=LD).reshape(A, P, P), np.asarray(Lz, dtype=LD).reshape(A, P), _ld(rvec).reshape(A, P), _ld(hq).reshape(A, P)
    dl = []
    for s, a in enumerate(steps):
        r = r0[a].copy()
        for u in range(s):
            r -= band_mv(HL(a, steps[u]), dl[u])
        nw = ((C[a] + C[a].T) / 2) @ (LD(f) * (r + hq0[a])) + lz[a]
        dl.append(nw - th[a])
        th[a] = nw
    return th


# ---------------------------------------------------------------------------------------------------------------------
# inputs on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def host_H_md(c, st, MD):
    """factor_ref.host_H for MD active components per cluster (the pair weights are Z_ij chi~_im, chi~_i0 = 1), t_a and YY"""
    d = F.case_data(c)
    n, K, P, BW = c.n, c.K, c.P, c.BW
    A = K * MD
    chit = np.concatenate([np.ones((n, 1)), st["chi"]], axis=1)[:, :MD]
    W = np.einsum("ij,im->ijm", st["Z"], chit).reshape(n, A)
    if c.kind == "mv":
        G = np.stack([np.eye(P)] * n)
        sv = np.asarray(d["Y"], dtype=np.float64)
        YY = float((sv * sv).sum())
    else:
        G = np.stack([B.T @ B for B in d["B"]])
        sv = np.stack([B.T @ y for B, y in zip(d["B"], d["y"])])
        YY = float(sum((y * y).sum() for y in d["y"]))
    R = (K * (K + 1) // 2) * (MD * (MD + 1) // 2)
    H = np.zeros((R, BW + 1, P))
    nb = min(BW, P - 1)
    for a in range(A):
        for b in range(a, A):
            Hab = np.einsum("i,ipq->pq", W[:, a] * W[:, b], G)
            for t in range(nb + 1):
                H[hrow_md(K, MD, a, b), t, :P - t] = np.diagonal(Hab, t)
    return H, W.T @ sv, YY


_inputs = {}


def cpu_inputs(run, q=0):
    """the sweep's inputs of chain q of a run, computed on the CPU: dict(theta0, H, tvec, Cmat, Lz, rvec, hq, f, YY)"""
    key = (run.case.name, run.MD, run.beta, q)
    if key in _inputs:
        return _inputs[key]
    c, MD = run.case, run.MD
    v = view(c, MD)
    A, P = v.A, c.P
    st = F.case_state(c, q)
    H, tvec, YY = host_H_md(c, st, MD)
    f = run.beta / float(st["sigma_sq"][0])
    stf = dict(st)
    stf["sigma_sq"] = np.array([1.0 / f])       # build_prec forms 1 / sigma^2: beta / sigma^2 up to a rounding
    th0 = theta_of(c, st, MD)
    zfull = F.normals(c, q)
    z = np.stack([zfull[(a // MD) * c.MD + a % MD] for a in range(A)])
    hb = np.stack([H[hrow_md(c.K, MD, a, a)] for a in range(A)])
    Cm, Lz = np.zeros((A, P, P)), np.zeros((A, P))
    for a in range(A):
        if F.is_pinv_direction(v, a):
            Cm[a], Lz[a] = F.emulate_pinv(F.build_prec(v, hb[a], stf, a, np.float64), z[a])
            continue
        Prec = F.build_prec(v, hb[a], stf, a, LD)
        if c.diag:
            dg = np.diagonal(Prec)
            Cm[a], Lz[a] = np.diag(np.asarray(1 / dg, dtype=np.float64)), np.asarray(z[a].astype(LD) / np.sqrt(dg), dtype=np.float64)
        else:
            R = F.inverse_ld(Prec)
            assert R.ok, (c.name, a)
            Cm[a], Lz[a] = np.asarray(R.C, dtype=np.float64), np.asarray(R.L @ z[a].astype(LD), dtype=np.float64)
            Cm[a] = (Cm[a] + Cm[a].T) / 2
    HL = Blocks(c, H, MD, LD)
    thL = th0.astype(LD)
    r, hq = tvec.astype(LD), np.zeros((A, P), dtype=LD)
    for a in range(A):
        for b in range(A):
            w = band_mv(HL(a, b), thL[b])
            r[a] -= w
            if a == b:
                hq[a] = w
    out = dict(theta0=th0, H=H.reshape(H.shape[0], -1), tvec=tvec, Cmat=Cm, Lz=Lz, rvec=np.asarray(r, dtype=np.float64),
               hq=np.asarray(hq, dtype=np.float64), f=f, YY=YY)
    if len(_inputs) > 8:
        _inputs.clear()
    _inputs[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulations of the kernels' orders of operations
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_term", "drop_lower", "stale_delta", "no_hq", "nu_first", "m_outer", "f_no_beta", "last_row", "late_delta", "lz_next")


def _targets(S):
    """(s*, u*) of the mutations that touch one term: the last step, and the delta of step 1 (0 in a 2-step sweep)"""
    return S - 1, (1 if S >= 3 else 0)


def _butterfly64(acc):
    """acc += shfl_xor(acc, o) for o = 32 .. 1 within waves of 64: lane 0 of every wave"""
    x = np.asarray(acc, dtype=np.float64).reshape(-1, 64).copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lanes ^ o]
    return x[:, 0]


def _seq_sum(v):
    s = 0.0
    for x in v:
        s = s + x
    return s


def emulate_general(case, mask, inp, MD=None, mut=None, beta=1.0, rss_mut=None):
    """k_sweep's order of operations in float64: (theta1 (A, P), rss)"""
    c = case
    MD = c.MD if MD is None else MD
    A, P, BW = c.K * MD, c.P, c.BW
    steps = sweep_steps(c, mask, MD, order=mut if mut in ("nu_first", "m_outer") else None)
    S = len(steps)
    st_, ut_ = _targets(S)
    Hb = Blocks(c, inp["H"], MD, np.float64)
    th = np.array(inp["theta0"], dtype=np.float64).reshape(A, P).copy()
    tv, Lz = np.asarray(inp["tvec"]).reshape(A, P), np.asarray(inp["Lz"]).reshape(A, P)
    r, hq = np.array(inp["rvec"]).reshape(A, P).copy(), np.array(inp["hq"]).reshape(A, P).copy()
    Cm = np.asarray(inp["Cmat"]).reshape(A, P, P)
    f = inp["f"] / beta if mut == "f_no_beta" else inp["f"]
    r_start = r.copy()
    diag = c.BW == 0 and c.BWP == 0

    def rhs_of(a):
        return f * r[a] if mut == "no_hq" else f * (r[a] + hq[a])

    def apply(a, dlt, s):          # phase B of step s: r_b -= H_ba delta for every b, hq_a follows theta_a
        for b in range(A):
            if mut == "drop_term" and s == ut_ and b == steps[st_]:
                continue
            if mut == "stale_delta" and s == ut_:
                continue
            H = Hb(b, a)
            v = H[0] * dlt
            for dd in range(1, min(BW, P - 1) + 1):
                g = H[dd, :P - dd]
                up, lo = np.zeros(P), np.zeros(P)
                up[:P - dd] = g * dlt[dd:]
                if not (mut == "drop_lower" and s == ut_ and b == steps[st_]):
                    lo[dd:] = g * dlt[:P - dd]
                v = v + (up + lo)
            r[b] = r[b] - v
            if b == a:
                hq[b] = hq[b] + v

    pend = None
    rhs = rhs_of(steps[0]) if S else None
    for s, a in enumerate(steps):
        if diag:
            nw = np.diagonal(Cm[a]) * rhs + Lz[a]
        else:
            Cu = Cm[a].T                   # row p of the draw reads the stored column p
            seg = np.zeros((8, P))
            for q in range(P):
                seg[q & 7] = seg[q & 7] + Cu[:, q] * rhs[q]
            acc = ((seg[0] + seg[1]) + (seg[2] + seg[3])) + ((seg[4] + seg[5]) + (seg[6] + seg[7]))
            nw = acc + Lz[(a + 1) % A if mut == "lz_next" else a]
        if mut == "last_row":
            nw[P - 1] = th[a, P - 1]
        dlt = nw - th[a]
        th[a] = nw
        if mut == "late_delta":            # the update of step s - 1 arrives now, this one at the next step
            if pend is not None:
                apply(*pend)
            pend = (a, dlt, s)
        else:
            apply(a, dlt, s)
        if s + 1 < S:
            rhs = rhs_of(steps[s + 1])
    rr = r_start if rss_mut == "r0_for_r1" else r
    terms = th * (tv + rr)
    if rss_mut == "drop_direction":
        terms[A // 2] = 0.0
    flat = np.zeros((A * P + 1023) // 1024 * 1024)
    flat[:A * P] = terms.ravel()
    per = np.zeros(1024)
    for row in flat.reshape(-1, 1024):
        per = per + row
    rss = inp["YY"] - _seq_sum(_butterfly64(per))
    return th, rss


def emulate_chain(case, mask, inp, MD=None, mut=None, beta=1.0):
    """k_sweep_chain's order of operations in float64 (P <= 32, BW <= 5): (theta1 (A, P), rss)"""
    c = case
    MD = c.MD if MD is None else MD
    A, P, BW = c.K * MD, c.P, c.BW
    assert P <= 32 and BW <= 5
    steps = sweep_steps(c, mask, MD, order=mut if mut in ("nu_first", "m_outer") else None)
    S = len(steps)
    st_, ut_ = _targets(S)
    Hb = Blocks(c, inp["H"], MD, np.float64)
    th0 = np.asarray(inp["theta0"], dtype=np.float64).reshape(A, P)
    th = th0.copy()
    tv, Lz = np.asarray(inp["tvec"]).reshape(A, P), np.asarray(inp["Lz"]).reshape(A, P)
    r0, hq0 = np.asarray(inp["rvec"]).reshape(A, P), np.asarray(inp["hq"]).reshape(A, P)
    Cm = np.asarray(inp["Cmat"]).reshape(A, P, P)
    f = inp["f"] / beta if mut == "f_no_beta" else inp["f"]
    nb = min(BW, P - 1)

    def G(H, d):                          # G(p, p + d) for every p, zero outside the matrix
        out = np.zeros(P)
        if abs(d) > nb:
            return out
        if d >= 0:
            out[:P - d] = H[d, :P - d]
        else:
            out[-d:] = H[-d, :P + d]
        return out

    def shifted(v, d):                    # v[p + d], zero outside
        out = np.zeros(P)
        if d >= 0:
            out[:P - d] = v[d:]
        else:
            out[-d:] = v[:P + d]
        return out

    def rows_form(H, dlt, lower=True):    # the row threads: the upper half and the lower half of the band, each ascending
        a0 = G(H, 0) * dlt
        a1 = np.zeros(P)
        for dd in range(1, BW + 1):
            a0 = a0 + G(H, dd) * shifted(dlt, dd)
            if lower:
                a1 = a1 + G(H, -dd) * shifted(dlt, -dd)
        return a0 + a1

    def wave_form(H, dlt, lower=True):    # the chain wave: entries k = 0 .. 2 BW + 1 of the H2 row (the last a zero pad), even / odd
        v0, v1 = np.zeros(P), np.zeros(P)
        for k in range(2 * BW + 2):
            d = k - BW
            t = G(H, d) * shifted(dlt, d) if (d <= BW and (lower or d >= 0)) else np.zeros(P)
            if k == 0:
                v0 = t
            elif k == 1:
                v1 = t
            elif k & 1:
                v1 = v1 + t
            else:
                v0 = v0 + t
        return v0 + v1

    deltas, rbef = [], []
    for rk, a in enumerate(steps):
        r = r0[a].copy()
        last = rk - 1 if mut == "late_delta" else rk          # late: the delta of step rk - 1 has not arrived
        for u in range(last):
            if mut == "drop_term" and u == ut_ and rk == st_:
                continue
            if mut == "stale_delta" and u == ut_:
                continue
            low = not (mut == "drop_lower" and u == ut_ and rk == st_)
            H = Hb(a, steps[u])
            r = r - (rows_form(H, deltas[u], low) if u <= rk - 3 else wave_form(H, deltas[u], low))
        rbef.append(r)
        rhs = np.zeros(32)
        rhs[:P] = f * r if mut == "no_hq" else f * (r + hq0[a])
        Cu = np.zeros((P, 32))
        Cu[:, :P] = Cm[a].T                # row p of the draw reads the stored column p; columns beyond P meet rhs = 0
        grp = []
        for g in range(4):
            s0 = Cu[:, 8 * g] * rhs[8 * g]
            s1 = Cu[:, 8 * g + 1] * rhs[8 * g + 1]
            for u in range(1, 4):
                s0 = s0 + Cu[:, 8 * g + 2 * u] * rhs[8 * g + 2 * u]
                s1 = s1 + Cu[:, 8 * g + 2 * u + 1] * rhs[8 * g + 2 * u + 1]
            grp.append(s0 + s1)
        acc = (grp[0] + grp[1]) + (grp[2] + grp[3])
        nw = acc + Lz[(a + 1) % A if mut == "lz_next" else a]
        if mut == "last_row":
            nw[P - 1] = th[a, P - 1]
        deltas.append(nw - th[a])
        th[a] = nw
    # the incremental RSS in the row threads' layout: thread 64 + rk LRK + pp owns rows 2 pp, 2 pp + 1 of rank rk
    PH = (P + 1) // 2
    LRK = 4 if PH <= 4 else 8 if PH <= 8 else 16
    nthr = 64 + (A * LRK + 63) // 64 * 64
    rank_dirs = list(steps) + [a for a in range(A) if a not in steps]
    acc = np.zeros(nthr)
    for rk, a in enumerate(rank_dirs):
        va = rows_form(Hb(a, a), deltas[rk]) if rk < S else None
        for pp in range(PH):
            t = 64 + rk * LRK + pp
            p0 = 2 * pp
            x = -(th0[a, p0] * (tv[a, p0] + r0[a, p0]))
            if p0 + 1 < P:
                x = x - th0[a, p0 + 1] * (tv[a, p0 + 1] + r0[a, p0 + 1])
            if rk < S:
                x = x + deltas[rk][p0] * (va[p0] - 2.0 * rbef[rk][p0])
                if p0 + 1 < P:
                    x = x + deltas[rk][p0 + 1] * (va[p0 + 1] - 2.0 * rbef[rk][p0 + 1])
            acc[t] = -x
    rss = inp["YY"] - _seq_sum(_butterfly64(acc))
    return th, rss


def chain_layout_ok(c):
    """the shapes k_sweep_chain's layout can hold (32 rhs slots, H2 rows of band <= 5), whatever its thread limit says"""
    return c.P <= 32 and c.BW <= 5


def nonvacuity(case, mask, inp, MD=None):
    """per step, from the reference alone: (max_p bound_p, max_p |delta_s[p]|) of the longdouble sweep"""
    th1 = np.asarray(reference_sweep(case, mask, inp["theta0"], inp["H"], inp["Cmat"], inp["Lz"], inp["rvec"], inp["hq"], inp["f"], MD), dtype=np.float64)
    res = check_steps(case, mask, inp["theta0"], th1, inp["H"], inp["Cmat"], inp["Lz"], inp["rvec"], inp["hq"], inp["f"], MD)
    return [(x["s"], x["a"], x["bmax"], x["dmax"]) for x in res["steps"]]
