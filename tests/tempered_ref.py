"""High-precision restatement of the tempered-transition block (csrc/bfmmm_capi.hip: bfmmm_tempered_transition, and the `tempered`
form of the sigma^2 draw in csrc/kernels_sweep.hip / csrc/scalar_jobs.hpp: job_hyper_draws), its checks, bounds, two float64
emulations of the host arithmetic, their mutations and the case list shared by tests/test_tempered_ref.py (CPU) and
tests/test_gpu_tempered_steps.py (device).  (Test infrastructure.)  u = 2^-53; reference values are np.longdouble, restated from
BFMMM.h:1452-1460 (ladder), :1556-1672 (block), CalculateTTAcceptance.h:22-97 and UpdateSigma.h:75-113, not from the host code's
order of operations.

The block of iteration `iter` (the plain sweep of that iteration has run; the working state is chain slot `iter`):

    ladder[i] = g^i, g = beta_N_t^(1 / N_t), i = 0 .. N_t - 1.  The reference first sets ladder[N_t - 1] = beta_N_t and then lets the
        loop ladder[i] = ladder[i - 1] g run over i = 1 .. N_t - 1, which overwrites that rung: beta_N_t itself is reached only for
        N_t = 1 (no loop).
    sweep l = 1 .. 2 N_t runs at beta_l = ladder[ind(l)], ind(l) = l - 1 for l <= N_t and 2 N_t - l above (temp_ind steps up after the
        sweeps l < N_t, stays at l = N_t, steps down after l > N_t): N_t = 3 gives 1, g, g^2, g^2, g, 1.  Every keyed variate of sweep
        l carries tt_step = l in counter word 1 (attempt | tt_step << 16).
    sigma^2 of a tempered sweep = 1 / Gamma(a, 1 / b), a = beta N / 2 + alpha_0 (REAL division; N = n_obs_total, for the
        multivariate model too: n P), b = (beta / 2) RSS + beta_0.  The plain form has a = sum_i (n_i // 2) + alpha_0 (multivariate:
        (n P) // 2) and b = RSS / 2 + beta_0: the two differ at beta = 1 as soon as one n_i is odd.
    PZ(b, l) = -(b / 2) log(sig_l) N - (b / (2 sig_l)) rss_l, with sig_l, rss_l the sigma^2 and RSS of tempered state l (l = 0: the
        state before the block), and, m = 2 N_t,
    logA = sum_{i = 0}^{N_t - 2} [ PZ(ladder[i + 1], i) - PZ(ladder[i], i) - PZ(ladder[i + 1], m - i) + PZ(ladder[i], m - i) ]
        (N_t = 1: the empty sum, logA = 0.0 exactly, always accepted).
    accepted = log u < logA, u the keyed uniform UPD_TT_ACC, index 0, of (iter, tt_step 0).
    Rejected: the state of before the block comes back and chain slot `iter` is rewritten from it.  Accepted: the state of sweep
        2 N_t stays, EXCEPT gamma, which the reference's re-initialisation of the next iteration does not copy (BFMMM.h:1660-1671): the
        next iteration starts from the gamma of before the block.  Either way iteration iter + 1 draws with (iter + 1, tt_step 0).

Checks.
  check_ladder: ladder[0] = 1.0 exactly (N_t = 1: beta_N_t exactly); rung i >= 1 within LADDER_TOL(i) = (i (2 + |log beta_N_t| / N_t) + i)
      u relative: pow is within one unit in the last place of its result (2 u relative), its exponent 1 / N_t carries one rounding,
      which moves the result by |log beta_N_t| / N_t u relative, and rung i is that number through i - 1 roundings of products (i
      counted).  N_t = 4, beta_N_t = 0.3, i = 3: 9.9 u.
  check_schedule: the 2 N_t betas are entries of the DEVICE's ladder, bit for bit, in the order above.
  check_sigma: from the sweep's own RSS and its "gstd" entry, sigma^2 against ((beta / 2) RSS + beta_0) / g under SIGMA_RTOL = 1e-12
      relative, the figure of tests/test_gpu_sweep.py::check_sigma, for its reasons (three roundings of the device against the
      factor beta, or 1 / 2, a wrong form would show); the "gstd" entry itself against the oracle's keyed gamma at (iter, tt_step l)
      with shape beta N / 2 + alpha_0 under scalar_jobs_ref.gamma_variate's allowance.
  check_logA: |logA - logA_ref| <= G_LOGA c_logA(N_t) u S, S = the sum over the 4 (N_t - 1) PZ values of |(b / 2) log(sig) N| +
      |(b / (2 sig)) rss| (the two halves of a PZ have opposite signs for sig < 1 and cancel: the sum is taken over the halves), and
      c_logA(N_t) = T + 8, T = 4 (N_t - 1): a half passes the log (one unit in the last place: 2), the division b / (2 sig) (1; b / 2 and
      2 sig are exact), four products (b / 2 by log, by N, the quotient by rss, and one spare for 2 sig: 4), the subtraction inside PZ
      (1), and then at most T additions of the running sum, each of which rounds a partial sum no larger than S.  The PZ values are of
      the order N |log sig| each and cancel to a logA of order 1 .. 100: the bound is a few 1e-12 .. 1e-10 and must stay below
      LOGA_NONVACUOUS = 1e-9 of S, so that one dropped PZ (>= S / T) is ten orders above it.
  check_decision: log u against log of the keyed UPD_TT_ACC uniform under 4 u |log u| + 2 u (log at 1 unit in the last place, the
      reference's own rounding); accepted == (log u < logA) from the device's OWN two numbers, exactly.

G_LOGA.  Two float64 emulations of the host arithmetic: `host`, the four running additions per rung in the host's order, and
`grouped`, sum_i (ladder[i + 1] - ladder[i]) (q_i - q_{m - i}) with q_l = -(1 / 2) log(sig_l) N - rss_l / (2 sig_l), the pairs grouped by
rung.  G_LOGA = 4 x the largest error / (bound at G = 1) over every case of CASES (from the oracle's traces) and the synthetic
traces of tests/test_tempered_ref.py, measured there and asserted not to have grown; never from a device run:

    host 0.0478 (synthetic:Nt2:0), grouped 0.0543 (synthetic:Nt2:1)      ->  G_LOGA = 0.217

Pinning to the oracle (tests/test_tempered_ref.py).  The oracle's CalculateTTAcceptance forms every PZ as a running sum over the N
observations, not from (sigma^2, RSS): its logA is held to the bound above + ((N + 1) / 2 + 5) u S1 + (N + 5) u S2, S1 and S2 the
absolute sums of the first and second halves (oracle_allowance has the count), from the oracle's own sigma^2 and (longdouble) RSS
trace; decisions equal.

Mutations (MUTATIONS; tests/test_tempered_ref.py shows that each fails at >= 10 x its bound or flips an exact check):
    last_rung_beta      ladder[N_t - 1] = beta_N_t (the rung the loop overwrites)                       ladder, >= 10 x LADDER_TOL
    temp_ind_early      temp_ind stepped before the sweep: the schedule one sweep early                schedule, exact
    shape_half_sum      half_sum for N / 2 in the tempered shape                                        the "gstd" entry, >= 10 x
    rate_half_rss       RSS / 2 for (beta / 2) RSS in the tempered rate                                 sigma^2, >= 10 x SIGMA_RTOL
    pz_half_sum         half_sum for N in PZ                                                            logA, >= 10 x
    mirror_off_by_one   m - i - 1 for m - i                                                             logA, >= 10 x
    sign_swapped        the third of the four signs of logA                                             logA, >= 10 x
    tt0_key_in_sweep    a tt_step 0 key in a tempered sweep            the keyed variate, exact; L_a z_a of k_factor, >= 10 x (check_direction)
    ttl_key_after       a tt_step l key in the iteration after the block                                the keyed variate, exact
    gamma_not_restored  gamma not put back after acceptance                                             hand-over, exact
    slot_not_rewritten  slot `iter` not rewritten after rejection                                       hand-over, exact

Cases (CASES): (case, family, mask, N_t, beta_N_t, iter, seed, sweep kernel, accepted) on curve_update_ref / cov_ref cases of 21
curves.  The routes are asserted on the device: k_sweep_chain (cubic_P30), k_sweep (cubic_P40: n_obs_total = 459 and odd n_i),
k_sweep_diag (mv_P7: n P = 147), and D = 2 with the Xi block (cubic_P30_D2).  beta_N_t, iter and seed were chosen on the CPU, from
the oracle alone, so that every family sees an accepted and a rejected block and no |logA - log u| is below 1e3 x the bound.
"""
import math

import numpy as np

import factor_ref as F
import scalar_jobs_ref as J

U, LD = F.U, F.LD
UPD_TT_ACC, UPD_SIGMA = 40, 14          # update ids of the keyed generator (oracle/oracle.h, csrc/rng.hpp)
SWEEP_WARM = 0x207ff                    # bayesfmmm_amd.sampler.SWEEP_WARM (asserted in tests/test_gpu_tempered_steps.py)
COV_FULL = 0x1f800                      # COV_MEAN | COV_XI
SIGMA_RTOL = 1e-12
LOGA_NONVACUOUS = 1e-9
UNDECIDED = 1e3
# measured by tests/test_tempered_ref.py::test_emulations_pass_and_g_loga_holds (largest error / bound at G = 1)
MEASURED_LOGA = {"host": 0.0478, "grouped": 0.0543}
G_LOGA = 0.217


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class TTCase:
    """one block: the case (by name, in curve_update_ref.BY_NAME or cov_ref.BY_NAME), its family, N_t, beta_N_t, the iteration the
    block acts on, the RNG seed, the sweep kernel its runs must take and the outcome the oracle gives it"""
    def __init__(self, name, family, N_t, beta_N_t, it, seed, kernel, accepted, base=0):
        self.name, self.family, self.N_t, self.beta_N_t, self.it, self.seed, self.kernel, self.accepted, self.base = (
            name, family, N_t, beta_N_t, it, seed, kernel, accepted, base)
        self.cov = family == "covariates"
        self.mask = SWEEP_WARM | (COV_FULL if self.cov else 0)
        self.id = f"{name}:Nt{N_t}" + (f":base{base}" if base else "")

    @property
    def case(self):
        import cov_ref as V
        import curve_update_ref as R
        return V.BY_NAME[self.name] if self.cov else R.BY_NAME[self.name]


CASES = [
    TTCase("cubic_P30-benign", "functional", 4, 0.8, 2, F.SEED, "chain", True),
    TTCase("cubic_P30-benign", "functional", 2, 0.05, 3, F.SEED, "chain", False),
    TTCase("cubic_P30-benign", "functional", 1, 0.5, 2, F.SEED, "chain", True),
    TTCase("cubic_P40-benign", "functional", 3, 0.1, 2, F.SEED, "general", False),
    TTCase("cubic_P40-benign", "functional", 2, 0.9, 2, F.SEED, "general", True, base=1),
    TTCase("mv_P7-benign", "multivariate", 4, 0.3, 2, F.SEED, "diag", True),
    TTCase("mv_P7-benign", "multivariate", 3, 0.1, 3, F.SEED, "diag", False),
    TTCase("cubic_P30_D2-benign", "covariates", 2, 0.95, 2, 2, "chain", True),
    TTCase("cubic_P30_D2-benign", "covariates", 3, 0.1, 2, F.SEED, "chain", False),
]
AFTER_BLOCK = ("cubic_P30-benign:Nt4", "cubic_P30-benign:Nt2")      # the accepted and the rejected block whose next iteration is judged
BY_ID = {t.id: t for t in CASES}
assert len(BY_ID) == len(CASES)
ROUTED = ("cubic_P30-benign", "cubic_P40-benign", "mv_P7-benign", "cubic_P30_D2-benign")      # the cases of the single tempered sweeps
SINGLE_SWEEPS = ((0.37, 2), (1.0, 1))      # (beta, tt_step) of the single sweeps: a middle rung, and the block's first


def case_state(t):
    import cov_ref as V
    import curve_update_ref as R
    return V.case_state(t.case) if t.cov else R.case_state(t.case)


def dims_of(c):
    return J.dims_of(c)


def tempered_state(st, beta):
    """the state as factor_ref.precisions must see it in a sweep at temperature beta: the data term of Prec_a is f H_aa with
    f = beta / sigma^2, which build_prec forms as 1 / sigma_sq -- sigma_sq = sigma^2 / beta, kept in longdouble"""
    out = dict(st)
    out["sigma_sq"] = np.array([LD(float(np.ravel(st["sigma_sq"])[0])) / LD(beta)], dtype=LD)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# ladder, schedule, sigma^2
# ---------------------------------------------------------------------------------------------------------------------
def ladder(N_t, beta_N_t, mut=None):
    """the N_t rungs in longdouble"""
    b = LD(beta_N_t)
    if N_t == 1:
        return np.array([b], dtype=LD)
    g = np.exp(np.log(b) / LD(N_t))
    lad = np.array([g ** i for i in range(N_t)], dtype=LD)
    if mut == "last_rung_beta":
        lad[N_t - 1] = b
    return lad


def ladder_tol(i, N_t, beta_N_t):
    """relative allowance of rung i (module docstring)"""
    return (i * (2 + abs(math.log(beta_N_t)) / N_t) + i) * U


def schedule_index(N_t, mut=None):
    """ind(l) of the sweeps l = 1 .. 2 N_t (restated from BFMMM.h:1586-1634: the index steps after the sweep)"""
    out, ind = [], 0
    for l in range(1, 2 * N_t + 1):
        out.append(ind)
        if l < N_t:
            ind += 1
        if l > N_t:
            ind -= 1
    if mut == "temp_ind_early":      # the index steps BEFORE the sweep: the schedule shifted by one sweep (the last stays at rung 0)
        out = out[1:] + [0]
    return out


def check_ladder(N_t, beta_N_t, lad_dev, mut=None):
    """the device's ladder against the restatement: dict(worst, fails)"""
    ref = ladder(N_t, beta_N_t, mut)
    got = np.asarray(lad_dev, dtype=np.float64)
    out = dict(worst=0.0, fails=[])
    if got.shape != (N_t,):
        out["fails"].append(f"the ladder has {got.shape} entries, N_t is {N_t}")
        return out
    if got[0] != float(ref[0]):
        out["fails"].append(f"ladder[0] is {got[0]!r}, not {float(ref[0])!r} exactly")
    for i in range(1, N_t):
        r = float(abs(LD(got[i]) - ref[i]) / (ladder_tol(i, N_t, beta_N_t) * ref[i]))
        out["worst"] = max(out["worst"], r)
        if not r <= 1.0:
            out["fails"].append(f"ladder[{i}] is {got[i]!r}, the restatement {float(ref[i])!r}: error / allowance {r:.3g}")
    return out


def check_schedule(N_t, lad_dev, betas_dev, mut=None):
    """the betas of the 2 N_t sweeps are the device's own rungs in the order of the restatement, bit for bit: failures"""
    lad, got = np.asarray(lad_dev, dtype=np.float64), np.asarray(betas_dev, dtype=np.float64)
    if got.shape != (2 * N_t,):
        return [f"{got.shape} betas for N_t = {N_t}"]
    want = lad[schedule_index(N_t, mut)]
    bad = [l + 1 for l in range(2 * N_t) if got[l] != want[l]]
    return [f"sweeps {bad} ran at {got[[l - 1 for l in bad]]}, the schedule gives {want[[l - 1 for l in bad]]}"] if bad else []


def sigma_shape(beta, dims, hyp, mut=None):
    """a of the tempered draw as a double: what job_hyper_draws hands the gamma sampler"""
    if mut == "shape_half_sum":
        return beta * dims["half_sum"] + hyp["alpha_0"]
    return (beta * float(dims["n_obs_total"])) / 2 + hyp["alpha_0"]


def sigma_ref(beta, rss, g, hyp, mut=None):
    """sigma^2 of a tempered sweep from its RSS and its standard gamma variate, longdouble"""
    rate = (LD(rss) / 2 if mut == "rate_half_rss" else (LD(beta) / 2) * LD(rss)) + LD(hyp["beta_0"])
    return rate / LD(g)


def check_sigma(c, beta, tt, rss, gstd_sigma, s2_dev, dims, hyp, seed, it, q=0, mut=None):
    """the tempered sigma^2 of sweep tt of iteration `it` (module docstring): dict(worst (sigma^2, of SIGMA_RTOL), worst_g (the "gstd"
    entry, of its allowance), fails)"""
    ref = sigma_ref(beta, rss, gstd_sigma, hyp, mut)
    r = float(abs(LD(float(s2_dev)) - ref) / (SIGMA_RTOL * ref))
    out = dict(worst=r, worst_g=0.0, fails=[])
    if not r <= 1.0:
        out["fails"].append(f"{c.name}: tempered sigma^2 {float(s2_dev)!r}, ((beta / 2) RSS + beta_0) / g from the device's RSS gives {float(ref)!r} "
                            f"(relative difference {r * SIGMA_RTOL:.3g}, beta {beta}, tt_step {tt})")
    g, tol = J.gamma_variate(UPD_SIGMA, 0, sigma_shape(beta, dims, hyp, mut), seed, q, it, tt=0 if mut == "tt0_key_in_sweep" else tt)
    rg = J._ratio(abs(float(gstd_sigma) - g[0]), tol[0])
    out["worst_g"] = rg
    if not rg <= 1.0:
        out["fails"].append(f"{c.name}: the sigma^2 variate in \"gstd\" is {float(gstd_sigma)!r}, the keyed gamma of shape beta N / 2 + alpha_0 at "
                            f"(iteration {it}, tt_step {tt}) is {g[0]!r}: error / allowance {rg:.3g}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# logA and the decision
# ---------------------------------------------------------------------------------------------------------------------
def c_logA(N_t):
    return 4 * (N_t - 1) + 8


def pz_halves(b, sig, rss, N):
    """the two halves of PZ(b, l) in longdouble: PZ = first - second"""
    b, sig, rss = LD(b), LD(sig), LD(rss)
    return -(b / 2) * np.log(sig) * LD(N), (b / (2 * sig)) * rss


def logA_ref(lad, sig, rss, N, mut=None, half_sum=None):
    """(logA, S) in longdouble from the ladder, sig[0 .. 2 N_t], rss[0 .. 2 N_t] and N = n_obs_total (module docstring)"""
    N_t = len(lad)
    m = 2 * N_t
    Nn = half_sum if mut == "pz_half_sum" else N
    tot, S = LD(0), LD(0)
    for i in range(N_t - 1):
        mi = m - i - 1 if mut == "mirror_off_by_one" else m - i
        for sign, b, l in ((1, lad[i + 1], i), (-1, lad[i], i), (1 if mut == "sign_swapped" else -1, lad[i + 1], mi), (1, lad[i], mi)):
            a, c = pz_halves(b, sig[l], rss[l], Nn)
            tot += sign * (a - c)
            S += abs(a) + abs(c)
    return tot, S


def logA_bound(N_t, S):
    return float(G_LOGA * c_logA(N_t) * U * S)


def abs_halves(lad, sig, rss, N):
    """(S1, S2): the sums over the 4 (N_t - 1) PZ values of |(b / 2) log(sig) N| and of |(b / (2 sig)) rss|; S = S1 + S2"""
    N_t = len(lad)
    m = 2 * N_t
    S1, S2 = LD(0), LD(0)
    for i in range(N_t - 1):
        for b, l in ((lad[i + 1], i), (lad[i], i), (lad[i + 1], m - i), (lad[i], m - i)):
            a, c = pz_halves(b, sig[l], rss[l], N)
            S1, S2 = S1 + abs(a), S2 + abs(c)
    return S1, S2


def oracle_allowance(N, S1, S2):
    """what the ORACLE's logA may differ by on top of the bound above.  It forms every PZ as a running sum over the N observations
    of t_l = -(b / 2) log(sig) - (b / (2 sig)) res_l^2 (CalculateTTAcceptance.h:22-51).  Addition k rounds the partial sum of k terms:
    the first halves are N EQUAL terms, so their partial sums add up to (N + 1) / 2 times their total; the second halves vary with
    the residual and are counted N times; each t_l itself carries five roundings (the log, the square, two products, the
    difference):  ((N + 1) / 2 + 5) u S1 + (N + 5) u S2"""
    return float((((N + 1) / 2 + 5) * S1 + (N + 5) * S2) * U)


def emulate_host(lad, sig, rss, N):
    """float64, the host's order: four running additions per rung, PZ as (-(b / 2) log(sig)) N - (b / (2 sig)) rss"""
    N_t = len(lad)
    m, N = 2 * N_t, float(N)

    def PZ(b, l):
        return (-(b / 2) * math.log(sig[l])) * N - (b / (2 * sig[l])) * rss[l]

    lad, sig, rss = [float(x) for x in lad], [float(x) for x in sig], [float(x) for x in rss]
    logA = 0.0
    for i in range(N_t - 1):
        logA = logA + PZ(lad[i + 1], i)
        logA = logA - PZ(lad[i], i)
        logA = logA - PZ(lad[i + 1], m - i)
        logA = logA + PZ(lad[i], m - i)
    return logA


def emulate_grouped(lad, sig, rss, N):
    """float64, the pairs grouped by rung: sum_i (ladder[i + 1] - ladder[i]) (q_i - q_{m - i}), q_l = -(log(sig_l) N + rss_l / sig_l) / 2"""
    N_t = len(lad)
    m, N = 2 * N_t, float(N)
    lad, sig, rss = [float(x) for x in lad], [float(x) for x in sig], [float(x) for x in rss]
    q = [-(math.log(s) * N + r / s) / 2 for s, r in zip(sig, rss)]
    return math.fsum((lad[i + 1] - lad[i]) * (q[i] - q[m - i]) for i in range(N_t - 1))


def check_logA(N_t, lad, sig, rss, N, logA_dev, mut=None, half_sum=None):
    """the device's (or an emulation's) logA against the restatement from the same ladder, sig and rss: dict(worst, ref, S, bound, fails)"""
    ref, S = logA_ref(np.asarray(lad, dtype=np.float64).astype(LD), sig, rss, N, mut, half_sum)
    out = dict(worst=0.0, ref=float(ref), S=float(S), bound=logA_bound(N_t, S), fails=[])
    if N_t == 1:
        if logA_dev != 0.0:
            out["fails"].append(f"N_t = 1: logA is {logA_dev!r}, not 0.0 exactly")
            out["worst"] = np.inf
        return out
    out["worst"] = J._ratio(abs(LD(float(logA_dev)) - ref), out["bound"])
    if not out["worst"] <= 1.0:
        out["fails"].append(f"logA {float(logA_dev)!r}, the restatement {float(ref)!r}: error / bound {out['worst']:.3g} (bound {out['bound']:.3g}, "
                            f"sum of absolute terms {float(S):.6g})")
    if not out["bound"] <= LOGA_NONVACUOUS * float(S):
        out["fails"].append(f"the bound of logA {out['bound']:.3g} is not below {LOGA_NONVACUOUS} of the sum of absolute terms {float(S):.3g}")
    return out


def log_u_ref(seed, it, q=0, tt=0):
    """log of the keyed UPD_TT_ACC uniform of (iteration `it`, tt_step tt: 0 in the block) in longdouble"""
    import oracle_lib as O
    return np.log(LD(O.fill(0, 1, seed=seed, chain=q, it=it, upd=UPD_TT_ACC, tt=tt)[0]))


def check_decision(log_u_dev, logA_dev, accepted_dev, seed, it, q=0):
    """log u against the keyed uniform and the decision against the device's own two numbers: dict(worst, fails)"""
    ref = log_u_ref(seed, it, q)
    tol = 4 * U * abs(ref) + 2 * U
    r = float(abs(LD(float(log_u_dev)) - ref) / tol)
    out = dict(worst=r, fails=[])
    if not r <= 1.0:
        out["fails"].append(f"log u {float(log_u_dev)!r}, log of the keyed UPD_TT_ACC uniform of (iteration {it}, tt_step 0) {float(ref)!r}: error / allowance {r:.3g}")
    if bool(accepted_dev) != bool(log_u_dev < logA_dev):
        out["fails"].append(f"accepted = {bool(accepted_dev)} although log u = {log_u_dev!r} and logA = {logA_dev!r}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's block (CPU)
# ---------------------------------------------------------------------------------------------------------------------
_sim = {}


def oracle_chain(t, T):
    """(model, chain) of the oracle for case t with T slots, slot 0 the pushed state"""
    import oracle_lib as O
    import curve_update_ref as R
    c = t.case
    d = F.case_data(c)
    st = case_state(t)
    X = R.case_X(c) if t.cov else None
    if c.kind == "mv":
        model = O.Model(list(d["Y"]), [np.eye(c.P)] * c.n, c.K, c.M, X=X, mv=True, Pmat=np.eye(c.P))
    else:
        model = O.Model(d["y"], d["B"], c.K, c.M, X=X, Pmat=d["Pmat"])
    ch = O.Chain(model, T)
    kw = dict(nu=st["nu"], chi=st["chi"], Z=st["Z"], sigma=float(st["sigma_sq"][0]), Phi=st["Phi"], delta=st["delta"], gamma=st["gamma"],
              tau=st["tau"], pi=st["pi"], alpha3=float(st["alpha_3"][0]), A=st["A"])
    if t.cov:
        kw.update(eta=st["eta"], xi=st["xi"], tau_eta=st["tau_eta"], gamma_xi=st["gamma_xi"], delta_xi=st["delta_xi"], A_xi=st["A_xi"])
    for k, v in kw.items():      # (Chain.set_slot0 for slot `base`: the first iteration of the run is iteration `base`)
        arr = getattr(ch, k)
        if arr.ndim == 1:
            arr[t.base] = v
        elif k == "tau":
            arr[t.base, :] = v
        else:
            arr[..., t.base] = v
    return model, ch


def oracle_block(t):
    """the oracle's run of case t: the plain sweeps 0 .. iter, the block of iteration iter: dict(logA, accepted, sig, rss, log_u, N,
    half_sum); memoised"""
    if t.id in _sim:
        return _sim[t.id]
    import oracle_lib as O
    model, ch = oracle_chain(t, t.it + 2)
    L = 2 * t.N_t + 1
    buf = np.zeros(2 * L + 1)
    hook = O.lib().orc_tt_trace_hook
    hook(O.dp(buf), buf.size)
    try:
        logA, acc = O.run_warm_tt(model, O.make_hyper(t.case.K), ch, t.N_t, t.it, t.beta_N_t, n_iter=t.it + 1 - t.base, seed=t.seed,
                                  first_iter=t.base, covariance_adj=t.cov)
    finally:
        hook(None, 0)
    dm = dims_of(t.case)
    out = dict(logA=float(logA[t.it]), accepted=bool(acc[t.it] == 1), sig=buf[:L].copy(), rss=buf[L:2 * L].copy(), log_u=float(buf[2 * L]),
               N=dm["n_obs_total"], half_sum=dm["half_sum"], blocks=[i for i in range(t.it + 1) if acc[i] >= 0])
    _sim[t.id] = out
    return out


MUTATIONS = ("last_rung_beta", "temp_ind_early", "shape_half_sum", "rate_half_rss", "pz_half_sum", "mirror_off_by_one", "sign_swapped",
             "tt0_key_in_sweep", "ttl_key_after", "gamma_not_restored", "slot_not_rewritten")


# ---------------------------------------------------------------------------------------------------------------------
# the hand-over (what the device test asserts of sampler A against its snapshot and sampler B; the CPU test runs it on a model)
# ---------------------------------------------------------------------------------------------------------------------
STATE_NAMES = ("nu", "Phi", "chi", "Z", "delta", "A", "gamma")
COV_STATE_NAMES = ("eta", "xi", "tau_eta", "gamma_xi", "delta_xi", "A_xi")
SCALAR_NAMES = ("pi", "alpha_3", "sigma_sq", "tau")


def check_handover(accepted, after, snapshot, replay, slot, names):
    """the state after a block (`after`: name -> array) against the snapshot of before it and the state the replayed sweeps ended in
    (`replay`), and chain slot `iter` (`slot`: name -> array): accepted -- every array bit-equal to the replay, gamma to the snapshot;
    rejected -- every array bit-equal to the snapshot and the slot bit-equal to the state.  Failures."""
    fails = []
    for nm in names:
        a = np.ravel(after[nm])
        if accepted:
            want, src = (snapshot, "the snapshot of before the block") if nm == "gamma" else (replay, "the state the replayed sweeps ended in")
        else:
            want, src = snapshot, "the snapshot of before the block"
        if not np.array_equal(a, np.ravel(want[nm])):
            fails.append(f"{nm} after the {'accepted' if accepted else 'rejected'} block is not bit-equal to {src}")
        if not accepted and nm in slot and not np.array_equal(np.ravel(slot[nm]), a):
            fails.append(f"chain slot `iter` of {nm} is not bit-equal to the restored state")
    return fails
