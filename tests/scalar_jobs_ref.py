"""High-precision restatement of the main model's scalar jobs (csrc/scalar_jobs.hpp: job_pi_alpha, pi_alpha_tables, job_pi_prepare,
job_hyper_draws, job_hyper / delta_recursion, and the sigma^2 draw that closes the three sweep kernels), their per-entry checks,
bounds, two float64 emulations and the case list shared by tests/test_scalar_jobs_ref.py (CPU) and tests/test_gpu_scalar_jobs.py
(device).  (Test infrastructure.)  u = 2^-53; every reference value is np.longdouble, restated from the formulas of the reference's
Update*.h files (oracle/updates.c), not from the kernels' order of operations.

Inputs are the device's own arrays: the state the judged iteration started from (the pushed one, or chain slot t - 1), Z, nu and
Phi of iteration t itself (working state or chain slot t), "gstd", "piprep", "logz_part", "rss".  Every quantity is judged alone:
delta(k, i) is restated from the DEVICE's new delta(k, nn) for nn < i, gamma from the device's delta after the delta step, A from the
same, alpha_3 from the pi the device left.

Variates ("gstd", check_gstd).  job_hyper_draws (spare workgroups of k_factor) writes, whatever the mask,
    [ gamma: K P M | delta: K M | tau: K | A proposals: 2K | A uniforms: 2K | sigma: 1 | A terms: 8K ]
and job_pi_alpha, while recording, its two acceptance values in the two doubles behind.  (The draws do not look at the mask, so
no part of the array is "as before the run": every entry is held to its keyed variate after every run.)  Standard gammas against
the oracle's keyed variate under the AS241 allowance of cov_ref.check_gstd2: both are Marsaglia-Tsang draws d (1 + c z)^3 of the same
uniforms, so the normal's (32 |z| + 4) u passes through the cube as 3 c (32 |z| + 4) u / (1 + c z) relative, + 8 u for the products; a
shape below 1 (the boost path, g(a + 1) u0^(1 / a)) adds (8 + 4 |log u0| / a) u for pow and the rounding of 1 / a, with g(a + 1) read
from the oracle at shape a + 1 (same uniforms).  Shapes keep the reference's integer divisions: alpha_nu + P // 2; alpha_0 + half_sum
(sum_i n_i // 2) or, multivariate, alpha_0 + n_obs_total // 2; A_k0 + (P M) / 2.0 and A_k1 + (P (M - i)) / 2.0.  Ids: UPD_GAMMA index
(k P + p) M + m, UPD_DELTA k M + i, UPD_TAU k, UPD_SIGMA 0, UPD_A_PROP / UPD_A_ACC 2 j + i.  A proposals: rtruncnorm at 0, allowance
sd (32 |x| + 4) u + 2 u |na|.  The four A terms per cell, log(tgamma(a)) and log(a) at the current value and at the proposal:
16 u (|value| + 1) + the change of the value over the proposal's allowance.

pi / alpha_3 tables ("piprep", check_piprep: what job_pi_prepare leaves for iteration t + 1, from the pi and alpha_3 iteration t
left; the in-place evaluation of a run's first iteration is judged through the acceptance values).  g against UPD_PI_PROP under
the allowance above; each of the 6K + 6 lgamma_pos entries against lgamma_ld under the ABSOLUTE bound
    lg_bound(x) = 8 u ((x' - 1/2) |log x'| + x' + 1 + |log prod|) + 1.2e-14,   x' = x + s >= 8, prod = x (x + 1) .. (x + s - 1)
(the Stirling series through x'^-13 is cut where its next term, (7 / 6) / (182 x'^13) <= 1.2e-14, bounds the remainder; log Gamma has
zeros at 1 and 2, a relative bound means nothing there), evaluated at the device's own argument scale x pi_k as restated in
longdouble with the proposal's allowance carried through psi; the 2K logs 4 u |log| + 2 u + allowance; log u 4 u |log u| + 2 u; the
truncated-normal proposal and its two densities 16 u (sum of absolute terms + 1) + allowance.

pi and alpha_3 decisions (check_pi_alpha).  S_k = sum_i log Z_ik in longdouble from the Z the run left bit-equal ("logz_part" is
held to the same sums by curve_update_ref.check_logz).  Both acceptance values (UpdatePi.h:84-116, UpdateAlpha3.h:36-63) are
restated at the device's new pi where it accepted, at the keyed proposal g / sum g otherwise; the new pi must be bit-equal to the
old one or within the variate's allowance of the proposal; the recorded acceptance value must lie within the bound and the
decision must agree with log u < acc wherever |log u - acc| exceeds it; a step the bound leaves undecided is a failure of the
case (another seed).  alpha_3 uses the pi the pi step left (lB rows 3 / 5 after an acceptance).  Bound:
    G_ACC (c_acc u S + sum_j w_j lg_bound(x_j)) + |acc(x +- allowance) - acc(x)|
S the sum of absolute terms, w_j = n for the lB terms of the densities and 1 for those of the proposal, and
c_acc = 4 K + 12 + (GPB + 13): a log (2), the coefficient (a product, a difference), the product with S_k -- itself GPB + 4 roundings in
logz_part and 9 in the 256-lane tree --, 4 K additions in lane 0, the final combination.

delta, gamma, tau, sigma^2 (check_hyper, check_sigma).  Each G u c (sum of absolute terms) (+ the variate's allowance where the
variate is the oracle's, an iteration judged from chain slots alone):
    S_km = sum_p gamma_old phi^2       c_S = 13: two products, 8 serial additions of a lane, 3 DPP additions
    delta(k, i) = g / (1 + sum_{m >= i} S_km / 2 prod_{nn <= m, nn != i} delta(k, nn))      c = 2 M + c_S + 3: the carried prefix and running
        products (at most M multiplications: M (M + 1) / 2 over the whole recursion, each judged from the device's own earlier deltas),
        the product with S_km, M additions, the reciprocal and the product with g; every term is positive
    gamma = g 2 / (nu_1 + tilde-tau_new phi^2)      c = M + 5
    tau = g / (beta_nu + nu'P nu / 2)      c = P + 2 w + 7, w = min(BWP, P - 1) for the banded rows, P for whole rows; times the
        cancellation factor (beta_nu + |nu|'|P||nu| / 2) / (beta_nu + nu'P nu / 2) as tau_eta; multivariate: nu'nu, stored 1 / that
    sigma^2 = (rss / 2 + beta_0) / g       c = 4
A (check_A) cell by cell as cov_ref.check_axi: column 0 with log delta(k, 0), column 1 with (M - 1) log Gamma and sum_{q >= 1} log delta
(k, q) of the NEW delta (empty at M = 1), decisions judged under G_AACC u (M + 10) (S + 1) + the proposal's allowance.
Entries whose mask bit is off (all of delta / A / gamma at MD = 1) come back bit-equal and their chain slot is still written.

Constants: 4 x the largest error / (bound at G = 1) of two float64 emulations over CPU_CASES (`kernel`: 8 lanes per (k, m) with the
DPP tree, carried prefix products, banded rows, lgamma_pos, block partial sums of log Z; `plain`: numpy sums, products rebuilt from
scratch, dense rows, libm's lgamma), measured by tests/test_scalar_jobs_ref.py::test_emulations_pass_and_constants_hold, never from
a device run:

    delta:   kernel 0.131 (mv_P7),              plain 0.154 (quad_P29_K8M2-reject)   ->  G_DELTA = 0.616
    gamma:   kernel 0.325 (quad_P29_K8M2),      plain 0.328 (quad_P64_K5M2)          ->  G_GAMMA = 1.31
    tau:     kernel 0.116 (mv_P7),              plain 0.066 (lin_P6_K2M1)            ->  G_TAU = 0.464
    sigma:   kernel 0.426 (mid_5x5),            plain 0.145 (cubic_P30-n32)          ->  G_SIGMA = 1.7
    acc:     kernel 0.0287 (cubic_P30-reject),  plain 0.00879 (lin_P6_K2M16)         ->  G_ACC = 0.115
    A acc:   kernel 0.0862 (lin_P6_K2M16),      plain 0.188 (quint_P27_K5M8)         ->  G_AACC = 0.752

Every decision bound must stay below NONVACUOUS = 1e-3 of the margin |log u - acc| it judges.

Cases: n = 24 curves (factor_ref.case_data); the single-chain case that defers job_hyper needs two k-slices of the pair-Gram
contraction, n // 16 >= 2, so n = 32, and the one whose k_pair_gram gives the log-likelihood a workgroup of its own three, n = 48.
"""
import math
import zlib

import numpy as np

import curve_update_ref as R
import factor_ref as F

U, LD, SEED = F.U, F.LD, F.SEED
NONVACUOUS = 1e-3
KMAX, BWMAX = 8, 5
UPD_PI_PROP, UPD_PI_ACC, UPD_A3_PROP, UPD_A3_ACC = 3, 4, 5, 6      # update ids of the keyed generator (oracle/oracle.h, csrc/rng.hpp)
UPD_DELTA, UPD_A_PROP, UPD_A_ACC, UPD_GAMMA, UPD_TAU, UPD_SIGMA = 8, 9, 10, 11, 13, 14
U_Z, U_PI, U_ALPHA3, U_PHI, U_DELTA, U_A, U_GAMMA, U_NU, U_TAU, U_SIGMA, U_CHI = (1 << i for i in range(11))
U_LOGLIK = 1 << 17
SEVEN = U_PI | U_ALPHA3 | U_DELTA | U_A | U_GAMMA | U_TAU | U_SIGMA
BITS = dict(pi=U_PI, alpha_3=U_ALPHA3, delta=U_DELTA, A=U_A, gamma=U_GAMMA, tau=U_TAU, sigma_sq=U_SIGMA)
SWEEP_WARM = 0x207ff
MASK_LEAN = U_Z | SEVEN | U_NU      # no chi pass: over two or more iterations the Z update trails as the lean k_curve_z
LOG_SQRT_2PI = LD("0.918938533204672741780329736405617639861")
HYPER_DEFAULTS = dict(b=10.0, nu_1=3.0, alpha1l=1.0, alpha2l=2.0, beta1l=1.0, beta2l=1.0, a_pi_PM=1000.0, var_alpha3=0.05, var_epsilon1=1.0,
                      var_epsilon2=1.0, alpha_nu=10.0, beta_nu=1.0, alpha_0=1.0, beta_0=1.0)      # (oracle_lib.HYPER_DEFAULTS; c = 10)
HYP_NAMES = tuple(HYPER_DEFAULTS)

# measured by tests/test_scalar_jobs_ref.py::test_emulations_pass_and_constants_hold (largest error / bound at G = 1 over CPU_CASES)
MEASURED_DELTA = {"kernel": 0.131, "plain": 0.154}
MEASURED_GAMMA = {"kernel": 0.325, "plain": 0.328}
MEASURED_TAU = {"kernel": 0.116, "plain": 0.066}
MEASURED_SIGMA = {"kernel": 0.426, "plain": 0.145}
MEASURED_ACC = {"kernel": 0.0287, "plain": 0.00879}
MEASURED_AACC = {"kernel": 0.0862, "plain": 0.188}
G_DELTA, G_GAMMA, G_TAU, G_SIGMA, G_ACC, G_AACC = 0.616, 1.31, 0.464, 1.7, 0.115, 0.752
C_S = 13


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class SJCase(F.Case):
    """factor_ref.Case with n of its own, hyper parameters for default_config, a special state, the RNG seed of its runs, a
    chain-id stride, bits every run's mask carries besides the judged ones, the k-slices the route decision gives it, and the
    groups of runs the device test makes"""
    def __init__(self, name, n=24, pcz=False, cfg=None, state=None, seed=SEED, stride=1, carrier=0, nks=1, groups=("core", "bits", "multi"), **kw):
        super().__init__(name=name, **kw)
        self.n, self.pcz, self.cfg, self.state, self.seed, self.stride, self.carrier, self.nks, self.groups = n, pcz, dict(cfg or {}), state, seed, stride, carrier, nks, groups
        self.LPC = 32 if self.P <= 32 else 64
        self.GPB = 256 // self.LPC
        self.nblk = -(-self.n // self.GPB)

    @property
    def data_key(self):
        return ("sj", self.n) + super().data_key


_INST = {d["name"]: d for d in F._INST}


def _case(inst, suffix="", regime="benign", **kw):
    d = dict(_INST[inst]) if inst in _INST else {}
    d.update(kw)
    d.pop("name", None)
    return SJCase(name=inst + suffix, regime=regime, **d)


REJECT_CFG = dict(a_pi_PM=60.0, var_alpha3=2.5, var_epsilon1=3.0, var_epsilon2=3.0)


def _cases():
    lean = ("core", "bits", "multi", "lean")
    return [
        _case("lin_P6", "_K2M1", K=2, M=1),                              # empty sum for column 1 of A, no delta column >= 1
        _case("cubic_P30", K=3, M=2, groups=lean),                       # the common exact instance; job_hyper in the lean k_curve_z
        _case("quad_P29", "_K8M2", K=8, M=2),                            # K = KMAX: 54 lgamma lanes, 16 log lanes
        _case("quint_P27", "_K5M8", K=5, M=8),                           # K M = 40 > 32, register recursion, K P M = 1080 > 768, BWP = BWMAX
        _case("lin_P33", "_K2M9", K=2, M=9),                             # LDS recursion, ragged P over the 8-lane split
        _case("lin_P6", "_K2M16", K=2, M=16),                            # the build's largest M
        _case("quad_P64", "_K5M2", K=5, M=2),                            # K P = 320 > 256, all 8 trips of S_km
        _case("mid_5x5", K=2, M=2), _case("wide_5x6", K=2, M=2),         # BWP > BWMAX: whole-row nu'P nu
        _case("step_P10_pen1", kind="step", P=10, pen_band=1, K=2, M=2),      # narrow band, u > 2 BWP lanes off
        _case("mv_P7", K=3, M=2), _case("mv_P64", K=2, M=2),             # odd P in the integer divisions, inverted tau, the mv log-likelihood
        _case("cubic_P30", "-pcz", K=3, M=2, pcz=True),                  # MD = 1: delta / A / gamma off, tau on
        _case("cubic_P30", "-4chains", K=3, M=2, nch=4, stride=3, carrier=U_NU),      # packed path: job_pi_alpha in k_factor
        _case("cubic_P30", "-n32", K=3, M=2, n=32, nks=2, carrier=U_NU | U_CHI | U_LOGLIK),     # defer_hyper
        _case("cubic_P30", "-n48", K=3, M=2, n=48, nks=3, carrier=U_NU | U_CHI | U_LOGLIK),     # + PG_SOLO_LL
        _case("cubic_P30", "-smallpi", K=3, M=2, state="smallpi"),       # a_pi_PM pi_k < 1: the boost path of rgamma
        _case("cubic_P30", "-zerophi", K=3, M=2, state="zerophi"),       # S_km = 0, param2 = 1
        _case("cubic_P30", "-widedelta", K=3, M=2, state="widedelta"),   # log delta dominates the A ratio
        _case("cubic_P30", "-reject", K=3, M=2, cfg=REJECT_CFG, seed=2),      # proposals that are often rejected
        _case("quad_P29", "_K8M2-reject", K=8, M=2, cfg=REJECT_CFG, seed=1),
    ]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), [c.name for c in CASES]
# the emulations are measured, and the mutations judged, on every single-chain case
CPU_CASES = [c for c in CASES if c.nch == 1]


def hyp_of(c, cfg=None):
    """the hyper parameters of case c: the sampler's configuration, or (CPU tests) the oracle's defaults with the case's own"""
    if cfg is not None:
        h = {nm: float(getattr(cfg, nm)) for nm in HYP_NAMES}
        h["c"] = np.array([cfg.c[k] for k in range(c.K)], dtype=np.float64)
        return h
    h = dict(HYPER_DEFAULTS)
    h.update(c.cfg)
    h["c"] = np.full(c.K, 10.0)
    return h


def dims_of(c):
    """n_obs_total and half_sum = sum_i n_i // 2 of the case's data (the device: Sampler.dims())"""
    if c.kind == "mv":
        return dict(n_obs_total=c.n * c.P, half_sum=c.n * (c.P // 2))
    ni = [len(y) for y in F.case_data(c)["y"]]
    return dict(n_obs_total=int(sum(ni)), half_sum=int(sum(k // 2 for k in ni)))


def case_state(c, q=0):
    """factor_ref.case_state and the special states of the scalar jobs"""
    st = F.case_state(c, q)
    rng = np.random.default_rng(zlib.crc32(("sj" + c.name).encode()) + 17 * q)
    if c.state == "smallpi":
        pi = np.array(st["pi"], dtype=np.float64)
        pi[0] = 4e-4
        pi[1:] *= (1 - pi[0]) / pi[1:].sum()
        st["pi"] = pi
    elif c.state == "zerophi":
        st["Phi"][0] = 0.0
    elif c.state == "widedelta":
        st["delta"] = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), size=(c.K, c.M)))
    return st


def expected_route(c, mask, iters):
    """what "hyper_route" must report after a run of `mask` (carrier included) over `iters` iterations on case c"""
    MD = 1 if c.pcz else c.M + 1
    pg = bool(mask & (U_PHI | U_NU | U_SIGMA))
    chi_update = bool(mask & U_CHI) and MD > 1
    chi = chi_update or (bool(mask & U_LOGLIK) and not mask & U_SIGMA)
    z, zu = bool(mask & (U_Z | U_PI | U_ALPHA3)), bool(mask & U_Z)
    packed = pg and c.nch >= 4
    fuse = z and zu and chi and iters >= 2
    defer = not fuse and z and zu and c.K <= 4 and c.BW <= 5 and iters >= 2
    solo = c.nch == 1 and c.kind != "mv" and c.K <= 4 and c.M <= 8 and c.P <= 32 and (c.BW + 1) * c.P <= 128
    hyper = "deferred" if (pg and chi and c.nch == 1 and c.nks >= 2) else ("lean_z" if defer and not chi else "chi")
    pi = "factor" if packed else ("pair_gram_solo_ll" if (pg and solo and c.nks >= 3) else "pair_gram")
    return dict(hyper=hyper, pi=pi, pi_prepare=bool(mask & (U_PI | U_ALPHA3)))


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


_ratio = R._ratio


def pnorm(x):
    return 0.5 * math.erfc(-float(x) / math.sqrt(2.0))


# ---------------------------------------------------------------------------------------------------------------------
# keyed variates
# ---------------------------------------------------------------------------------------------------------------------
def gamma_variate(upd, idx, shape, seed, q, it, count=1, tt=0):
    """the oracle's keyed standard gamma variates of indices idx .. idx + count - 1 at one shape and their allowances (module
    docstring): (values, absolute tolerances)"""
    import oracle_lib as O
    shape = float(shape)
    ref = O.fill(2, idx + count, seed=seed, chain=q, it=it, upd=upd, p1=shape, p2=1.0, tt=tt)[idx:]
    a, base, extra = shape, ref, 0.0
    if shape < 1.0:
        base = O.fill(2, idx + count, seed=seed, chain=q, it=it, upd=upd, p1=shape + 1.0, p2=1.0, tt=tt)[idx:]
        extra = (8 + 4 * np.abs(np.log(ref / base))) * U
        a = shape + 1.0
    d = a - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * d)
    t = (base / d) ** (1.0 / 3.0)
    rel = (3 * cc * (32 * np.abs((t - 1) / cc) + 4) / t + 8) * U + extra
    return ref, rel * ref


def gstd_layout(c):
    K, P, M = c.K, c.P, c.M
    nG = K * P * M
    o = dict(gamma=(0, nG), delta=(nG, nG + K * M), tau=(nG + K * M, nG + K * M + K))
    at = nG + K * M + K
    o["aprop"], o["aunif"], o["sigma"], o["aterm"] = (at, at + 2 * K), (at + 2 * K, at + 4 * K), (at + 4 * K, at + 4 * K + 1), (at + 4 * K + 1, at + 12 * K + 1)
    o["acc"] = (at + 12 * K + 1, at + 12 * K + 3)
    o["len"] = nG + K * M + 13 * K + 8
    return o


def a_sd(hyp, i):
    return hyp["var_epsilon1"] / hyp["beta1l"] if i == 0 else hyp["var_epsilon2"] / hyp["beta2l"]


def variates(c, A_old, hyp, dims, q=0, it=0, seed=SEED, mut=None, tt=0, sigma_shape=None):
    """what job_hyper_draws must leave in "gstd" for the iteration that starts with A_old (K, 2), from the oracle's keyed generator:
    dict(g: the array up to the A terms, tol: its absolute allowances).  tt: the sweep of a tempered-transition block (counter word
    tt_step), whose sigma^2 variate has the shape sigma_shape (tempered_ref.sigma_shape) in place of alpha_0 + half_sum"""
    import oracle_lib as O
    K, P, M = c.K, c.P, c.M
    lay = gstd_layout(c)
    g, tol = np.zeros(lay["aterm"][1]), np.zeros(lay["aterm"][1])
    A_old = np.asarray(A_old, dtype=np.float64).reshape(K, 2)
    if K * P * M:
        g[slice(*lay["gamma"])], tol[slice(*lay["gamma"])] = gamma_variate(UPD_GAMMA, 0, (hyp["nu_1"] + 1) / 2, seed, q, it, K * P * M, tt=tt)
    for k in range(K):
        for i in range(M):
            shape = A_old[k, 0] + (P * M) / 2.0 if i == 0 else A_old[k, 1] + (P * (M - i)) / 2.0
            e = lay["delta"][0] + k * M + i
            g[e:e + 1], tol[e:e + 1] = gamma_variate(UPD_DELTA, k * M + i, shape, seed, q, it, tt=tt)
    g[slice(*lay["tau"])], tol[slice(*lay["tau"])] = gamma_variate(UPD_TAU, 0, hyp["alpha_nu"] + (P / 2.0 if mut == "tau_shape_real_div" else P // 2), seed, q, it, K, tt=tt)
    half = dims["n_obs_total"] // 2 if c.kind == "mv" else dims["half_sum"]
    if mut == "sigma_half_sum_real":
        half = dims["n_obs_total"] / 2.0
    e = lay["sigma"][0]
    g[e:e + 1], tol[e:e + 1] = gamma_variate(UPD_SIGMA, 0, hyp["alpha_0"] + half if sigma_shape is None else sigma_shape, seed, q, it, tt=tt)
    g[slice(*lay["aunif"])] = O.fill(0, 2 * K, seed=seed, chain=q, it=it, upd=UPD_A_ACC, tt=tt)
    tol[slice(*lay["aunif"])] = 2 * U
    for j in range(K):
        for i in range(2):
            cell, cur, sd = 2 * j + i, float(A_old[j, i]), a_sd(hyp, i)
            na = float(O.fill(3, cell + 1, seed=seed, chain=q, it=it, upd=UPD_A_PROP, p1=cur, p2=sd, tt=tt)[-1])
            tn = sd * (32 * abs((na - cur) / sd) + 4) * U + 2 * U * abs(na)
            g[lay["aprop"][0] + cell], tol[lay["aprop"][0] + cell] = na, tn
            e = lay["aterm"][0] + 4 * cell
            for o, a, ta in ((0, cur, 0.0), (2, na, tn)):
                lg, la = R.lgamma_ld(a), np.log(LD(a))
                g[e + o], g[e + o + 1] = float(lg), float(la)
                tol[e + o] = 16 * U * (abs(float(lg)) + 1) + float(abs(R.lgamma_ld(a + ta) - lg)) + float(abs(R.lgamma_ld(a - ta) - lg)) if ta else 16 * U * (abs(float(lg)) + 1)
                tol[e + o + 1] = 16 * U * (abs(float(la)) + 1) + 2 * ta / a
    return dict(g=g, tol=tol)


def check_gstd(c, gstd, var):
    """every entry of "gstd" up to the A terms against the keyed variates: dict(worst, fails)"""
    got = np.asarray(gstd, dtype=np.float64)
    lay = gstd_layout(c)
    out = dict(worst=0.0, fails=[])
    if got.shape[0] != lay["len"]:
        out["fails"].append(f"{c.name}: \"gstd\" has {got.shape[0]} entries, {lay['len']} are allocated")
        return out
    n = var["g"].shape[0]
    rat = np.array([_ratio(e, b) for e, b in zip(np.abs(got[:n] - var["g"]), var["tol"])])
    out["worst"] = float(rat.max())
    for e in np.argwhere(~(rat <= 1.0)).ravel()[:6]:
        part = next(nm for nm in ("gamma", "delta", "tau", "aprop", "aunif", "sigma", "aterm") if lay[nm][0] <= e < lay[nm][1])
        out["fails"].append(f"{c.name}: job_hyper_draws: gstd[{e}] ({part}, index {e - lay[part][0]}): {got[e]!r}, the keyed reference {var['g'][e]!r}, "
                            f"error / allowance {rat[e]:.3g}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pi / alpha_3
# ---------------------------------------------------------------------------------------------------------------------
def lg_bound(x):
    """the absolute bound of lgamma_pos(x) (module docstring)"""
    x = LD(x)
    lp = LD(0)
    while x < 8:
        lp += np.log(x)
        x += 1
    return float(8 * U * ((x - LD(0.5)) * abs(np.log(x)) + x + 1 + abs(lp)) + LD(1.2e-14))


def pi_draws(c, pi_old, alpha3, hyp, q, it, seed, tt=0):
    """the keyed variates of the pi / alpha_3 job of iteration `it`: the K gammas (allowances), the truncated-normal proposal of
    alpha_3 (allowance), log u of both tests"""
    import oracle_lib as O
    K = c.K
    pi_old, alpha3 = np.asarray(pi_old, dtype=np.float64).ravel(), float(np.ravel(alpha3)[0])
    g, gt = np.zeros(K), np.zeros(K)
    for k in range(K):
        a = hyp["a_pi_PM"] * pi_old[k]
        g[k:k + 1], gt[k:k + 1] = gamma_variate(UPD_PI_PROP, k, 10.0 if a <= 0 else a, seed, q, it, tt=tt)
    sd = hyp["var_alpha3"]
    ph = float(O.fill(3, 1, seed=seed, chain=q, it=it, upd=UPD_A3_PROP, p1=float(alpha3), p2=sd, tt=tt)[0])
    pt = sd * (32 * abs((ph - float(alpha3)) / sd) + 4) * U + 2 * U * abs(ph)
    lu = [np.log(LD(O.fill(0, 1, seed=seed, chain=q, it=it, upd=u, tt=tt)[0])) for u in (UPD_PI_ACC, UPD_A3_ACC)]
    pn = _ld(g) / _ld(g).sum()
    rel = gt / g + (gt / g).max() + 4 * U
    return dict(g=g, gtol=gt, pi_new=pn, pi_rel=rel, ph=ph, ph_tol=pt, lu=lu)


def _lB(v):
    """calc_lB (Distributions.h:51-60) of a longdouble vector: (value, sum of absolute terms, sum of the lgamma bounds)"""
    lg = [R.lgamma_ld(x) for x in v] + [R.lgamma_ld(v.sum())]
    return sum(lg[:-1], LD(0)) - lg[-1], sum((abs(x) for x in lg), LD(0)), sum(lg_bound(x) for x in v) + lg_bound(v.sum())


def acc_pi(c, pi_old, x, alpha3, S, hyp):
    """the acceptance value of updatePi_PM at the proposal x: (value, sum of absolute terms, weighted sum of the lgamma bounds)"""
    po, x, a3, ap, n = _ld(pi_old), np.asarray(x, dtype=LD), LD(float(alpha3)), LD(hyp["a_pi_PM"]), c.n
    cv = _ld(hyp["c"])
    lo, ln = np.log(po), np.log(x)
    terms = list((cv - 1) * ln) + list(-(cv - 1) * lo) + list((a3 * x - 1) * S) + list(-(a3 * po - 1) * S)
    lpn, lpo = list((ap * po - 1) * ln), list((ap * x - 1) * lo)
    b3n, b3o, bpn, bpo = _lB(a3 * x), _lB(a3 * po), _lB(ap * x), _lB(ap * po)
    val = sum(terms, LD(0)) - n * b3n[0] + n * b3o[0] + (sum(lpo, LD(0)) - bpn[0]) - (sum(lpn, LD(0)) - bpo[0])
    Sabs = sum((abs(t) for t in terms + lpn + lpo), LD(0)) + n * (b3n[1] + b3o[1]) + bpn[1] + bpo[1]
    return val, Sabs, n * (b3n[2] + b3o[2]) + bpn[2] + bpo[2]


def acc_a3(c, pi, cur, ph, S, hyp, pi_lB=None):
    """the acceptance value of updateAlpha3 at the proposal ph with the pi the pi step left (pi_lB: the pi of the lB terms)"""
    pi, cur, ph, n, sd = _ld(pi), LD(float(cur)), LD(float(ph)), c.n, hyp["var_alpha3"]
    pb = pi if pi_lB is None else _ld(pi_lB)
    bn, bo = _lB(ph * pb), _lB(cur * pb)
    lpc, lpp = np.log(LD(pnorm(cur / sd))), np.log(LD(pnorm(ph / sd)))
    terms = [-LD(hyp["b"]) * ph, LD(hyp["b"]) * cur] + list((ph * pi - 1) * S) + list(-(cur * pi - 1) * S) + [-lpc, lpp]
    val = sum(terms, LD(0)) - n * bn[0] + n * bo[0]
    Sabs = sum((abs(t) for t in terms), LD(0)) + n * (bn[1] + bo[1]) + 2 * (LOG_SQRT_2PI + abs(np.log(LD(sd))))
    return val, Sabs, n * (bn[2] + bo[2])


def c_acc(c):
    return 4 * c.K + 12 + c.GPB + 13


def _judge(name, what, logu, a0, bound, took, acc_dev, out):
    margin = abs(logu - a0)
    out["vacuous"] = max(out["vacuous"], _ratio(bound, margin))
    if acc_dev is not None:
        r = _ratio(abs(LD(acc_dev) - a0), bound)
        out["worst"] = max(out["worst"], r)
        if not r <= 1.0:
            out["fails"].append(f"{name}: {what}: acceptance value {acc_dev!r}, longdouble {float(a0)!r}, error / bound {r:.3g}")
    if not margin > bound:
        out["fails"].append(f"{name}: {what}: undecided by the reference (|log u - acc| {float(margin):.3g}, bound {float(bound):.3g}): choose another seed")
    elif took != bool(logu < a0):
        out["fails"].append(f"{name}: {what} was {'accepted' if took else 'rejected'}; log u {float(logu):.6g}, longdouble acceptance value {float(a0):.6g} "
                            f"(bound {float(bound):.3g})")
    if not _ratio(bound, margin) <= NONVACUOUS:
        out["fails"].append(f"{name}: {what}: the bound {float(bound):.3g} is not below {NONVACUOUS} of the margin {float(margin):.3g}")


def check_pi_alpha(c, pi_old, a3_old, Z, pi_dev, a3_dev, hyp, mask, q=0, it=0, seed=SEED, acc_dev=None, tt=0):
    """the pi and alpha_3 steps of iteration `it` (module docstring): dict(worst, vacuous, fails, outcome: {"pi", "alpha_3": bool})"""
    out = dict(worst=0.0, vacuous=0.0, fails=[], outcome={})
    pi_old, pi_dev = np.asarray(pi_old, dtype=np.float64).ravel(), np.asarray(pi_dev, dtype=np.float64).ravel()
    a3_old, a3_dev = float(np.ravel(a3_old)[0]), float(np.ravel(a3_dev)[0])
    S = np.log(_ld(Z).reshape(c.n, c.K)).sum(axis=0)
    dr = pi_draws(c, pi_old, a3_old, hyp, q, it, seed, tt)
    if mask & U_PI:
        took = not np.array_equal(pi_dev, pi_old)
        x = dr["pi_new"]
        if took:
            bad = np.abs(_ld(pi_dev) - x) > dr["pi_rel"] * x
            if bad.any():
                out["fails"].append(f"{c.name}: job_pi_alpha: pi {pi_dev} is neither the old pi {pi_old} nor the keyed proposal {np.asarray(x, dtype=np.float64)}")
            x = _ld(pi_dev)
        a0, Sa, lgb = acc_pi(c, pi_old, x, a3_old, S, hyp)
        sens = LD(0)
        if not took:
            for k in range(c.K):
                xp = x.copy()
                xp[k] *= 1 + LD(dr["pi_rel"][k])
                sens += abs(acc_pi(c, pi_old, xp, a3_old, S, hyp)[0] - a0)
        bound = G_ACC * (c_acc(c) * U * Sa + lgb) + sens
        _judge(c.name, "job_pi_alpha: the pi step", dr["lu"][0], a0, bound, took, None if acc_dev is None else acc_dev[0], out)
        out["outcome"]["pi"] = took
    elif not np.array_equal(pi_dev, pi_old):
        out["fails"].append(f"{c.name}: job_pi_alpha: pi changed although its mask bit is off")
    if mask & U_ALPHA3:
        took = a3_dev != a3_old
        ph, tol = dr["ph"], dr["ph_tol"]
        if took:
            if not abs(a3_dev - ph) <= tol:
                out["fails"].append(f"{c.name}: job_pi_alpha: alpha_3 {a3_dev!r} is neither its old value {a3_old!r} nor the keyed proposal {ph!r}")
            ph = a3_dev
        a0, Sa, lgb = acc_a3(c, pi_dev, a3_old, ph, S, hyp)
        sens = max(abs(acc_a3(c, pi_dev, a3_old, ph + tol, S, hyp)[0] - a0), abs(acc_a3(c, pi_dev, a3_old, ph - tol, S, hyp)[0] - a0))
        bound = G_ACC * (c_acc(c) * U * Sa + lgb) + sens
        _judge(c.name, "job_pi_alpha: the alpha_3 step", dr["lu"][1], a0, bound, took, None if acc_dev is None else acc_dev[1], out)
        out["outcome"]["alpha_3"] = took
    elif a3_dev != a3_old:
        out["fails"].append(f"{c.name}: job_pi_alpha: alpha_3 changed although its mask bit is off")
    return out


def check_piprep(c, tab, pi, alpha3, hyp, q, it, seed=SEED, tt=0):
    """ "piprep" as job_pi_prepare leaves it for iteration `it` from pi and alpha_3 (module docstring): dict(worst, fails)"""
    K = c.K
    t = np.asarray(tab, dtype=np.float64)
    out = dict(worst=0.0, fails=[])
    if t.shape[0] != 9 * KMAX + 16:
        out["fails"].append(f"{c.name}: \"piprep\" has {t.shape[0]} entries")
        return out
    g, lg, ph, lu, lp, dt = t[:K], t[KMAX:KMAX + 6 * K + 6], t[7 * KMAX + 8], t[7 * KMAX + 10:7 * KMAX + 12], t[7 * KMAX + 12:7 * KMAX + 12 + 2 * K], t[9 * KMAX + 12:9 * KMAX + 14]
    dr = pi_draws(c, pi, alpha3, hyp, q, it, seed, tt)
    po, a3, sd = _ld(pi).ravel(), float(np.ravel(alpha3)[0]), hyp["var_alpha3"]

    def hold(what, got, ref, bound):
        r = _ratio(abs(LD(got) - ref), bound)
        out["worst"] = max(out["worst"], r)
        if not r <= 1.0:
            out["fails"].append(f"{c.name}: job_pi_prepare (iteration {it}): {what}: {got!r}, reference {float(ref)!r}, error / bound {r:.3g}")

    for k in range(K):
        hold(f"g[{k}] (shape {hyp['a_pi_PM'] * float(po[k])!r})", g[k], LD(dr["g"][k]), dr["gtol"][k])
    hold("the alpha_3 proposal", ph, LD(dr["ph"]), dr["ph_tol"])
    pn = _ld(g) / _ld(g).sum()          # the device's own proposal: the tables are judged from it
    sc = (LD(hyp["a_pi_PM"]), LD(hyp["a_pi_PM"]), LD(a3), LD(a3), LD(float(ph)), LD(float(ph)))
    for row in range(6):
        v = sc[row] * (pn if row & 1 else po)
        for k in range(K + 1):
            x = v[k] if k < K else v.sum()
            e = row * K + k if k < K else 6 * K + row
            hold(f"lgamma_pos entry {e} (row {row}, {'k ' + str(k) if k < K else 'sum'}, argument {float(x)!r})", lg[e], R.lgamma_ld(x), lg_bound(x) + 8 * U * abs(float(x) * math.log(max(float(x), 1e-300))) + 4 * U)
    for e in range(2 * K):
        ref = np.log(po[e] if e < K else pn[e - K])
        hold(f"log entry {e}", lp[e], ref, 4 * U * abs(ref) + 6 * U)
    for e in range(2):
        hold(f"log u[{e}]", lu[e], dr["lu"][e], 4 * U * abs(dr["lu"][e]) + 2 * U)
    for e, m in enumerate((float(ph), a3)):
        ref = -LOG_SQRT_2PI - np.log(LD(sd)) - np.log(LD(pnorm(m / sd)))
        hold(f"dtruncnorm_lo_log term {e}", dt[e], ref, 16 * U * (LOG_SQRT_2PI + abs(np.log(LD(sd))) + abs(np.log(LD(pnorm(m / sd)))) + 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# delta, gamma, tau, A, sigma^2
# ---------------------------------------------------------------------------------------------------------------------
def penalty(c, dtype=LD):
    return np.eye(c.P, dtype=dtype) if c.kind == "mv" else np.asarray(F.case_data(c)["Pmat"], dtype=np.float64).astype(dtype)


def hyper_ref(c, st_in, nu, Phi, g, hyp, mask, pcz=False, delta_dev=None, delta_cur=None):
    """delta (K, M), gamma (K, P, M), tau (K) in longdouble from the state the iteration started from, nu (K, P) and Phi (K, P, M)
    of the iteration and the standard variates g ("gstd" layout).  delta_dev: the device's new delta, used for nn < i (each
    delta judged alone; None: the reference's own); delta_cur: the delta the gamma step sees (None: the reference's).
    dict(delta, gamma, tau, tau_amp, S)"""
    K, P, M = c.K, c.P, c.M
    lay = gstd_layout(c)
    g = _ld(g)
    phi_on = not pcz
    out = {}
    d_old = _ld(st_in["delta"]).reshape(K, M)
    ph2 = _ld(Phi).reshape(K, P, M) ** 2
    S = (_ld(st_in["gamma"]).reshape(K, P, M) * ph2).sum(axis=1)
    out["S"] = S
    d_new = d_old.copy()
    if (mask & U_DELTA) and phi_on:
        gd = g[slice(*lay["delta"])].reshape(K, M)
        src = d_old.copy() if delta_dev is None else _ld(delta_dev).reshape(K, M)
        for k in range(K):
            cur = d_old[k].copy()
            for i in range(M):
                p2 = LD(1)
                for m in range(i, M):
                    tt = LD(1)
                    for nn in range(m + 1):
                        if nn != i:
                            tt = tt * cur[nn]
                    p2 = p2 + tt * S[k, m] / 2
                d_new[k, i] = gd[k, i] / p2
                cur[i] = d_new[k, i] if delta_dev is None else src[k, i]
        out["delta"] = d_new
    if (mask & U_GAMMA) and phi_on:
        dc = d_new if delta_cur is None else _ld(delta_cur).reshape(K, M)
        tt = np.cumprod(dc, axis=1)
        out["gamma"] = g[slice(*lay["gamma"])].reshape(K, P, M) * (2 / (LD(hyp["nu_1"]) + tt[:, None, :] * ph2))
    if mask & U_TAU:
        Pm = penalty(c)
        nv = _ld(nu).reshape(K, P)
        qf = np.einsum("kp,pq,kq->k", nv, Pm, nv)
        qa = np.einsum("kp,pq,kq->k", np.abs(nv), np.abs(Pm), np.abs(nv))
        b = LD(hyp["beta_nu"]) + qf / 2
        v = g[slice(*lay["tau"])] / b
        out["tau"] = 1 / v if c.kind == "mv" else v
        out["tau_amp"] = (LD(hyp["beta_nu"]) + qa / 2) / b
    return out


def c_tau(c):
    w = 0 if c.kind == "mv" else (c.P if c.BWP > BWMAX else min(c.BWP, c.P - 1))
    return c.P + 2 * w + 7


def check_hyper(c, st_in, st_out, nu, Phi, g, gtol, hyp, mask, pcz=False):
    """the device's new delta / gamma / tau (st_out) against hyper_ref, each entry under its own bound (module docstring); gtol: the
    absolute allowances of g (zeros where g is the device's own "gstd").  dict(worst_delta, worst_gamma, worst_tau, fails)"""
    K, P, M = c.K, c.P, c.M
    lay = gstd_layout(c)
    ref = hyper_ref(c, st_in, nu, Phi, g, hyp, mask, pcz, delta_dev=st_out["delta"], delta_cur=st_out["delta"])
    grel = np.abs(np.asarray(gtol, dtype=np.float64)) / np.maximum(np.abs(np.asarray(g, dtype=np.float64)[:len(gtol)]), 1e-300)
    out = dict(worst_delta=0.0, worst_gamma=0.0, worst_tau=0.0, fails=[])
    spec = (("delta", (K, M), G_DELTA * (2 * M + C_S + 3), grel[slice(*lay["delta"])].reshape(K, M)),
            ("gamma", (K, P, M), G_GAMMA * (M + 5), grel[slice(*lay["gamma"])].reshape(K, P, M)),
            ("tau", (K,), G_TAU * c_tau(c), grel[slice(*lay["tau"])]))
    for nm, shp, gc, gr in spec:
        got = np.asarray(st_out[nm], dtype=np.float64).reshape(shp)
        if nm not in ref:
            if not np.array_equal(got, np.asarray(st_in[nm], dtype=np.float64).reshape(shp)):
                out["fails"].append(f"{c.name}: job_hyper: {nm} changed although its step is off")
            continue
        val = ref[nm]
        bound = (gc * U * (ref["tau_amp"] if nm == "tau" else 1) + gr) * np.abs(val)
        rat = np.array([_ratio(e, b) for e, b in zip(np.abs(got.astype(LD) - val).ravel(), np.broadcast_to(bound, val.shape).ravel())])
        k = int(np.argmax(rat))
        out["worst_" + nm] = float(rat[k])
        if not rat[k] <= 1.0:
            idx = np.unravel_index(k, val.shape)
            out["fails"].append(f"{c.name}: job_hyper: {nm}{tuple(int(x) for x in idx)}: {float(got[idx])!r}, reference {float(val[idx])!r}, error / bound {rat[k]:.3g}")
    return out


def a_cells(c, A_old, delta_cur, var, hyp, sum_from=1):
    """the A step (UpdateA.h:58-123) of every cell (j, i): list of dict(cell, cur, na, tol, logu, acc(a) -> (value, sum of abs terms))"""
    K, M = c.K, c.M
    lay = gstd_layout(c)
    A_old = np.asarray(A_old, dtype=np.float64).reshape(K, 2)
    lg = np.log(_ld(delta_cur).reshape(K, M))
    out = []
    for j in range(K):
        for i in range(2):
            cell, cur, sd = 2 * j + i, float(A_old[j, i]), a_sd(hyp, i)
            na, tol = float(var["g"][lay["aprop"][0] + cell]), float(var["tol"][lay["aprop"][0] + cell])
            al, be = (hyp["alpha1l"], hyp["beta1l"]) if i == 0 else (hyp["alpha2l"], hyp["beta2l"])
            kk = 1 if i == 0 else M - 1
            sl = lg[j, 0] if i == 0 else lg[j, sum_from:].sum()

            def acc(na, cur=cur, sd=sd, kk=kk, sl=sl, al=al, be=be):
                na, cu = LD(na), LD(cur)
                terms = []
                for x, sign in ((na, 1), (cu, -1)):
                    terms += [-sign * kk * R.lgamma_ld(x), sign * (x - 1) * sl, sign * (LD(al) - 1) * np.log(x), -sign * x * LD(be)]
                terms += [-np.log(LD(pnorm(float(na) / sd))), np.log(LD(pnorm(float(cu) / sd)))]
                return sum(terms, LD(0)), sum((abs(t) for t in terms), LD(0)) + ((cu - na) / LD(sd)) ** 2

            out.append(dict(cell=(j, i), cur=cur, na=na, tol=tol, logu=np.log(LD(var["g"][lay["aunif"][0] + cell])), acc=acc))
    return out


def check_A(c, A_old, A_dev, delta_cur, var, hyp, mask, pcz=False, acc_emu=None):
    """every cell of A: bit-equal to its old value or within the allowance of the keyed proposal, the decision as the longdouble
    acceptance value has it (module docstring).  acc_emu: an emulation's acceptance values (2K), held to the bound too.
    dict(worst, vacuous, fails, outcome: {"A0": [bool], "A1": [bool]})"""
    out = dict(worst=0.0, vacuous=0.0, fails=[], outcome={"A0": [], "A1": []})
    A_old, A_dev = np.asarray(A_old, dtype=np.float64).reshape(c.K, 2), np.asarray(A_dev, dtype=np.float64).reshape(c.K, 2)
    if not ((mask & U_A) and not pcz):
        if not np.array_equal(A_dev, A_old):
            out["fails"].append(f"{c.name}: job_hyper: A changed although its step is off")
        return out
    for r in a_cells(c, A_old, delta_cur, var, hyp):
        j, i = r["cell"]
        got, cur, na, tol = float(A_dev[j, i]), r["cur"], r["na"], r["tol"]
        took = got != cur
        if took and not abs(got - na) <= tol:
            out["fails"].append(f"{c.name}: job_hyper: A{r['cell']} {got!r} is neither its old value {cur!r} nor the keyed proposal {na!r}")
            continue
        x = got if took else na
        a0, Sa = r["acc"](x)
        bound = G_AACC * (c.M + 10) * U * (Sa + 1) + max(abs(r["acc"](x + tol)[0] - a0), abs(r["acc"](x - tol)[0] - a0))
        _judge(c.name, f"job_hyper: A{r['cell']}", r["logu"], a0, bound, took, None if acc_emu is None else acc_emu[2 * j + i], out)
        out["outcome"]["A%d" % i].append(took)
    return out


def check_sigma(c, rss, g, gtol, s2_dev, hyp):
    """sigma^2 = (rss / 2 + beta_0) / g from the device's "rss" and the variate: dict(worst, fails)"""
    ref = (LD(float(rss)) / 2 + LD(hyp["beta_0"])) / LD(float(g))
    bound = (G_SIGMA * 4 * U * (abs(LD(float(rss))) / 2 + LD(hyp["beta_0"])) / abs(LD(float(g)))) + abs(ref) * float(gtol) / float(g)
    r = _ratio(abs(LD(float(s2_dev)) - ref), bound)
    return dict(worst=r, fails=[] if r <= 1.0 else [f"{c.name}: the sweep's sigma^2 draw: {float(s2_dev)!r}, reference {float(ref)!r}, error / bound {r:.3g}"])


def reference_iteration(c, st, Z, nu, Phi, hyp, dims, mask=SEVEN, q=0, it=0, seed=SEED, rss=None, pcz=False):
    """one iteration of the scalar jobs in longdouble from the keyed variates alone, every step from the reference's own earlier
    steps: dict(pi, alpha_3, delta, A, gamma, tau, sigma_sq (with rss), outcome, margins)"""
    K = c.K
    S = np.log(_ld(Z).reshape(c.n, K)).sum(axis=0)
    pi_old, a3 = np.asarray(st["pi"], dtype=np.float64).ravel(), float(np.ravel(st["alpha_3"])[0])
    dr = pi_draws(c, pi_old, a3, hyp, q, it, seed)
    out = dict(outcome={}, pi=pi_old.copy(), alpha_3=a3)
    if mask & U_PI:
        a0 = acc_pi(c, pi_old, dr["pi_new"], a3, S, hyp)[0]
        out["outcome"]["pi"] = bool(dr["lu"][0] < a0)
        if out["outcome"]["pi"]:
            out["pi"] = np.asarray(dr["pi_new"], dtype=np.float64)
    if mask & U_ALPHA3:
        a0 = acc_a3(c, out["pi"], a3, dr["ph"], S, hyp)[0]
        out["outcome"]["alpha_3"] = bool(dr["lu"][1] < a0)
        if out["outcome"]["alpha_3"]:
            out["alpha_3"] = dr["ph"]
    var = variates(c, st["A"], hyp, dims, q, it, seed)
    ref = hyper_ref(c, st, nu, Phi, var["g"], hyp, mask, pcz)
    for nm in ("delta", "gamma", "tau"):
        out[nm] = np.asarray(ref[nm], dtype=np.float64) if nm in ref else np.asarray(st[nm], dtype=np.float64)
    A = np.array(st["A"], dtype=np.float64).reshape(K, 2)
    if (mask & U_A) and not pcz:
        out["outcome"]["A0"], out["outcome"]["A1"] = [], []
        for r in a_cells(c, st["A"], out["delta"], var, hyp):
            took = bool(r["logu"] < r["acc"](r["na"])[0])
            out["outcome"]["A%d" % r["cell"][1]].append(took)
            if took:
                A[r["cell"]] = r["na"]
    out["A"] = A
    if rss is not None and (mask & U_SIGMA):
        out["sigma_sq"] = float((LD(float(rss)) / 2 + LD(hyp["beta_0"])) / LD(var["g"][gstd_layout(c)["sigma"][0]]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulations
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # name: (case, which check must reject it)
    "delta_old_prefix": ("cubic_P30", "delta"),
    "gamma_old_tilde_tau": ("cubic_P30", "gamma"),
    "a2_sum_from_0": ("cubic_P30", "A"),
    "lB_row_stale": ("cubic_P30-reject", "alpha_3"),
    "pi_prop_swapped": ("cubic_P30", "pi"),
    "tau_mv_not_inverted": ("mv_P7", "tau"),
    "tau_shape_real_div": ("mv_P7", "gstd"),
    "skm_tail_dropped": ("quint_P27_K5M8", "delta"),
    "gamma_tail_dropped": ("quint_P27_K5M8", "gamma"),
    "penalty_row_clipped": ("wide_5x6", "tau"),      # (mid_5x5's penalty has band 5 = BWMAX: nothing to clip)
    "sigma_half_sum_real": ("cubic_P30", "gstd"),
}


def lgamma_pos64(x):
    """csrc/rng.hpp: lgamma_pos in float64"""
    x, prod = float(x), 1.0
    for _ in range(8):
        if x < 8.0:
            prod, x = prod * x, x + 1.0
    r = 1.0 / x
    r2 = r * r
    ser = 1.0 / 156.0
    for cf in (-691.0 / 360360.0, 1.0 / 1188.0, -1.0 / 1680.0, 1.0 / 1260.0, -1.0 / 360.0, 1.0 / 12.0):
        ser = ser * r2 + cf
    return (x - 0.5) * math.log(x) - x + 0.91893853320467274178 + ser * r - math.log(prod)


def _tree(v):
    v = list(v) + [0.0] * (256 - len(v))
    o = 128
    while o:
        v = [v[t] + v[t + o] for t in range(o)]
        o //= 2
    return v[0]


def emulate(c, st, Z, nu, Phi, gstd, hyp, mask, rss, variant="kernel", mut=None, q=0, it=0, seed=SEED, pcz=False):
    """one iteration of the scalar jobs in float64 from the variates gstd (keyed: pi / alpha_3 draws their own): dict(pi, alpha_3,
    acc (2), delta, gamma, tau, A, acc_A (2K), sigma_sq)"""
    K, P, M, n = c.K, c.P, c.M, c.n
    kern = variant == "kernel"
    lay = gstd_layout(c)
    g = np.asarray(gstd, dtype=np.float64)
    lgam = lgamma_pos64 if kern else math.lgamma
    Z = np.asarray(Z, dtype=np.float64).reshape(n, K)
    if kern:
        parts = [[sum(math.log(z) for z in Z[b * c.GPB:(b + 1) * c.GPB, k]) for b in range(c.nblk)] for k in range(K)]
        S = np.array([_tree(p) for p in parts])
    else:
        S = np.log(Z).sum(axis=0)
    pi_old, a3 = np.asarray(st["pi"], dtype=np.float64).ravel(), float(np.ravel(st["alpha_3"])[0])
    dr = pi_draws(c, pi_old, a3, hyp, q, it, seed)
    gs = dr["g"]
    pn = gs / (sum(gs) if kern else gs.sum())
    ap, cv = hyp["a_pi_PM"], hyp["c"]

    def lB(v):
        return sum(lgam(x) for x in v) - lgam(sum(v))

    out = dict(pi=pi_old.copy(), alpha_3=a3, acc=[np.nan, np.nan])
    pi_is_new = False
    if mask & U_PI:
        lo, ln = np.log(pi_old), np.log(pn)
        ln_, lo_, p_n, p_o = 0.0, 0.0, 0.0, 0.0
        for k in range(K):
            ln_ += (cv[k] - 1) * ln[k] + ((a3 * pn[k]) - 1) * S[k]
            lo_ += (cv[k] - 1) * lo[k] + ((a3 * pi_old[k]) - 1) * S[k]
            p_n += (ap * pi_old[k] - 1) * ln[k]
            p_o += (ap * pn[k] - 1) * lo[k]
        ln_ -= n * lB(a3 * pn)
        lo_ -= n * lB(a3 * pi_old)
        lpn, lpo = p_n - lB(ap * pi_old), p_o - lB(ap * pn)
        if mut == "pi_prop_swapped":
            lpn, lpo = lpo, lpn
        acc = ln_ - lo_ + lpo - lpn
        out["acc"][0] = acc
        if float(dr["lu"][0]) < acc:
            out["pi"], pi_is_new = pn.copy(), True
    if mask & U_ALPHA3:
        pi, ph, sd = out["pi"], dr["ph"], hyp["var_alpha3"]
        pb = pi_old if (mut == "lB_row_stale" and pi_is_new) else pi
        l_old, l_new = (-hyp["b"]) * a3, (-hyp["b"]) * ph
        for k in range(K):
            l_old += ((a3 * pi[k]) - 1) * S[k]
            l_new += ((ph * pi[k]) - 1) * S[k]
        l_old -= n * lB(a3 * pb)
        l_new -= n * lB(ph * pb)
        dtr = lambda m: -0.91893853320467274178 - math.log(sd) - math.log(pnorm(m / sd))      # noqa: E731
        l_old += dtr(ph)
        l_new += dtr(a3)
        out["acc"][1] = l_new - l_old
        if float(dr["lu"][1]) < l_new - l_old:
            out["alpha_3"] = ph
    # ---- delta, gamma, tau, A ----
    phi_on = not pcz
    Phi = np.asarray(Phi, dtype=np.float64).reshape(K, P, M)
    gam_old = np.asarray(st["gamma"], dtype=np.float64).reshape(K, P, M)
    d_old = np.asarray(st["delta"], dtype=np.float64).reshape(K, M)
    dl = d_old.copy()
    if (mask & U_DELTA) and phi_on:
        S2 = np.zeros((K, M))
        for k in range(K):
            for m in range(M):
                if mut == "skm_tail_dropped" and k * M + m >= 32:
                    continue
                pr = gam_old[k, :, m] * (Phi[k, :, m] * Phi[k, :, m])
                if kern:
                    a = [0.0] * 8
                    for lane in range(8):
                        for u in range(8):
                            a[lane] += pr[lane + 8 * u] if lane + 8 * u < P else 0.0
                    S2[k, m] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[7] + a[6]) + (a[5] + a[4]))
                else:
                    S2[k, m] = pr.sum()
        gd = g[slice(*lay["delta"])].reshape(K, M)
        for k in range(K):
            dv = d_old[k].copy()
            pre = 1.0
            for i in range(M):
                if kern:
                    tt = pre
                    p2 = 1.0 + 0.5 * tt * S2[k, i]
                    for m in range(i + 1, M):
                        tt *= dv[m]
                        p2 += 0.5 * tt * S2[k, m]
                    new = gd[k, i] * (1.0 / p2)
                    pre *= d_old[k, i] if mut == "delta_old_prefix" else new
                else:
                    src = d_old[k] if mut == "delta_old_prefix" else dv
                    p2 = 1.0 + sum(np.prod([(src[nn] if nn < i else dv[nn]) for nn in range(m + 1) if nn != i]) * S2[k, m] / 2 for m in range(i, M))
                    new = gd[k, i] / p2
                dv[i] = new
            dl[k] = dv
    out["delta"] = dl
    gam = gam_old.copy()
    if (mask & U_GAMMA) and phi_on:
        dsrc = d_old if mut == "gamma_old_tilde_tau" else dl
        gG = g[slice(*lay["gamma"])].reshape(K, P, M)
        for k in range(K):
            tt = 1.0
            for m in range(M):
                tt = tt * dsrc[k, m] if kern else float(np.prod(dsrc[k, :m + 1]))
                for p in range(P):
                    if mut == "gamma_tail_dropped" and (k * P + p) * M + m >= 768:
                        continue
                    gam[k, p, m] = gG[k, p, m] * (2 / (hyp["nu_1"] + tt * (Phi[k, p, m] * Phi[k, p, m])))
    out["gamma"] = gam
    tau = np.asarray(st["tau"], dtype=np.float64).ravel().copy()
    if mask & U_TAU:
        nv = np.asarray(nu, dtype=np.float64).reshape(K, P)
        Pm = penalty(c, np.float64)
        bw = c.BWP if not (mut == "penalty_row_clipped" and c.BWP > BWMAX) else BWMAX
        for k in range(K):
            if c.kind == "mv":
                qf = sum(nv[k, p] * nv[k, p] for p in range(P)) if kern else float(nv[k] @ nv[k])
            elif kern:
                qf = 0.0
                for p in range(P):
                    s = 0.0
                    rng_q = range(P) if (c.BWP > BWMAX and bw > BWMAX) else range(max(0, p - bw), min(P, p + bw + 1))
                    for qq in rng_q:
                        s += Pm[p, qq] * nv[k, qq]
                    qf += nv[k, p] * s
            else:
                Pq = Pm if bw == c.BWP else np.triu(np.tril(Pm, bw), -bw)
                qf = float(nv[k] @ (Pq @ nv[k]))
            gT = g[lay["tau"][0] + k]
            gg = gT * (1.0 / (hyp["beta_nu"] + 0.5 * qf)) if kern else gT / (hyp["beta_nu"] + qf / 2)
            tau[k] = gg if (c.kind != "mv" or mut == "tau_mv_not_inverted") else 1.0 / gg
    out["tau"] = tau
    A = np.array(st["A"], dtype=np.float64).reshape(K, 2)
    out["acc_A"] = np.full(2 * K, np.nan)
    if (mask & U_A) and phi_on:
        lgd = np.log(dl)
        tg = (lambda a: math.log(math.gamma(a))) if kern else math.lgamma
        for j in range(K):
            for i in range(2):
                cell, cur, sd = 2 * j + i, float(A[j, i]), a_sd(hyp, i)
                na, un = g[lay["aprop"][0] + cell], g[lay["aunif"][0] + cell]
                w = []
                for a in (cur, na):
                    if i == 0:
                        w.append(-tg(a) + (a - 1) * lgd[j, 0] + (hyp["alpha1l"] - 1) * math.log(a) - (a * hyp["beta1l"]))
                    else:
                        sl = sum(lgd[j, (0 if mut == "a2_sum_from_0" else 1):]) if kern else float(lgd[j, (0 if mut == "a2_sum_from_0" else 1):].sum())
                        w.append(-(M - 1.0) * tg(a) + (hyp["alpha2l"] - 1) * math.log(a) - (a * hyp["beta2l"]) + (a - 1) * sl)
                dt = lambda x, mu: -0.91893853320467274178 - math.log(sd) - 0.5 * ((x - mu) / sd) ** 2 - math.log(pnorm(mu / sd))      # noqa: E731
                acc = (w[1] + dt(cur, na)) - w[0] - dt(na, cur)
                out["acc_A"][cell] = acc
                if math.log(un) < acc:
                    A[j, i] = na
    out["A"] = A
    if mask & U_SIGMA:
        sg = g[lay["sigma"][0]]
        b = 0.5 * rss + hyp["beta_0"]
        out["sigma_sq"] = 1.0 / (sg * (1.0 / b)) if kern else b / sg
    return out
