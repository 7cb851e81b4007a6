"""numpy restatement of the marginal PSIS-LOO over curves on top of tests/predict_ref.py and tests/psis_ref.py: the
rule that selects the (curve, draw) pairs to refine and the order of their list, the refinement (the stages of predict_ref from a
starting proposal, so that the Dirichlet correction applies in stage 0 as well), the floor of that stage 0 in float64 against
np.longdouble, and the pipeline from the traces to PSIS."""
import math

import numpy as np

import predict_ref as R
import psis_ref


def selected(lpd, ess, ess_floor):
    """a pair is refined where its ess is below the floor or its lpd is not finite (a NaN ess alone selects nothing)"""
    lpd, ess = np.asarray(lpd, dtype=np.float64), np.asarray(ess, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (ess < ess_floor) | ~np.isfinite(lpd)


def select_list(lpd, ess, ess_floor):
    """(n_ref, 3) int32 rows (curve, chain, slot) of the selected pairs of (n, C, S) traces, in increasing (curve, chain, slot) order,
    and the (n,) counts per curve"""
    sel = selected(lpd, ess, ess_floor)
    return np.argwhere(sel).astype(np.int32), sel.reshape(sel.shape[0], -1).sum(axis=1).astype(np.int32)


def refine_stages(ell_fn, prior, start, J2, R2, sample):
    """R2 stages of J2 samples from the proposal `start`; sample(a, st) -> z (J2, K).  Returns the last stage's dict of
    predict_ref.stage with "z", "lw" and "proposals" (R2, K) added."""
    prior = np.asarray(prior, dtype=np.float64)
    a, props = np.asarray(start, dtype=np.float64), []
    for st in range(R2):
        props.append(a)
        z = np.maximum(sample(a, st), R.TINY)
        lw = R.log_weights(ell_fn(z), z, prior, a)          # the correction from stage 0 on
        out = R.stage(lw, z)
        a = out["next"]
    out.update(z=z, lw=lw, proposals=np.array(props))
    return out


def staged_then_refined(ell_fn, prior, J, R_, J2, R2, rng):
    """the first pass from the prior, then the refinement from its last proposal: (first, refined)"""
    first = R.staged_estimate(ell_fn, prior, J, R_, rng)
    refined = refine_stages(ell_fn, prior, first["proposals"][-1], J2, R2, lambda a, st: rng.dirichlet(a, size=J2))
    return first, refined


# ---- the floor of the refinement's stage 0 --------------------------------------------------------------------------------------
_LD = np.longdouble
_BERN = [(1, 12), (-1, 360), (1, 1260), (-1, 1680), (1, 1188), (-691, 360360), (1, 156), (-3617, 122400), (43867, 244188)]


def lgamma_ld(x):
    """log Gamma(x), x > 0, in np.longdouble: the recurrence up to x >= 40, then nine terms of the Stirling series (the first one left
    out is below 1e-30 there)"""
    x = _LD(x)
    shift = _LD(0.0)
    while x < 40:
        shift += np.log(x)
        x = x + _LD(1.0)
    r, r2 = _LD(1.0) / x, (_LD(1.0) / x) ** 2
    ser, p = _LD(0.0), r
    for num, den in _BERN:
        ser += _LD(num) / _LD(den) * p
        p = p * r2
    half_log_2pi = _LD(0.5) * np.log(_LD(2.0) * np.arccos(_LD(-1.0)))
    return (x - _LD(0.5)) * np.log(x) - x + half_log_2pi + ser - shift


def log_beta_ld(a):
    return sum(lgamma_ld(v) for v in a) - lgamma_ld(np.sum(np.asarray(a, dtype=_LD)))


def log_weights_ld(ell, z, prior, proposal):
    ell, z = np.asarray(ell).astype(_LD), np.asarray(z).astype(_LD)
    prior, proposal = np.asarray(prior).astype(_LD), np.asarray(proposal).astype(_LD)
    return ell + np.log(z) @ (prior - proposal) + (log_beta_ld(proposal) - log_beta_ld(prior))


def stage0_floor(cases=600, seed=22):
    """the worst |float64 - longdouble| / max(1, |longdouble|) over the log weights of a refinement's stage 0 (a proposal that is not
    the prior) and every output of the stage rule on them, over `cases` random inputs in the ranges of predict_ref.rule_floor: K in
    {2, 3, 8}, J in {37, 300}, prior and proposal a scale in {0.3, 1, 4, 60} times uniform(0.5, 2) entries (the proposal not below
    0.5, as the rule leaves it), z ~ Dir(proposal) clamped, l a scale in {0.1, 1, 5, 30} times a standard normal minus up to 50"""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for i in range(cases):
        K = int(rng.choice([2, 3, 8]))
        J = int(rng.choice([37, 300]))
        prior = rng.choice([0.3, 1.0, 4.0, 60.0]) * rng.uniform(0.5, 2.0, size=K)
        a = np.maximum(rng.choice([0.3, 1.0, 4.0, 60.0]) * rng.uniform(0.5, 2.0, size=K), 0.5)
        z = np.maximum(rng.dirichlet(a, size=J), R.TINY)
        ell = rng.choice([0.1, 1.0, 5.0, 30.0]) * rng.standard_normal(J) - 50.0 * rng.uniform()
        lw, lw_ld = R.log_weights(ell, z, prior, a), log_weights_ld(ell, z, prior, a)
        worst = max(worst, float(np.max(np.abs(lw.astype(_LD) - lw_ld) / np.maximum(1.0, np.abs(lw_ld)))))
        got, ref = R.stage(lw, z), R.stage(lw_ld, z, np.longdouble)
        for k in got:
            d = np.max(np.abs(np.asarray(got[k], dtype=_LD) - ref[k]) / np.maximum(1.0, np.abs(ref[k])))
            worst = max(worst, float(d))
    return worst


# ---- the K = 2 curve of the estimator check ---------------------------------------------------------------------------------------
def k2_case():
    """K = 2, M = 2, P = 6, the curve of tests/test_predict_ref.py's K = 2 check made longer and sharper: 20 points (uniform basis
    rows, generator seed 5), sigma^2 = 0.05, its mean at the memberships (0.7, 0.3), the prior alpha_3 pi = (2, 3) with its mass on
    the other side.  256 prior samples reach an ess of about 35 on it, the case the refinement is for.  (A sharper one -- 40 points,
    sigma^2 = 0.02, prior (1, 4) -- made the staged proposals of some seeds collapse short of the curve's mass, where the estimate's
    own standard error says nothing: the check would then test the seeds, not the rule.)  Returns l as a function of z (J, 2) and the prior."""
    rng = np.random.default_rng(5)
    K, M, P, n, sig = 2, 2, 6, 20, 0.05
    B = rng.uniform(0.0, 1.0, size=(n, P))
    th = R.directions(rng.standard_normal((K, P)), 0.4 * rng.standard_normal((K, P, M)))
    y = B @ (np.array([0.7, 0.3]) @ th[:, 0]) + math.sqrt(sig) * rng.standard_normal(n)
    G, s, yy, n = R.record(B, y)
    Gam, tau = R.gamma_tables(G, s, th)
    prior = np.array([2.0, 3.0])
    ell = lambda z: np.array([R.ell_gamma(Gam, tau, yy, n, zj, sig) for zj in z])
    return ell, prior


def k2_exact(ell, prior, nodes=400):
    """log of the integral of exp l(u, 1 - u) Beta(u; prior) du by Gauss-Legendre on `nodes` nodes"""
    x, w = np.polynomial.legendre.leggauss(nodes)
    u = 0.5 * (x + 1.0)
    lp = ell(np.stack([u, 1.0 - u], axis=1)) + (prior[0] - 1) * np.log(u) + (prior[1] - 1) * np.log1p(-u) - R.log_beta(prior)
    mx = lp.max()
    return mx + math.log(np.sum(0.5 * w * np.exp(lp - mx)))


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
def loo_from_traces(lpd_trace):
    """PSIS-LOO and WAIC of (n, C, S) traces with the chains pooled: psis_ref.psis_loo on the (n, C S) matrix"""
    lpd_trace = np.asarray(lpd_trace, dtype=np.float64)
    return psis_ref.psis_loo(lpd_trace.reshape(lpd_trace.shape[0], -1))
