"""numpy restatement of the PSIS-LOO / WAIC steps of DESIGN.md 7b (loo's psis() / gpdfit() with relative efficiency 1), the
yardstick of k_post_psis.  A helper, not a test module."""
import math
import sys

import numpy as np


def _lse(x):
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m)))


def gpdfit(e):
    """generalized Pareto fit of the ascending exceedances e (steps under 4): (k_hat, sigma), k_hat with the prior"""
    N = len(e)
    m = 30 + int(math.floor(math.sqrt(N)))
    xstar = e[int(math.floor(N / 4 + 0.5)) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    theta = 1.0 / e[N - 1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * xstar)
    with np.errstate(all="ignore"):
        kappa = np.array([np.mean(np.log1p(-t * e)) for t in theta])
        lth = N * (np.log(-theta / kappa) - kappa - 1.0)
        w = np.exp(lth - _lse(lth))
        th = np.sum(w * theta)
        k = np.mean(np.log1p(-th * e))
        sigma = -k / th
        khat = (N * k + 5.0) / (N + 10.0)
    if math.isnan(khat):
        khat = math.inf
    return khat, sigma


def psis_row(ll):
    """steps 1-6 on one row: dict of lppd, elpd_loo, p_loo, pareto_k, elpd_waic, p_waic, and lw (the final log weights)"""
    ll = np.asarray(ll, dtype=np.float64)
    S = len(ll)
    lppd = _lse(ll) - math.log(S)
    mean = np.mean(ll)
    p_waic = float(np.sum((ll - mean) ** 2) / (S - 1)) if S > 1 else 0.0
    r = -ll
    lw = r - np.max(r)
    L = int(math.ceil(min(0.2 * S, 3 * math.sqrt(S))))
    khat = math.inf
    if L >= 5:
        order = np.argsort(lw, kind="stable")            # ties by draw index
        tail_ix = order[S - L:]
        x = lw[tail_ix]
        c = lw[order[S - L - 1]]
        if not (x[-1] - x[0] < sys.float_info.epsilon / 100):
            with np.errstate(all="ignore"):
                e = np.exp(x) - np.exp(c)
            khat, sigma = gpdfit(e)
            if math.isfinite(khat):
                p = (np.arange(1, L + 1) - 0.5) / L
                with np.errstate(all="ignore"):
                    lw = lw.copy()
                    lw[tail_ix] = np.log(sigma * np.expm1(-khat * np.log1p(-p)) / khat + np.exp(c))
    lw = np.minimum(lw, 0.0)
    elpd = _lse(lw + ll) - _lse(lw)
    return dict(lppd=lppd, elpd_loo=elpd, p_loo=lppd - elpd, pareto_k=khat, elpd_waic=lppd - p_waic, p_waic=p_waic, lw=lw)


def _total_se(v):
    s = 0.0
    for x in v:                                          # curve order
        s += float(x)
    n = len(v)
    if n < 2:
        return s, math.nan
    mean = s / n
    q = 0.0
    for x in v:
        q += (float(x) - mean) ** 2
    return s, math.sqrt(n * (q / (n - 1)))


def psis_loo(ll):
    """every row of an n x S matrix and the totals, keyed as FLOO returns them"""
    ll = np.atleast_2d(np.asarray(ll, dtype=np.float64))
    n, S = ll.shape
    rows = [psis_row(r) for r in ll]
    pw = {"lppd": np.array([r["lppd"] for r in rows]), "pointwise_elpd_loo": np.array([r["elpd_loo"] for r in rows]),
          "pointwise_p_loo": np.array([r["p_loo"] for r in rows]), "pareto_k": np.array([r["pareto_k"] for r in rows]),
          "pointwise_elpd_waic": np.array([r["elpd_waic"] for r in rows]), "pointwise_p_waic": np.array([r["p_waic"] for r in rows])}
    e_loo, se_loo = _total_se(pw["pointwise_elpd_loo"])
    p_loo, se_ploo = _total_se(pw["pointwise_p_loo"])
    e_waic, se_ewaic = _total_se(pw["pointwise_elpd_waic"])
    p_waic, se_pwaic = _total_se(pw["pointwise_p_waic"])
    with np.errstate(divide="ignore"):
        thr = float(min(1.0 - 1.0 / np.log10(float(S)), 0.7))
    out = dict(elpd_loo=e_loo, se_elpd_loo=se_loo, p_loo=p_loo, se_p_loo=se_ploo, looic=-2 * e_loo, se_looic=2 * se_loo,
               elpd_waic=e_waic, se_elpd_waic=se_ewaic, p_waic=p_waic, se_p_waic=se_pwaic, waic=-2 * e_waic, se_waic=2 * se_ewaic,
               khat_threshold=thr, n_khat_above=int(np.sum(pw["pareto_k"] > thr)))
    out.update(pw)
    return out
