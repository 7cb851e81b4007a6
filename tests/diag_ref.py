"""numpy restatement of the convergence diagnostics of DESIGN.md 7c (split R-hat, bulk / tail ESS, MCSE of the mean after
Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021), the yardstick of k_diag.  A helper, not a test module.

A row is one scalar parameter: x[c][s], chains c < C, draws s < S."""
import math

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

EPS = 2.0 ** -52
STATS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")


def split(x):
    """(C, S) -> (2C, h) sequences: the first h and the last h draws of every chain (the middle draw of an odd S dropped)"""
    x = np.asarray(x, dtype=np.float64)
    C, S = x.shape
    h = S // 2
    out = np.empty((2 * C, h))
    out[0::2] = x[:, :h]
    out[1::2] = x[:, S - h:]
    return out


def degenerate(v):
    v = np.asarray(v, dtype=np.float64)
    return v.size == 0 or not np.all(np.isfinite(v)) or float(np.max(v) - np.min(v)) < EPS


def z_scale(y):
    """rank normalisation of the whole set, average ranks for ties, (r - 3/8) / (N + 1/4)"""
    r = rankdata(y, method="average").reshape(y.shape)
    return ndtri((r - 0.375) / (y.size + 0.25))


def quantile7(v, p):
    """type-7 quantile of a sorted array: linear between v[floor(g)] and v[floor(g) + 1], g = (N - 1) p"""
    g = (len(v) - 1) * p
    lo = int(math.floor(g))
    if lo + 1 >= len(v):
        return float(v[lo])
    return float(v[lo] + (g - lo) * (v[lo + 1] - v[lo]))


def rhat_seq(y):
    """R-hat of m sequences (rows) of length n >= 2; NaN on a degenerate set"""
    m, n = y.shape
    if n < 2 or degenerate(y):
        return math.nan
    B = n * np.var(np.mean(y, axis=1), ddof=1) if m > 1 else 0.0
    W = np.mean(np.var(y, axis=1, ddof=1))
    return math.sqrt((B / W + n - 1) / n)


def ess_seq(y, trace=None):
    """ESS of m sequences (rows) of length n >= 3 (Geyer's initial monotone sequence); NaN on a degenerate set.  `trace`, a
    dict, receives the stop lag and |e + o| there (the truncation decision)."""
    m, n = y.shape
    if n < 3 or degenerate(y):
        return math.nan
    mu = np.mean(y, axis=1)
    yc = y - mu[:, None]

    def gamma(t):
        return np.mean(np.sum(yc[:, :n - t] * yc[:, t:], axis=1) / n)

    W = n / (n - 1) * gamma(0)
    var_plus = (n - 1) / n * W + (np.var(mu, ddof=1) if m > 1 else 0.0)

    def rho(t):      # (only the lags the truncation reaches are computed)
        return 1.0 - (W - gamma(t)) / var_plus

    rh = np.zeros(n)
    rh[0] = 1.0
    rh[1] = rho(1)
    t, e, o = 0, 1.0, rh[1]
    while t < n - 5 and e + o > 0:
        t += 2
        e, o = rho(t), rho(t + 1)
        if e + o >= 0:
            rh[t], rh[t + 1] = e, o
    max_t = t
    if e > 0:
        rh[max_t] = e
    if trace is not None:
        trace["stop"] = max_t
        trace["margin"] = abs(e + o)
        trace["hit_end"] = not (t < n - 5)
    t = 0
    while t <= max_t - 4:
        t += 2
        if rh[t] + rh[t + 1] > rh[t - 2] + rh[t - 1]:
            rh[t] = rh[t + 1] = (rh[t - 2] + rh[t - 1]) / 2
    tau = -1.0 + 2.0 * np.sum(rh[:max_t]) + rh[max_t]
    cap = 1.0 / math.log10(m * n)
    if tau < cap:
        tau = cap
    return m * n / tau


def diag_row(x, traces=None):
    """the seven statistics of one row x (C, S); `traces`, a dict, receives the ESS truncation traces by set name"""
    x = np.asarray(x, dtype=np.float64)
    C, S = x.shape
    N = C * S
    flat = x.reshape(-1)
    mean = float(np.mean(flat))
    sd = float(math.sqrt(np.sum((flat - mean) ** 2) / (N - 1))) if N > 1 else math.nan
    out = dict(rhat=math.nan, ess_bulk=math.nan, ess_tail=math.nan, ess_mean=math.nan, mean=mean, sd=sd)
    xs = split(x)
    h = xs.shape[1]
    if h >= 1 and not degenerate(xs):
        v = np.sort(xs.reshape(-1))
        med = quantile7(v, 0.5)
        z = z_scale(xs)
        zf = z_scale(np.abs(xs - med))
        if h >= 2:
            rb, rf = rhat_seq(z), rhat_seq(zf)
            out["rhat"] = math.nan if (math.isnan(rb) or math.isnan(rf)) else max(rb, rf)
        tr = {k: {} for k in ("bulk", "mean", "q05", "q95")}
        out["ess_bulk"] = ess_seq(z, tr["bulk"])
        out["ess_mean"] = ess_seq(xs, tr["mean"])
        e05 = ess_seq((xs <= quantile7(v, 0.05)).astype(np.float64), tr["q05"])
        e95 = ess_seq((xs <= quantile7(v, 0.95)).astype(np.float64), tr["q95"])
        out["ess_tail"] = math.nan if (math.isnan(e05) or math.isnan(e95)) else min(e05, e95)
        if traces is not None:
            traces.update(tr)
    out["mcse_mean"] = sd / math.sqrt(out["ess_mean"])
    return out


def diagnostics(draws, traces=None):
    """draws (S, C) or (S, C, *shape) -> dict of the seven statistics, each of shape `shape` (the layout api.diagnostics
    takes); `traces`, a list, receives one trace dict per row in row order"""
    d = np.asarray(draws, dtype=np.float64)
    if d.ndim < 2:
        raise ValueError("draws must be (S, C) or (S, C, *shape)")
    S, C = d.shape[:2]
    shape = d.shape[2:]
    rows = d.reshape(S, C, -1)
    res = {k: np.empty(rows.shape[2]) for k in STATS}
    for p in range(rows.shape[2]):
        tr = {}
        r = diag_row(rows[:, :, p].T, tr)
        if traces is not None:
            traces.append(tr)
        for k in STATS:
            res[k][p] = r[k]
    return {k: v.reshape(shape) for k, v in res.items()}
