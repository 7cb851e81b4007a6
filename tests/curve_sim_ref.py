"""numpy restatement of the simultaneous credible band of a curve's pooled draws (k_fit_sim in
kernels_curve_fit.hip), the reference's rule (FMeanCI's `simultaneous`) per curve with the chains pooled:

    C(cs)    = max over g with sd(g) != 0 of |(v(g, cs) - mean(g)) / sd(g)|, starting from 0.0
    crit     = the (1 - alpha) quantile of the N values C(.) by curve_fit_ref.quantiles' rule
    lower(g) = mean(g) - crit sd(g),        upper(g) = mean(g) + crit sd(g)

A grid point with sd exactly 0 is left out of the maximum (its band is its mean); crit is 0 where every sd is 0; for one draw
sd is NaN and so are crit, lower and upper (the maximum keeps a NaN)."""
import numpy as np

import curve_fit_ref as R


def sim_bands(vals, alpha, mean=None, sd=None):
    """vals (m, G, N): the values of m curves on G grid points under N draws.  mean, sd (m, G): the moments to standardise by
    (default: curve_fit_ref.moments).  Returns {"mean", "sd", "lower", "upper": (m, G), "crit": (m,), "C": (m, N)}."""
    vals = np.asarray(vals, dtype=np.float64)
    if mean is None or sd is None:
        mean, sd = R.moments(vals)
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.abs((vals - mean[..., None]) / sd[..., None])
    dev = np.where((sd != 0.0)[..., None], dev, 0.0)
    C = np.maximum(dev.max(axis=1), 0.0)              # np.max and np.maximum keep a NaN
    crit = R.quantiles(C, (1.0 - float(alpha),))[..., 0]
    return {"mean": mean, "sd": sd, "crit": crit, "C": C,
            "lower": mean - crit[..., None] * sd, "upper": mean + crit[..., None] * sd}
