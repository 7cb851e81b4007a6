"""numpy restatement, in long double, of the contrasts of cluster mean functions and covariate effects (DESIGN.md 7t;
kernels_cluster_contrast.hip).  For one draw with label map A (K, K), nu (K, P), eta (P, D, K) in get_chain's layout without the
slot axis, contrast weights w_nu (R, K), w_eta (R, K, D) and the grid basis E (G, P):

    a[r, c]   = sum_k w_nu[r, k] A[k, c]              a'[r, c, d] = sum_k w_eta[r, k, d] A[k, c]
    b[r, p]   = sum_c ( a[r, c] nu[c, p] + sum_d a'[r, c, d] eta[p, d, c] )
    v[r, g]   = sum_p E[g, p] b[r, p]
    abar      = the same three sums with every factor replaced by its absolute value

Forward error of a device value, u = 2^-52 (the project's convention: twice the unit roundoff, which pays for the restatement's own
rounding and for the second-order terms).  A term w_k A_kc nu_cp E_gp of v (or its eta sibling) is rounded along one path: its own
product and at most K additions inside a_c, the product a_c nu, at most K (1 + D) additions inside b_r[p], the product E_gp b_r[p],
at most P additions over p: n = P + K (D + 2) + 3 roundings of at most u / 2 each, so to first order |device - exact| <= (n / 2) u abar,
and the bound held is about twice that,
    b = (P + K (D + 2) + 2) u abar          (K for a_c, one product, K (1 + D) additions, one product, P additions)
The shipped order (k, then c with its d, then p, each from 0.0, one rounding per product and per sum) is the one counted; b is
derived, not tuned.

Over the N pooled draws V (..., N), as the device reduces them:
    prob_positive = #{v > 0} / N                       dev[r, cs] = max_g |v - mean| / sd   (sd = 0 skipped, from 0.0; NaN kept)
    crit[r]       = the (1 - alpha) quantile of dev[r] (Hyndman and Fan 5, curve_fit_ref.quantiles)
    band          = mean -/+ crit sd                    t[r] = max over g with sd > 0 of |mean| / sd   (0 where there is none)
    p_sim[r]      = #{cs : dev[r, cs] >= t[r]} / N      norm[r, cs] = sqrt(sum_g w_g v[r, g, cs]^2)
p_sim and the band: the band at level alpha excludes zero at g where |mean_g| > crit sd_g, so somewhere where t > crit.  Let m =
#{dev >= t}.  Where alpha N = i + 1/2 for an integer i, definition 5 puts the (1 - alpha) quantile on the order statistic x_(N - i)
itself, and without ties t > x_(N - i) holds exactly where at most i of the dev are >= t: m <= i, which is m / N < alpha.  At other
levels crit lies between two order statistics and the two statements can differ for a t between them: p_sim is the level of the
band up to that interpolation, 1 / N."""
import numpy as np

import curve_fit_ref as FR

LD = np.longdouble
U = 2.0 ** -52


def perm_matrix(perm):
    """A[k, c] = 1 where c = perm[k]"""
    perm = np.asarray(perm)
    return (perm[..., None] == np.arange(perm.shape[-1])).astype(np.float64)


def coef(A, w_nu, w_eta=None, absolute=False):
    """a (R, K) and a' (R, K, D) (None without w_eta) of one draw"""
    f = (lambda x: np.abs(np.asarray(x, dtype=LD))) if absolute else (lambda x: np.asarray(x, dtype=LD))
    A = f(A)
    a = f(w_nu) @ A                                                          # [r, c] = sum_k w[r, k] A[k, c]
    ad = None if w_eta is None else np.einsum("rkd,kc->rcd", f(w_eta), A)
    return a, ad


def values(E, nu, A, w_nu, eta=None, w_eta=None, absolute=False):
    """v (R, G) of one draw in long double; absolute: abar"""
    f = (lambda x: np.abs(np.asarray(x, dtype=LD))) if absolute else (lambda x: np.asarray(x, dtype=LD))
    a, ad = coef(A, w_nu, w_eta, absolute)
    b = a @ f(nu)                                                            # (R, P)
    if w_eta is not None:
        b = b + np.einsum("rcd,pdc->rp", ad, f(eta))
    return b @ f(E).T


def bound_count(P, K, D):
    return P + K * (D + 2) + 2


def pooled(chains, E, mix, w_nu, w_eta, first, S):
    """(v, abar), each (R, G, N) in long double, N = C S draws chain-major: the trace the call returns and what its bound scales with"""
    v, a = [], []
    for q, ch in enumerate(chains):
        for s in range(S):
            nu = ch["nu"][..., first + s]
            eta = ch["eta"][..., first + s] if w_eta is not None else None
            v.append(values(E, nu, mix[q, s], w_nu, eta, w_eta))
            a.append(values(E, nu, mix[q, s], w_nu, eta, w_eta, absolute=True))
    return np.stack(v, axis=-1), np.stack(a, axis=-1)


def prob_positive(V):
    V = np.asarray(V)
    return np.sum(V > 0, axis=-1) / float(V.shape[-1])


def dev(V, mean, sd):
    """(R, N): the largest standardised deviation over the grid (axis 1) of every draw"""
    V, mean, sd = (np.asarray(x, dtype=np.float64) for x in (V, mean, sd))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs((V - mean[..., None]) / sd[..., None])
    d = np.where((sd != 0.0)[..., None], d, 0.0)
    return np.maximum(d.max(axis=1), 0.0)


def crit(dv, alpha):
    return FR.quantiles(dv, (1.0 - float(alpha),))[..., 0]


def band(mean, sd, cr):
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    return mean - cr[..., None] * sd, mean + cr[..., None] * sd


def threshold(mean, sd):
    """t (R,)"""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(sd > 0.0, np.abs(mean) / sd, 0.0)
    return t.max(axis=-1)


def p_sim(dv, t):
    dv = np.asarray(dv)
    return np.sum(dv >= np.asarray(t)[..., None], axis=-1) / float(dv.shape[-1])


def norm(V, w=None):
    """(R, N) in the dtype of V: sqrt(sum_g w_g v^2), w (G,) (default 1 / G)"""
    V = np.asarray(V)
    G = V.shape[1]
    w = np.full(G, 1.0 / G) if w is None else np.asarray(w)
    return np.sqrt(np.einsum("g,rgn->rn", w.astype(V.dtype), V * V))


def summary(V, alpha=None, w=None):
    """everything the call pools from the values V (R, G, N), in float64 with numpy's moments"""
    V = np.asarray(V, dtype=np.float64)
    mean, sd = FR.moments(V)
    out = {"mean": mean, "sd": sd, "prob_positive": prob_positive(V), "norm": norm(V, w)}
    if alpha is not None:
        dv = dev(V, mean, sd)
        cr = crit(dv, alpha)
        lo, up = band(mean, sd, cr)
        out.update(dev=dv, crit=cr, lower=lo, upper=up, excludes_zero=(lo > 0) | (up < 0), p_sim=p_sim(dv, threshold(mean, sd)))
    return out
