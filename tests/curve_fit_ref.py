"""numpy restatement of the pooled per-curve fitted functions of chain slots (kernels_curve_fit.hip):

    c_i   = sum_k Z_ik (nu_k + sum_d x_id eta_kd)
    V_im  = sum_k Z_ik (phi_km + sum_d x_id xi_kmd)        (xi only when covariance-adjusted)
    mean_i(g) = E_g . c_i,        fit_i(g) = E_g . (c_i + sum_m chi_im V_im)

from get_chain copies (nu (K, P, T), Phi (K, P, M, T), Z (n, K, T), chi (n, M, T), eta (P, D, K, T), xi (P, D, M, K, T)), the
quantile rule of k_bands_quantiles, and the forward error bound of a value.  The bound is derived, not measured: a value is a
sum of N_t = P K (M + 1) (1 + D) products, whose computed value in any order is within N_t u A (u = 2^-53, to first order) of
the exact one, A being the same expression with every factor replaced by its absolute value; doubled for the reference's own
rounding, and written with 2^-52 for u: 2 N_t 2^-52 A."""
import numpy as np


def draw_values(E, Z, chi, nu, Phi, which, X=None, eta=None, xi=None, covariance_adj=False, dtype=np.float64, absolute=False):
    """(n, G, S) values of S draws: Z (n, K, S), chi (n, M, S), nu (K, P, S), Phi (K, P, M, S), eta (P, D, K, S), xi (P, D, M, K, S).
    which: "mean" or "fit".  absolute: every factor replaced by its absolute value (the A of `bound`)."""
    f = (lambda a: np.abs(np.asarray(a, dtype=dtype))) if absolute else (lambda a: np.asarray(a, dtype=dtype))
    E, Z, nu = f(E), f(Z), f(nu)
    c = np.einsum("iks,kps->ips", Z, nu)
    if X is not None:
        X, eta = f(X), f(eta)
        c = c + np.einsum("iks,id,pdks->ips", Z, X, eta)
    if which == "fit":
        chi, Phi = f(chi), f(Phi)
        c = c + np.einsum("ims,iks,kpms->ips", chi, Z, Phi)
        if X is not None and covariance_adj:
            c = c + np.einsum("ims,iks,id,pdmks->ips", chi, Z, X, f(xi))
    elif which != "mean":
        raise ValueError(which)
    return np.einsum("gp,ips->igs", E, c)


def n_terms(P, K, M, D):
    return P * K * (M + 1) * (1 + D)


def _pooled(chains, E, which, first, n_slots, X, covariance_adj, curves, absolute):
    sl = slice(first, first + n_slots)
    idx = slice(None) if curves is None else np.asarray(curves, dtype=np.int64)
    out = []
    for ch in chains:
        kw = {}
        if X is not None:
            kw = dict(X=np.asarray(X)[idx], eta=ch["eta"][..., sl], xi=ch["xi"][..., sl], covariance_adj=covariance_adj)
        out.append(draw_values(E, ch["Z"][idx][..., sl], ch["chi"][idx][..., sl], ch["nu"][..., sl], ch["Phi"][..., sl], which,
                               absolute=absolute, **kw))
    return np.stack(out, axis=2)          # (m, G, C, S)


def values(chains, E, which, first, n_slots, X=None, covariance_adj=False, curves=None):
    """what Sampler.curve_fit returns, from the get_chain copies of every chain: (m, G, C, S)"""
    return _pooled(chains, E, which, first, n_slots, X, covariance_adj, curves, False)


def bound(chains, E, which, first, n_slots, X=None, covariance_adj=False, curves=None):
    """2 N_t 2^-52 A for every entry of `values`"""
    ch = chains[0]
    K, P, M = ch["Phi"].shape[:3]
    D = 0 if X is None else np.asarray(X).shape[1]
    return 2.0 * n_terms(P, K, M, D) * 2.0 ** -52 * _pooled(chains, E, which, first, n_slots, X, covariance_adj, curves, True)


def quantiles(v, probs):
    """k_bands_quantiles' rule (arma::quantile; Hyndman and Fan definition 5) along the last axis of v: (..., nq)"""
    s = np.sort(np.asarray(v, dtype=np.float64), axis=-1)
    T = s.shape[-1]
    N = float(T)
    out = np.empty(s.shape[:-1] + (len(probs),))
    for q, p in enumerate(probs):
        p = float(p)
        if p < 0.5 / N:
            out[..., q] = s[..., 0]
        elif p > (N - 0.5) / N:
            out[..., q] = s[..., T - 1]
        else:
            k = int(np.floor(N * p + 0.5))
            pk = (float(k) - 0.5) / N
            w = (p - pk) * N
            out[..., q] = (1.0 - w) * s[..., k - 1] + w * s[..., min(k, T - 1)]
    return out


def moments(v):
    """numpy's mean and two-pass sd (N - 1; NaN for one draw) along the last axis"""
    v = np.asarray(v, dtype=np.float64)
    T = v.shape[-1]
    mean = v.mean(axis=-1)
    sd = np.full(mean.shape, np.nan) if T < 2 else v.std(axis=-1, ddof=1)
    return mean, sd
