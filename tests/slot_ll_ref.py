"""Long-double restatement of the log-likelihood given the scores, from the observations and independent of the
per-curve records: for curve i under a draw

    theta_i = sum_k Z_ik (nu_k + eta_k x_i) + sum_m chi_im sum_k Z_ik (phi_km + xi_km x_i)
    functional:    l_i = sum_l log dnorm(y_il; (B_i theta_i)_l, sqrt(sigma^2))
    multivariate:  l_i = -((P // 2) log(2 pi sigma^2)) - |y_i - theta_i|^2 / (2 sigma^2)    (CalculateLikelihood.h:155, an integer division)

and loglik = sum_i l_i.  `record_curve` is the fp64 record route of the kernel (G_i = B_i'B_i, s_i = B_i'y_i, yy_i) for the
CPU test that bounds what that route can lose against the dense form."""
import numpy as np

LD = np.longdouble
LOG_2PI = np.log(2 * np.arccos(LD(-1)))      # pi to the precision of long double


def theta(nu, Phi, Z, chi, X=None, eta=None, xi=None, dtype=LD):
    """(n, P): the coefficient vector of every curve under one draw.  nu (K, P), Phi (K, P, M), Z (n, K), chi (n, M), X (n, D), eta
    (P, D, K), xi (P, D, M, K) (None: not covariance-adjusted)."""
    nu, Phi, Z, chi = (np.asarray(a, dtype=dtype) for a in (nu, Phi, Z, chi))
    n, K = Z.shape
    M = chi.shape[1]
    mean = np.broadcast_to(nu[None], (n,) + nu.shape)
    Xl = None if X is None else np.asarray(X, dtype=dtype)
    if X is not None and eta is not None:
        mean = mean + np.einsum("pdk,id->ikp", np.asarray(eta, dtype=dtype), Xl)
    th = np.einsum("ik,ikp->ip", Z, mean)
    for m in range(M):
        ph = np.broadcast_to(Phi[None, :, :, m], (n,) + Phi.shape[:2])
        if X is not None and xi is not None:
            ph = ph + np.einsum("pdk,id->ikp", np.asarray(xi, dtype=dtype)[:, :, m, :], Xl)
        th = th + chi[:, m, None] * np.einsum("ik,ikp->ip", Z, ph)
    return th


def dense_curve(y, B, th, s2):
    """l_i from the observations; B None: the multivariate model (y the row of P coordinates)"""
    y, th, s2 = np.asarray(y, dtype=LD).reshape(-1), np.asarray(th, dtype=LD), LD(s2)
    if B is None:
        r = y - th
        return -((y.size // 2) * (LOG_2PI + np.log(s2))) - (r * r).sum() / (2 * s2)
    r = y - np.asarray(B, dtype=LD) @ th
    return (-(LOG_2PI + np.log(s2)) / 2 - r * r / (2 * s2)).sum()


def record_curve(y, B, th, s2):
    """the same in fp64 through the record: rss = yy - 2 theta's + theta'G theta"""
    y, th = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(th, dtype=np.float64)
    if B is None:
        G, s, ni_term = np.eye(y.size), y, (y.size // 2) * np.log(2 * np.pi * s2)
    else:
        B = np.asarray(B, dtype=np.float64)
        G, s, ni_term = B.T @ B, B.T @ y, y.size * (0.91893853320467274178 + np.log(np.sqrt(s2)))
    rss = y @ y - 2.0 * (th @ s) + th @ (G @ th)
    return -ni_term - rss / (2.0 * s2)


def _draw(ch, t, cov, covariance_adj):
    return dict(nu=ch["nu"][..., t], Phi=ch["Phi"][..., t], Z=ch["Z"][..., t], chi=ch["chi"][..., t],
                eta=ch["eta"][..., t] if cov else None, xi=ch["xi"][..., t] if cov and covariance_adj else None)


def curve_matrix(Y, B, chains, first, n_slots, X=None, covariance_adj=False, route=dense_curve):
    """(n, C, n_slots) long double: l_i of slots [first, first + n_slots) of every chain; chains: a list of dicts of get_chain
    arrays ("nu", "Phi", "Z", "chi", "sigma_sq" and, with X, "eta" and "xi"); B: the list of basis matrices, None for the
    multivariate model (Y the rows)"""
    n = len(Y)
    out = np.zeros((n, len(chains), n_slots), dtype=LD)
    for q, ch in enumerate(chains):
        for s in range(n_slots):
            t = first + s
            th = theta(X=X, **_draw(ch, t, X is not None, covariance_adj))
            for i in range(n):
                out[i, q, s] = route(Y[i], None if B is None else B[i], th[i], ch["sigma_sq"][t])
    return out


def totals(curve):
    """(C, n_slots): the sum over the curves, in long double"""
    return np.asarray(curve, dtype=LD).sum(axis=0)


def n_obs(Y):
    return int(sum(np.asarray(y).size for y in Y))


def bound(ref, N_obs):
    """the tolerance the GPU tests hold the kernel and the run's own array to: 1e-10 (|ref| + N_obs)"""
    return 1e-10 * (np.abs(np.asarray(ref, dtype=np.float64)) + N_obs)
