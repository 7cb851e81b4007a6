"""numpy restatements of the per-curve marginal log-density l_i(t), scores integrated out:

    y_i ~ N( B_i c, sigma^2 I + U U' ),  c = sum_k Z_ik (nu_k + eta_k x_i),  U = B_i [V_1 .. V_M],
    V_m = sum_k Z_ik (phi_km + xi_km x_i)

`dense` forms the n_i x n_i covariance and uses slogdet / solve, as the CPU restatement of the post-processing does;
`suffstat` is the rank-M form over (G_i, s_i, yy_i, n_i) that k_chain_curve_ll evaluates.  Arrays are in the reference's
shapes: nu (K, P), Phi (K, P, M), eta (P, D, K), xi (P, D, M, K)."""
import numpy as np

LOG_2PI = 1.83787706640934548356

# Worst |dense - suffstat| / max(1, |l|) that tests/test_curve_ll_ref.py measures over its 2000 random curves: the floor the
# two forms themselves impose.  The device is held to ten times it (a different summation order).
FORM_FLOOR = 8.3e-12
GPU_TOL = 10.0 * FORM_FLOOR


def coefficients(z, nu, Phi, x=None, eta=None, xi=None):
    """c (P,) and V (P, M) of one curve under one draw; xi None: mean-adjusted only"""
    K, P, M = Phi.shape
    c = np.zeros(P)
    V = np.zeros((P, M))
    for k in range(K):
        a = nu[k].copy()
        if x is not None and eta is not None:
            a = a + eta[:, :, k] @ x
        c += z[k] * a
        for m in range(M):
            v = Phi[k, :, m].copy()
            if x is not None and xi is not None:
                v = v + xi[:, :, m, k] @ x
            V[:, m] += z[k] * v
    return c, V


def dense(y, B, c, V, sigma_sq):
    ni = len(y)
    U = B @ V
    cov = sigma_sq * np.eye(ni) + U @ U.T
    r = y - B @ c
    sign, logdet = np.linalg.slogdet(cov)
    assert sign > 0
    return -0.5 * (ni * LOG_2PI + logdet + r @ np.linalg.solve(cov, r))


def suffstat(G, s, yy, ni, c, V, sigma_sq):
    M = V.shape[1]
    g = G @ c
    rr = yy - 2.0 * (c @ s) + c @ g
    u = V.T @ (s - g)
    A = sigma_sq * np.eye(M) + V.T @ G @ V
    L = np.linalg.cholesky(A)
    w = np.linalg.solve(L, u)
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    return -0.5 * (ni * LOG_2PI + (ni - M) * np.log(sigma_sq) + logdet + (rr - w @ w) / sigma_sq)


def rel_diff(a, b):
    """|a - b| / max(1, |b|), elementwise"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def dense_matrix(Y, B, chains, first_slot, n_slots, X=None, covariance_adj=False):
    """(n, C, S) by `dense`: chains is a list (one per chain) of dicts of get_chain arrays nu (K, P, T), Phi (K, P, M, T),
    Z (n, K, T), sigma_sq (T,), with covariates eta (P, D, K, T) and xi (P, D, M, K, T); B None: the multivariate model
    (B_i = I)."""
    n = len(Y)
    out = np.zeros((n, len(chains), n_slots))
    for q, ch in enumerate(chains):
        for j in range(n_slots):
            t = first_slot + j
            nu, Phi, sig = ch["nu"][:, :, t], ch["Phi"][:, :, :, t], float(ch["sigma_sq"][t])
            eta = ch["eta"][..., t] if X is not None else None
            xi = ch["xi"][..., t] if X is not None and covariance_adj else None
            for i in range(n):
                y = np.asarray(Y[i], dtype=np.float64)
                Bi = np.eye(len(y)) if B is None else B[i]
                c, V = coefficients(ch["Z"][i, :, t], nu, Phi, None if X is None else X[i], eta, xi)
                out[i, q, j] = dense(y, Bi, c, V, sig)
    return out
