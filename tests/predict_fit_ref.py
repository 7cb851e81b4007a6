"""numpy restatement of the fitted function of held-out curves, given the samples and their weights: the conditional
law of the new curve's function on a grid under one sample z in its dense form (the n* x n* marginal of y_new built from B_new, the
Gaussian conditional of E f on it) and in the table form the device evaluates (Gamma, tau and e = E Theta', an M x M Cholesky), the
mixture over the samples, the pooling over the draws and the path rule.  The table form is written over a dtype, with its own
Cholesky and substitutions, so that float64 can be held against np.longdouble."""
import math

import numpy as np

import predict_ref as R


# ---- one sample: mu_j(g), s_j(g) ------------------------------------------------------------------------------------------------
def fit_dense(B, y, th, z, sigma_sq, E, noise=False):
    """mean and variance on the rows of E of f = c + V chi, chi ~ N(0, I_M) a priori (c = sum_k z_k theta_k0, V = [sum_k z_k
    theta_km]), given y = B f + N(0, sigma^2 I): the Gaussian conditional on the dense n* x n* marginal of predict_ref.ell_dense,
    y ~ N(B c, S), S = sigma^2 I + U U' with U = B V: Cov(E f, y) = E V U', Var(E f) = E V V'E'."""
    n = len(y)
    c = z @ th[:, 0]
    V = np.einsum("k,kmp->pm", z, th[:, 1:])
    U = B @ V
    S = sigma_sq * np.eye(n) + U @ U.T
    EV = E @ V
    Si_r = np.linalg.solve(S, y - B @ c)
    Si_U = np.linalg.solve(S, U)
    mu = E @ c + EV @ (U.T @ Si_r)
    cov = EV @ (np.eye(V.shape[1]) - U.T @ Si_U) @ EV.T
    s = np.diag(cov).copy()
    return mu, s + (sigma_sq if noise else 0.0)


def fit_dense_batch(B, y, th, Z, sigma_sq, E, noise=False):
    """fit_dense for the J rows of Z at once: mu (J, G), s (J, G)"""
    n = len(y)
    c = Z @ th[:, 0]
    V = np.einsum("jk,kmp->jpm", Z, th[:, 1:])
    U = B @ V
    S = sigma_sq * np.eye(n) + U @ np.transpose(U, (0, 2, 1))
    EV = E @ V
    r = y[None, :] - c @ B.T
    Si_r = np.linalg.solve(S, r[..., None])[..., 0]
    Si_U = np.linalg.solve(S, U)
    mu = c @ E.T + np.einsum("jgm,jm->jg", EV, np.einsum("jnm,jn->jm", U, Si_r))
    inner = np.eye(V.shape[2])[None] - np.einsum("jnm,jnl->jml", U, Si_U)
    s = np.einsum("jgm,jml,jgl->jg", EV, inner, EV)
    return mu, s + (sigma_sq if noise else 0.0)


def path_dense(B, y, th, z, sigma_sq, E, xi, eps=None):
    """the path of sample z from the M x M posterior of chi built from B: chi | y ~ N(A^-1 u, sigma^2 A^-1), A = sigma^2 I + U'U = L L',
    u = U'(y - B c); path = E c + E V (A^-1 u + sigma L^-T xi) (+ sigma eps)"""
    c = z @ th[:, 0]
    V = np.einsum("k,kmp->pm", z, th[:, 1:])
    U = B @ V
    A = sigma_sq * np.eye(V.shape[1]) + U.T @ U
    L = np.linalg.cholesky(A)
    coef = np.linalg.solve(A, U.T @ (y - B @ c)) + math.sqrt(sigma_sq) * np.linalg.solve(L.T, np.asarray(xi, dtype=np.float64))
    out = E @ c + E @ (V @ coef)
    return out if eps is None else out + math.sqrt(sigma_sq) * np.asarray(eps)


def e_table(E, th):
    """e[g, k, mt] = E_g . theta_kmt"""
    return np.einsum("gp,kap->gka", E, th)


def _chol(A, dtype):
    M = A.shape[0]
    L = np.zeros((M, M), dtype=dtype)
    for c in range(M):
        L[c, c] = np.sqrt(A[c, c] - (L[c, :c] * L[c, :c]).sum())
        for r in range(c + 1, M):
            L[r, c] = (A[r, c] - (L[r, :c] * L[c, :c]).sum()) / L[c, c]
    return L


def _fwd(L, v, dtype):
    """L^-1 v (v: (M,) or (M, G))"""
    x = np.zeros(v.shape, dtype=dtype)
    for c in range(L.shape[0]):
        x[c] = (v[c] - np.tensordot(L[c, :c], x[:c], axes=1)) / L[c, c]
    return x


def _bwd(L, v, dtype):
    """L^-T v"""
    M = L.shape[0]
    x = np.zeros(v.shape, dtype=dtype)
    for c in range(M - 1, -1, -1):
        x[c] = (v[c] - np.tensordot(L[c + 1:, c], x[c + 1:], axes=1)) / L[c, c]
    return x


def factor(Gam, tau, z, sigma_sq, dtype=np.float64):
    """(L, b) of the sample: A = sigma^2 I + W = L L', b = L^-1 u, from the tables of predict_ref.gamma_tables"""
    Gam, tau, z = np.asarray(Gam, dtype=dtype), np.asarray(tau, dtype=dtype), np.asarray(z, dtype=dtype)
    M = tau.shape[1] - 1
    zz = np.outer(z, z)
    u = z @ tau[:, 1:] - np.einsum("kl,kml->m", zz, Gam[:, 1:, :, 0])
    W = np.einsum("kl,kmlj->mj", zz, Gam[:, 1:, :, 1:])
    L = _chol(dtype(sigma_sq) * np.eye(M, dtype=dtype) + W, dtype)
    return L, _fwd(L, u, dtype)


def fit_table(Gam, tau, e, z, sigma_sq, noise=False, dtype=np.float64):
    """mu_j(g), s_j(g) of the table form: chi^ = L^-T b, mu = c + chi^ . v, s = sigma^2 |L^-1 v|^2 (+ sigma^2)"""
    L, b = factor(Gam, tau, z, sigma_sq, dtype)
    e, z = np.asarray(e, dtype=dtype), np.asarray(z, dtype=dtype)
    chi = _bwd(L, b, dtype)
    c = e[:, :, 0] @ z
    v = np.einsum("k,gkm->mg", z, e[:, :, 1:])
    t = _fwd(L, v, dtype)
    s = dtype(sigma_sq) * (t * t).sum(axis=0)
    return c + chi @ v, s + (dtype(sigma_sq) if noise else dtype(0.0))


def path_table(Gam, tau, e, z, sigma_sq, xi, eps=None):
    """the path of sample z with the standard normals xi (M,): c + (chi^ + sigma L^-T xi) . v (+ sigma eps, eps (G,))"""
    L, b = factor(Gam, tau, z, sigma_sq)
    coef = _bwd(L, b, np.float64) + math.sqrt(sigma_sq) * _bwd(L, np.asarray(xi, dtype=np.float64), np.float64)
    out = e[:, :, 0] @ z + coef @ np.einsum("k,gkm->mg", z, e[:, :, 1:])
    return out if eps is None else out + math.sqrt(sigma_sq) * np.asarray(eps)


# ---- the mixture over the samples, the pooling over the draws, the path rule -------------------------------------------------------
def mixture(w, mu, s):
    """mu_t(g), v_t(g) of sum_j w~_j N(mu_j, s_j): w (J,), mu and s (J, G); two passes"""
    wt = np.asarray(w) / np.sum(w)
    mt = wt @ mu
    return mt, wt @ (s + (mu - mt) ** 2)


def pooled_fit(mu_t, v_t):
    """mean and sd over the N equally weighted draws: mu_t, v_t (N, G)"""
    mean = mu_t.mean(axis=0)
    return mean, np.sqrt(v_t.mean(axis=0) + ((mu_t - mean) ** 2).mean(axis=0))


def path_index(w, U):
    """the first j with sum_{i <= j} w_i > U sum w, the sum in sample order (the last j should rounding leave none)"""
    cum = np.cumsum(np.asarray(w, dtype=np.float64))
    hit = np.nonzero(cum > U * np.sum(w))[0]
    return int(hit[0]) if hit.size else len(cum) - 1


# ---- the floors the tolerances of the tests are built on --------------------------------------------------------------------------
def random_fit_case(rng, i):
    """predict_ref.random_case (P = 12, M = 1 .. 3, K = 3, with and without covariates) with a grid of G = 1 .. 20 B-spline-like rows
    over the whole domain; every fourth curve is observed on the left half of the domain only (its rows touch the first half of the
    basis alone)"""
    D, cadj = [(0, False), (2, False), (2, True), (0, False)][i % 4]
    M = 1 + i % 3
    B, y, th, z, sig = R.random_case(rng, M=M, D=D, covariance_adj=cadj)
    P = B.shape[1]
    if i % 4 == 3:
        B = B.copy()
        B[:, P // 2:] = 0.0
        z0 = rng.dirichlet(np.ones(len(z)))
        y = B @ (z0 @ th[:, 0]) + math.sqrt(sig) * rng.standard_normal(len(y))
    G = int(rng.integers(1, 21))
    E = rng.uniform(0.0, 1.0, size=(G, P))
    mask = np.zeros((G, P))
    for g, p0 in enumerate(rng.integers(0, P - 3, size=G)):
        mask[g, p0:p0 + 4] = 1.0
    return B, y, th, z, sig, E * mask


def _rel(a, b):
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - b) / np.maximum(1.0, np.abs(b))))


def fit_floor(cases=2000, seed=30):
    """(the worst |dense - table| / max(1, |value|) of mu_j and s_j over `cases` random curves, the same of the float64 table form
    against the np.longdouble one, the largest |mu_j|)"""
    rng = np.random.default_rng(seed)
    w_dense, w_ld, big = 0.0, 0.0, 0.0
    for i in range(cases):
        B, y, th, z, sig, E = random_fit_case(rng, i)
        G_, s_, yy, n = R.record(B, y)
        Gam, tau = R.gamma_tables(G_, s_, th)
        e = e_table(E, th)
        mu_d, s_d = fit_dense(B, y, th, z, sig, E)
        mu_t, s_t = fit_table(Gam, tau, e, z, sig)
        ld = np.longdouble
        Gl, sl = (B.astype(ld).T @ B.astype(ld)), B.astype(ld).T @ y.astype(ld)
        thl = th.astype(ld)
        Gam_l, tau_l = np.einsum("kap,lbp->kalb", thl, thl @ Gl), thl @ sl
        mu_l, s_l = fit_table(Gam_l, tau_l, np.einsum("gp,kap->gka", E.astype(ld), thl), z, sig, dtype=ld)
        w_dense = max(w_dense, _rel(mu_d, mu_t), _rel(s_d, s_t))
        w_ld = max(w_ld, _rel(mu_t, mu_l), _rel(s_t, s_l))
        big = max(big, float(np.abs(mu_t).max()))
    return w_dense, w_ld, big
