"""numpy restatements of the observation-level leave-one-out quantities: under one draw, with the scores integrated
out, y_i ~ N(B_i c, sigma^2 I + U U'), U = B_i [V_1 .. V_M] (c, V from curve_ll_ref.coefficients), and the law of y_ij given the
rest of the curve is N(m_ij, v_ij):

    l = log N(y_ij; m_ij, v_ij),  z = (y_ij - m_ij) / sqrt(v_ij)

`dense` conditions explicitly on the n_i x n_i covariance, deleting row and column j and solving; `leverage` is the closed form
k_loo_pointwise evaluates, with A and u taken from (G_i, s_i) as the device takes them from the resident record; `expect` is the
expectation of an auxiliary row under the Pareto-smoothed weights of psis_ref.psis_row.  A helper, not a test module."""
import math

import numpy as np

import curve_ll_ref as CL
import psis_ref

LOG_2PI = CL.LOG_2PI

# Worst |leverage - dense| / max(1, |dense|) that tests/test_loo_pointwise_ref.py measures over its 2000 random curves, for l, m,
# sqrt(v) and z: the floor the two forms impose on each other.  The device is held to ten times it, against `dense` (the rule of
# DESIGN.md 7d); the figures are not taken from the kernel.
# The worst cases are long curves at sigma^2 near 1e-4: there the dense solve (condition number about 1e7) is the inexact side, and z
# and l carry its error in m divided by sigma.
FORM_FLOOR_L = 4.6e-8
FORM_FLOOR_M = 3.4e-10
FORM_FLOOR_SD = 2.7e-12
FORM_FLOOR_Z = 1.4e-8
GPU_TOL_L = 10.0 * FORM_FLOOR_L
GPU_TOL_M = 10.0 * FORM_FLOOR_M
GPU_TOL_SD = 10.0 * FORM_FLOOR_SD
GPU_TOL_Z = 10.0 * FORM_FLOOR_Z
# Phi(z) has slope phi(z) <= 0.4, and phi(z) max(1, |z|) <= 0.4 as well: an error of GPU_TOL_Z max(1, |z|) in z moves Phi by less than
# 0.4 GPU_TOL_Z, whatever z; erfc itself adds a few units of 1e-16.
GPU_TOL_PIT = 0.4 * GPU_TOL_Z + 1e-15

rel_diff = CL.rel_diff


def norm_cdf(z):
    """Phi(z) through math.erfc, elementwise"""
    return np.vectorize(lambda v: 0.5 * math.erfc(-v / math.sqrt(2.0)))(np.asarray(z, dtype=np.float64))


def dense(y, B, c, V, sigma_sq):
    """(l, m, v, z), each (n_i,): observation j given the others by deleting row and column j of the dense covariance"""
    y = np.asarray(y, dtype=np.float64)
    ni = len(y)
    U = B @ V
    cov = sigma_sq * np.eye(ni) + U @ U.T
    mu = B @ c
    if ni == 1:
        m, v = mu.copy(), np.diag(cov).copy()
    else:
        # the n_i systems of order n_i - 1 in one stacked solve: row j of `keep` lists the observations other than j
        keep = np.array([[a for a in range(ni) if a != j] for j in range(ni)])
        k = cov[np.arange(ni)[:, None], keep]                                        # (n_i, n_i - 1): cov(y_j, y_-j)
        sol = np.linalg.solve(cov[keep[:, :, None], keep[:, None, :]], np.stack([(y - mu)[keep], k], axis=-1))
        m = mu + np.einsum("ja,ja->j", k, sol[:, :, 0])
        v = np.diag(cov) - np.einsum("ja,ja->j", k, sol[:, :, 1])
    z = (y - m) / np.sqrt(v)
    l = -0.5 * (LOG_2PI + np.log(v) + z * z)
    return l, m, v, z


def leverage(y, B, c, V, sigma_sq, G=None, s=None):
    """(l, m, v, z) by the leverage form; G = B'B and s = B'y as the device holds them (computed here where not given)"""
    y = np.asarray(y, dtype=np.float64)
    M = V.shape[1]
    G = B.T @ B if G is None else G
    s = B.T @ y if s is None else s
    A = sigma_sq * np.eye(M) + V.T @ G @ V
    u = V.T @ (s - G @ c)
    L = np.linalg.cholesky(A)
    beta = np.linalg.solve(A, u)
    W = B @ V                                            # rows w_j
    r = y - B @ c
    Lw = np.linalg.solve(L, W.T)                         # columns L^-1 w_j
    h = np.sum(Lw * Lw, axis=0)
    om = 1.0 - h
    e = r - W @ beta
    l = -0.5 * (LOG_2PI + math.log(sigma_sq) - np.log(om) + e * e / (sigma_sq * om))
    z = e / np.sqrt(sigma_sq * om)
    return l, y - e / om, sigma_sq / om, z


def expect(ll, h):
    """sum_t exp(lw_t) h_t / sum_t exp(lw_t) with the final log-weights of psis_ref.psis_row(ll); h: (S,) or (n_aux, S)"""
    lw = psis_ref.psis_row(ll)["lw"]
    w = np.exp(lw - np.max(lw))
    return np.asarray(h, dtype=np.float64) @ w / np.sum(w)


def dense_traces(Y, B, chains, first_slot, n_slots, X=None, covariance_adj=False, curves=None):
    """(l, Phi(z), m, v, z), each (N_obs, C, S), by `dense`: the arguments of curve_ll_ref.dense_matrix and the curves selected
    (None: all), observation by observation in that order"""
    sel = range(len(Y)) if curves is None else list(curves)
    N = sum(len(Y[i]) for i in sel)
    out = [np.zeros((N, len(chains), n_slots)) for _ in range(4)]
    for q, ch in enumerate(chains):
        for j in range(n_slots):
            t = first_slot + j
            nu, Phi, sig = ch["nu"][:, :, t], ch["Phi"][:, :, :, t], float(ch["sigma_sq"][t])
            eta = ch["eta"][..., t] if X is not None else None
            xi = ch["xi"][..., t] if X is not None and covariance_adj else None
            o = 0
            for i in sel:
                y = np.asarray(Y[i], dtype=np.float64)
                Bi = np.eye(len(y)) if B is None else B[i]
                c, V = CL.coefficients(ch["Z"][i, :, t], nu, Phi, None if X is None else X[i], eta, xi)
                for a, val in zip(out, dense(y, Bi, c, V, sig)):
                    a[o:o + len(y), q, j] = val
                o += len(y)
    l, m, v, z = out
    return l, norm_cdf(z), m, v, z
