"""numpy restatements of the leave-block-out quantities within a curve: under one draw, with the scores integrated
out, y_i ~ N(B_i c, sigma^2 I + U U'), U = B_i [V_1 .. V_M] (c, V from curve_ll_ref.coefficients), and the law of the block y_b
given the rest of the curve is N(m_b, S_b):

    l_b = log N(y_b; m_b, S_b),  m_j, v_j = (S_b)_jj and z_j = (y_j - m_j) / sqrt(v_j) the marginals per observation of the block

`dense` conditions explicitly on the n_i x n_i covariance; `closed` is the form k_loo_blocks evaluates on the M x M system, with A
and u taken from (G_i, s_i) as the device takes them from the resident record.  A helper, not a test module."""
import math

import numpy as np

import curve_ll_ref as CL
import loo_pointwise_ref as LP

LOG_2PI = CL.LOG_2PI

# Worst |closed - dense| / max(1, |dense|) that tests/test_loo_blocks_ref.py measures over its 2000 random curves and blocks, for l,
# m, sqrt(v) and z: the floor the two forms impose on each other.  The device is held to ten times it, against `dense` (the rule of
# DESIGN.md 7d); the figures are not taken from the kernel.
FORM_FLOOR_L = 2.9e-11
FORM_FLOOR_M = 2.5e-10
FORM_FLOOR_SD = 6.9e-11
FORM_FLOOR_Z = 4.6e-9
GPU_TOL_L = 10.0 * FORM_FLOOR_L
GPU_TOL_M = 10.0 * FORM_FLOOR_M
GPU_TOL_SD = 10.0 * FORM_FLOOR_SD
GPU_TOL_Z = 10.0 * FORM_FLOOR_Z
# Phi(z) has slope phi(z) <= 0.4, and phi(z) max(1, |z|) <= 0.4 as well (loo_pointwise_ref.GPU_TOL_PIT)
GPU_TOL_PIT = 0.4 * GPU_TOL_Z + 1e-15

rel_diff = CL.rel_diff
norm_cdf = LP.norm_cdf


def dense(y, B, c, V, sigma_sq, idx):
    """(l_b, m, v, z) of the block idx (indices within the curve, in the order of the result; m, v, z: (|b|,)) by conditioning
    on the dense covariance: the rows and columns of the rest are solved against"""
    y = np.asarray(y, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    ni = len(y)
    U = B @ V
    cov = sigma_sq * np.eye(ni) + U @ U.T
    mu = B @ c
    inb = np.zeros(ni, dtype=bool)
    inb[idx] = True
    rest = np.flatnonzero(~inb)
    if rest.size == 0:
        m, S = mu[idx], cov[np.ix_(idx, idx)]
    else:
        k = cov[np.ix_(idx, rest)]
        sol = np.linalg.solve(cov[np.ix_(rest, rest)], np.column_stack([(y - mu)[rest], k.T]))
        m = mu[idx] + k @ sol[:, 0]
        S = cov[np.ix_(idx, idx)] - k @ sol[:, 1:]
    dlt = y[idx] - m
    _, ld = np.linalg.slogdet(S)
    l = -0.5 * (len(idx) * LOG_2PI + ld + dlt @ np.linalg.solve(S, dlt))
    v = np.diag(S).copy()
    return float(l), m, v, dlt / np.sqrt(v)


def closed(y, B, c, V, sigma_sq, idx, G=None, s=None):
    """(l_b, m, v, z) by the closed form on the M x M system; G = B'B and s = B'y as the device holds them (computed here where
    not given)"""
    y = np.asarray(y, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    M = V.shape[1]
    G = B.T @ B if G is None else G
    s = B.T @ y if s is None else s
    A = sigma_sq * np.eye(M) + V.T @ G @ V
    u = V.T @ (s - G @ c)
    L = np.linalg.cholesky(A)
    W = (B @ V)[idx]                                     # rows w_j of the block
    r = (y - B @ c)[idx]
    Ab = A - W.T @ W
    Lb = np.linalg.cholesky(Ab)
    beta = np.linalg.solve(Ab, u - W.T @ r)
    rt = r - W @ beta
    T = np.linalg.solve(Lb, W.T)                         # columns L_b^-1 w_j
    v = sigma_sq * (1.0 + np.sum(T * T, axis=0))
    t = np.linalg.solve(L, W.T @ rt)
    quad = (rt @ rt - t @ t) / sigma_sq
    l = -0.5 * (len(idx) * (LOG_2PI + math.log(sigma_sq)) + 2.0 * np.sum(np.log(np.diag(L))) - 2.0 * np.sum(np.log(np.diag(Lb))) + quad)
    return float(l), y[idx] - rt, v, rt / np.sqrt(v)


def dense_traces(Y, B, chains, first_slot, n_slots, block_curve, block_offsets, block_obs, X=None, covariance_adj=False):
    """l: (n_blocks, C, S) and (Phi(z), m, v, z): (N_rows, C, S) by `dense`: the chains' get_chain copies as in
    loo_pointwise_ref.dense_traces, the block lists as bfmmm_chain_loo_blocks takes them"""
    nb, N = len(block_curve), int(block_offsets[-1])
    l = np.zeros((nb, len(chains), n_slots))
    out = [np.zeros((N, len(chains), n_slots)) for _ in range(3)]
    for q, ch in enumerate(chains):
        for j in range(n_slots):
            t = first_slot + j
            nu, Phi, sig = ch["nu"][:, :, t], ch["Phi"][:, :, :, t], float(ch["sigma_sq"][t])
            eta = ch["eta"][..., t] if X is not None else None
            xi = ch["xi"][..., t] if X is not None and covariance_adj else None
            cv = {}
            for k in range(nb):
                i = int(block_curve[k])
                y = np.asarray(Y[i], dtype=np.float64)
                if i not in cv:
                    cv[i] = CL.coefficients(ch["Z"][i, :, t], nu, Phi, None if X is None else X[i], eta, xi)
                Bi = np.eye(len(y)) if B is None else B[i]
                a, b = int(block_offsets[k]), int(block_offsets[k + 1])
                lb, m, v, z = dense(y, Bi, cv[i][0], cv[i][1], sig, block_obs[a:b])
                l[k, q, j] = lb
                for o, val in zip(out, (m, v, z)):
                    o[a:b, q, j] = val
    m, v, z = out
    return l, norm_cdf(z), m, v, z
