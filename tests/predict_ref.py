"""numpy restatement of the prediction of held-out curves, given the samples: the marginal log-density l(z) of a new
curve in its dense form (slogdet / solve on n* x n*) and in the Gamma form the device evaluates, and the stage rule of the
importance sampler (weights, lpd, ess, m, q, v and the next proposal), written over a dtype so that float64 can be held against
np.longdouble."""
import math

import numpy as np

LOG_2PI = 1.83787706640934548356
TINY = np.finfo(np.float64).tiny      # the clamp of the gamma variates


def directions(nu, Phi, eta=None, xi=None, x=None, covariance_adj=False):
    """theta[k, mt, p] of one draw with x folded in: mt = 0: nu_k + eta_k x, mt = m: phi_km (+ xi_km x with covariance_adj).
    nu (K, P), Phi (K, P, M), eta (P, D, K), xi (P, D, M, K): one slot of get_chain's arrays."""
    K, P = nu.shape
    M = Phi.shape[2]
    th = np.zeros((K, M + 1, P))
    th[:, 0] = nu
    th[:, 1:] = np.transpose(Phi, (0, 2, 1))
    if x is not None and eta is not None:
        th[:, 0] += np.einsum("pdk,d->kp", eta, x)
        if covariance_adj:
            th[:, 1:] += np.einsum("pdmk,d->kmp", xi, x)
    return th


def ell_dense(B, y, th, z, sigma_sq):
    """log N(y; B c, sigma^2 I + U U'), c = sum_k z_k theta_k0, U = B [V_1 .. V_M], V_m = sum_k z_k theta_km"""
    n = len(y)
    c = z @ th[:, 0]
    U = B @ np.einsum("k,kmp->pm", z, th[:, 1:])
    S = sigma_sq * np.eye(n) + U @ U.T
    r = y - B @ c
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    return -0.5 * (n * LOG_2PI + logdet + r @ np.linalg.solve(S, r))


def record(B, y):
    """(G, s, yy, n*) of a curve"""
    return B.T @ B, B.T @ y, float(y @ y), len(y)


def gamma_tables(G, s, th):
    """Gamma[(k, mt), (k', mt')] = theta_kmt' G theta_k'mt' as (K, M+1, K, M+1), tau[k, mt] = theta_kmt' s"""
    H = th @ G
    return np.einsum("kap,lbp->kalb", th, H), th @ s


def ell_gamma(Gam, tau, yy, n, z, sigma_sq):
    """l(z) from the tables alone"""
    M = tau.shape[1] - 1
    zz = np.outer(z, z)
    cGc = np.einsum("kl,kl->", zz, Gam[:, 0, :, 0])
    cs = z @ tau[:, 0]
    rr = yy - 2.0 * cs + cGc
    u = z @ tau[:, 1:] - np.einsum("kl,kml->m", zz, Gam[:, 1:, :, 0])
    W = np.einsum("kl,kmlj->mj", zz, Gam[:, 1:, :, 1:])
    A = sigma_sq * np.eye(M) + 0.5 * (W + W.T)
    sign, logdet = np.linalg.slogdet(A)
    assert sign > 0
    return -0.5 * (n * LOG_2PI + (n - M) * math.log(sigma_sq) + logdet + (rr - u @ np.linalg.solve(A, u)) / sigma_sq)


def log_beta(a):
    return sum(math.lgamma(v) for v in a) - math.lgamma(float(np.sum(a)))


def log_weights(ell, z, prior, proposal=None):
    """lw_j = l(z_j) + sum_k (prior_k - a_k) log z_jk + lB(a) - lB(prior); proposal None (stage 0): lw = l"""
    ell = np.asarray(ell, dtype=np.float64)
    if proposal is None:
        return ell.copy()
    return ell + np.log(z) @ (np.asarray(prior) - np.asarray(proposal)) + (log_beta(proposal) - log_beta(prior))


def stage(lw, z, dtype=np.float64):
    """The stage rule on log weights lw (J,) and samples z (J, K): {"lpd", "ess", "m", "q", "v", "next"}, `next` the proposal
    of the stage after it."""
    lw = np.asarray(lw).astype(dtype)
    z = np.asarray(z).astype(dtype)
    J, K = z.shape
    mx = lw.max()
    w = np.exp(lw - mx)
    sw = w.sum()
    m = (w[:, None] * z).sum(axis=0) / sw
    q = (w[:, None] * z * z).sum(axis=0) / sw
    v = (w[:, None] * (z - m) ** 2).sum(axis=0) / sw
    pos = v > 0
    one, cap = dtype(1.0), dtype(1e4)
    if pos.any():
        a0 = np.median(m[pos] * (one - m[pos]) / v[pos] - one)
    else:
        a0 = cap
    a0 = min(max(a0, one), cap)
    nxt = np.maximum(a0 * m, dtype(0.5))
    return {"lpd": mx + np.log(sw / dtype(J)), "ess": sw * sw / (w * w).sum(), "m": m, "q": q, "v": v, "next": nxt}


def staged_estimate(ell_fn, prior, J, R, rng):
    """The whole estimator of one (curve, draw) with numpy's Dirichlet samples: ell_fn(z (J, K)) -> (J,).  Returns the last stage's
    dict with "z", "lw" and "proposals" added."""
    prior = np.asarray(prior, dtype=np.float64)
    a, props = None, []
    for st in range(R):
        props.append(prior if a is None else a)
        z = rng.dirichlet(props[-1], size=J)
        z = np.maximum(z, TINY)
        lw = log_weights(ell_fn(z), z, prior, a)
        out = stage(lw, z)
        a = out["next"]
    out.update(z=z, lw=lw, proposals=np.array(props))
    return out


def pooled(lpd_trace, ess_trace, m_trace, q_trace):
    """the pooled results of one curve from its traces over the N draws (m_trace, q_trace: (N, K), already relabelled)"""
    mx = lpd_trace.max()
    zm = m_trace.mean(axis=0)
    return {"lpd": mx + math.log(np.exp(lpd_trace - mx).mean()), "Z_mean": zm,
            "Z_sd": np.sqrt(np.maximum(q_trace.mean(axis=0) - zm * zm, 0.0)), "ess_mean": ess_trace.mean(), "ess_min": ess_trace.min()}


# ---- the floors the tolerances of the tests are built on ----------------------------------------------------------------------
def random_case(rng, P=12, M=3, K=3, D=0, covariance_adj=False):
    """one random new curve and draw: n* in 1 .. 120, sigma^2 in [1e-4, 1] (log-uniform), basis rows with a sparse support of four
    neighbours (as a cubic spline's) or dense, y near the draw's own mean curve with a misfit now and then, z from a Dirichlet with an
    entry at the clamp now and then"""
    n = int(rng.integers(1, 121))
    sig = float(10.0 ** rng.uniform(-4.0, 0.0))
    B = rng.uniform(0.0, 1.0, size=(n, P))
    if rng.uniform() < 0.7:
        mask = np.zeros((n, P))
        for l, p0 in enumerate(rng.integers(0, P - 3, size=n)):
            mask[l, p0:p0 + 4] = 1.0
        B *= mask
    nu = rng.standard_normal((K, P)) * 2.0
    Phi = rng.standard_normal((K, P, M)) * 0.5
    eta = xi = x = None
    if D > 0:
        eta, xi, x = rng.standard_normal((P, D, K)), 0.3 * rng.standard_normal((P, D, M, K)), rng.standard_normal(D)
    th = directions(nu, Phi, eta, xi, x, covariance_adj)
    z = rng.dirichlet(rng.choice([0.3, 1.0, 5.0]) * np.ones(K))
    if rng.uniform() < 0.2:
        z[int(rng.integers(K))] = TINY
    z = np.maximum(z, TINY)
    z0 = rng.dirichlet(np.ones(K))
    y = B @ (z0 @ th[:, 0]) + B @ np.einsum("k,kmp->pm", z0, th[:, 1:]) @ rng.standard_normal(M) + math.sqrt(sig) * rng.standard_normal(n)
    if rng.uniform() < 0.2:
        y += rng.standard_normal(n)
    return B, y, th, z, sig


def ell_floor(cases=2000, seed=20):
    """the worst |l_dense - l_Gamma| / max(1, |l_dense|) over `cases` random curves, with and without covariates, and the largest |l|"""
    rng = np.random.default_rng(seed)
    worst, big = 0.0, 0.0
    for i in range(cases):
        D, cadj = [(0, False), (2, False), (2, True), (0, False)][i % 4]
        B, y, th, z, sig = random_case(rng, D=D, covariance_adj=cadj)
        a = ell_dense(B, y, th, z, sig)
        G, s, yy, n = record(B, y)
        Gam, tau = gamma_tables(G, s, th)
        b = ell_gamma(Gam, tau, yy, n, z, sig)
        worst = max(worst, abs(a - b) / max(1.0, abs(a)))
        big = max(big, abs(a))
    return worst, big


def rule_floor(cases=600, seed=21):
    """the worst |float64 - longdouble| / max(1, |longdouble|) over every output of the stage rule on `cases` random inputs"""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for i in range(cases):
        K = int(rng.choice([2, 3, 8]))
        J = int(rng.choice([37, 300]))
        z = np.maximum(rng.dirichlet(rng.choice([0.3, 1.0, 4.0, 60.0]) * rng.uniform(0.5, 2.0, size=K), size=J), TINY)
        lw = rng.choice([0.1, 1.0, 5.0, 30.0]) * rng.standard_normal(J) - 50.0 * rng.uniform()
        a, b = stage(lw, z), stage(lw, z, np.longdouble)
        for k in a:
            d = np.max(np.abs(np.asarray(a[k], dtype=np.longdouble) - b[k]) / np.maximum(1.0, np.abs(b[k])))
            worst = max(worst, float(d))
    return worst


def ell_dense_batch(B, y, th, Z, sigma_sq):
    """ell_dense for the J rows of Z at once"""
    n = len(y)
    c = Z @ th[:, 0]
    U = B @ np.einsum("jk,kmp->jpm", Z, th[:, 1:])
    S = sigma_sq * np.eye(n) + U @ np.transpose(U, (0, 2, 1))
    r = y[None, :] - c @ B.T
    sign, logdet = np.linalg.slogdet(S)
    assert np.all(sign > 0)
    quad = np.einsum("jn,jn->j", r, np.linalg.solve(S, r[..., None])[..., 0])
    return -0.5 * (n * LOG_2PI + logdet + quad)
