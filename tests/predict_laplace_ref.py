"""numpy restatement of the Laplace mixture proposal for the membership integral, in the style of predict_ref.py: the
integrand's log density g over the log-ratios eta with its gradient and Hessian from the tables Gamma and tau, written over a dtype so
that float64 can be held against np.longdouble; the damped Newton search from K + 1 starts; the component rule; the density of the
mixture of Student-t components with 4 degrees of freedom; the weights and the estimate."""
import math

import numpy as np

import predict_ref as R

LD = np.longdouble
NU = 4.0
ITERS, DEC, SAME = 40, 1e-6, 1e-3


# ---- small dense algebra over a dtype (numpy.linalg has no long double) ----------------------------------------------------------
def chol(A):
    """lower C with C C' = A, or None where a pivot is not positive"""
    n = A.shape[0]
    C = np.zeros_like(A)
    for i in range(n):
        for j in range(i + 1):
            v = A[i, j] - C[i, :j] @ C[j, :j]
            if i == j:
                if not (v > 0) or not np.isfinite(v):
                    return None
                C[i, i] = np.sqrt(v)
            else:
                C[i, j] = v / C[j, j]
    return C


def chol_solve(C, y):
    """(C C')^-1 y, y a vector or a matrix of columns"""
    n = C.shape[0]
    x = np.array(y, dtype=C.dtype, copy=True)
    for i in range(n):
        x[i] = (x[i] - C[i, :i] @ x[:i]) / C[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - C[i + 1:, i] @ x[i + 1:]) / C[i, i]
    return x


# ---- the target ---------------------------------------------------------------------------------------------------------------
def make_case(B, y, th, sigma_sq, alpha):
    """the tables of one (curve, draw): Gamma (K, M+1, K, M+1), tau (K, M+1), yy, n*, sigma^2, alpha = alpha_3 pi and lB(alpha)"""
    G, s, yy, n = R.record(B, y)
    Gam, tau = R.gamma_tables(G, s, th)
    alpha = np.asarray(alpha, dtype=np.float64)
    return {"Gam": Gam, "tau": tau, "yy": yy, "n": n, "sig": float(sigma_sq), "alpha": alpha, "lB": R.log_beta(alpha), "B": B, "y": y, "th": th}


def z_of_eta(eta, dtype=np.float64):
    """z_k = e^eta_k / (1 + sum e^eta), k < d, z_K = 1 / (1 + sum e^eta), clamped below at DBL_MIN; eta (d,) or (J, d)"""
    eta = np.asarray(eta, dtype=dtype)
    e = np.concatenate([eta, np.zeros(eta.shape[:-1] + (1,), dtype=dtype)], axis=-1)
    e = np.exp(e - np.maximum(e.max(axis=-1, keepdims=True), 0))
    return np.maximum(e / e.sum(axis=-1, keepdims=True), dtype(R.TINY))


def eta_of_z(z):
    z = np.asarray(z)
    return np.log(z[..., :-1] / z[..., -1:])


def evaluate(case, eta, dtype=np.float64, derivs=True):
    """g(eta), and with derivs its gradient (d,) and Hessian (d, d), by the formulas of DESIGN.md 7p.  g is -inf where A has no factor."""
    Gam, tau, alpha = case["Gam"].astype(dtype), case["tau"].astype(dtype), case["alpha"].astype(dtype)
    yy, sig, n = dtype(case["yy"]), dtype(case["sig"]), case["n"]
    K, M1 = tau.shape
    M, d = M1 - 1, K - 1
    z = z_of_eta(eta, dtype)
    S = np.einsum("kalb,l->kab", Gam, z)
    T = np.einsum("k,kab->ab", z, S)
    T = (T + T.T) / 2
    t = z @ tau
    rr = yy - 2 * t[0] + T[0, 0]
    u = t[1:] - T[1:, 0]
    A = sig * np.eye(M, dtype=dtype) + T[1:, 1:]
    Lc = chol(A)
    if Lc is None:
        return (-np.inf, None, None) if derivs else -np.inf
    b = chol_solve(Lc, u)
    F = 2 * np.log(np.diag(Lc)).sum() + (rr - u @ b) / sig
    a0 = alpha.sum()
    g = -(n * dtype(R.LOG_2PI) + (n - M) * np.log(sig) + F) / 2 + alpha @ np.log(z) - dtype(case["lB"])
    if not derivs:
        return g
    Ai = chol_solve(Lc, np.eye(M, dtype=dtype))
    D = S + S.transpose(0, 2, 1)
    dA, du, drr = D[:, 1:, 1:], tau[:, 1:] - D[:, 1:, 0], -2 * tau[:, 0] + D[:, 0, 0]
    Pk = np.einsum("mq,kqn->kmn", Ai, dA)
    Ab = np.einsum("kmn,n->km", dA, b)
    r = du - Ab
    w = np.einsum("mn,kn->km", Ai, r)
    dF = np.einsum("kmm->k", Pk) + (drr - 2 * du @ b + Ab @ b) / sig
    G2 = Gam.transpose(0, 2, 1, 3)                       # [k, l, a, b]
    Dkl = G2 + G2.transpose(0, 1, 3, 2)
    d2F = (np.einsum("nm,klmn->kl", Ai, Dkl[:, :, 1:, 1:]) - np.einsum("kmn,lnm->kl", Pk, Pk) +
           (Dkl[:, :, 0, 0] + 2 * np.einsum("m,klm->kl", b, Dkl[:, :, 1:, 0]) + np.einsum("m,klmn,n->kl", b, Dkl[:, :, 1:, 1:], b) -
            2 * np.einsum("km,lm->kl", r, w)) / sig)
    lk, lkl = -dF / 2, -d2F / 2
    E = np.eye(K, dtype=dtype)[:, :d] - z[None, :d]       # delta_ik - z_k
    Jm = z[:, None] * E
    Q = np.diag(z[:d]) - np.outer(z[:d], z[:d])           # z_k (delta_kl - z_l)
    grad = lk @ Jm + alpha[:d] - a0 * z[:d]
    H = Jm.T @ lkl @ Jm + np.einsum("i,il,ik->kl", lk * z, E, E) - (lk @ z + a0) * Q
    return g, grad, (H + H.T) / 2


def g_batch(case, etas):
    """g at the rows of etas (J, d) in float64, vectorised (numpy.linalg): the quadrature and the samples of the estimator"""
    Gam, tau, alpha = case["Gam"], case["tau"], case["alpha"]
    K, M1 = tau.shape
    M = M1 - 1
    z = z_of_eta(etas)
    T = np.einsum("jk,jl,kalb->jab", z, z, Gam)
    T = 0.5 * (T + T.transpose(0, 2, 1))
    t = z @ tau
    rr = case["yy"] - 2.0 * t[:, 0] + T[:, 0, 0]
    u = t[:, 1:] - T[:, 1:, 0]
    A = case["sig"] * np.eye(M) + T[:, 1:, 1:]
    sign, logdet = np.linalg.slogdet(A)
    b = np.linalg.solve(A, u[..., None])[..., 0]
    F = logdet + (rr - np.einsum("jm,jm->j", u, b)) / case["sig"]
    g = -0.5 * (case["n"] * R.LOG_2PI + (case["n"] - M) * math.log(case["sig"]) + F) + np.log(z) @ alpha - case["lB"]
    return np.where(sign > 0, g, -np.inf)


def g_dense(case, etas):
    """g at the rows of etas with l in its dense form (slogdet / solve on n* x n*)"""
    z = z_of_eta(etas)
    return R.ell_dense_batch(case["B"], case["y"], case["th"], z, case["sig"]) + np.log(z) @ case["alpha"] - case["lB"]


# ---- the search -----------------------------------------------------------------------------------------------------------------
def starts(alpha):
    """eta of the K + 1 starts: alpha / alpha_0, then for each k 0.9 at k and 0.1 / (K - 1) elsewhere"""
    K = len(alpha)
    zs = [np.asarray(alpha) / np.sum(alpha)]
    for k in range(K):
        z = np.full(K, 0.1 / max(K - 1, 1))
        z[k] = 0.9
        zs.append(z)
    return [eta_of_z(z) for z in zs]


def decrement(grad, H):
    """grad'(-H)^-1 grad, or None where -H is not positive definite"""
    C = chol(-H)
    return None if C is None else grad @ chol_solve(C, grad)


def search(case, eta0, dtype=np.float64):
    """the Levenberg-damped Newton ascent: {"conv", "eta", "g", "H", "iters"}"""
    eta = np.asarray(eta0, dtype=dtype).copy()
    d = len(eta)
    g, grad, H = evaluate(case, eta, dtype)
    out = {"conv": False, "eta": eta, "g": g, "g0": g, "H": H, "iters": 0}
    if not np.isfinite(g):
        return out
    lam = dtype(0)
    for it in range(ITERS + 1):
        out.update(eta=eta, g=g, H=H, iters=it)
        scale = max(1.0, float(np.max(np.abs(np.diag(H))))) if d else 1.0
        C = chol(-H)
        if C is not None:
            delta = chol_solve(C, grad)
            if grad @ delta < DEC:
                out["conv"] = True
                return out
        if it == ITERS:
            return out
        if C is None or lam > 0:
            if C is None and lam == 0:
                lam = dtype(1e-3 * scale)
            tries = 0
            while True:
                C = chol(-H + lam * np.eye(d, dtype=dtype))
                if C is not None:
                    break
                lam = max(10 * lam, dtype(1e-3 * scale))
                tries += 1
                if tries > 60:
                    return out
            delta = chol_solve(C, grad)
        gt, gradt, Ht = evaluate(case, eta + delta, dtype)
        if np.isfinite(gt) and gt >= g - 1e-13 * abs(g):
            eta, g, grad, H = eta + delta, gt, gradt, Ht
            lam = lam / 10
            if lam < 1e-6 * scale:
                lam = dtype(0)
        else:
            lam = max(10 * lam, dtype(1e-3 * scale))
    return out


# ---- the mixture ----------------------------------------------------------------------------------------------------------------
def unpack_L(Lp, d):
    L = np.zeros((d, d), dtype=np.asarray(Lp).dtype)
    for i in range(d):
        L[i, :i + 1] = Lp[i * (i + 1) // 2:i * (i + 1) // 2 + i + 1]
    return L


def defensive(alpha):
    """centre and L of component 0: the log-ratios of p = alpha / alpha_0 and the factor of [alpha_0 (diag p - p p')]^-1"""
    alpha = np.asarray(alpha, dtype=np.float64)
    d = len(alpha) - 1
    return eta_of_z(alpha / alpha.sum()), np.linalg.cholesky(np.diag(1.0 / alpha[:d]) + 1.0 / alpha[d]) if d else np.zeros((0, 0))


def components(case, J):
    """the component rule on the reference's own search: a list of {"eta", "L", "g", "J"}, component 0 first, and the searches"""
    alpha = case["alpha"]
    c0, L0 = defensive(alpha)
    runs = [search(case, e) for e in starts(alpha)]
    comps = [{"eta": c0, "L": L0, "g": runs[0]["g0"], "J": 0}]
    for r in runs:
        if not r["conv"] or any(np.max(np.abs(r["eta"] - c["eta"]), initial=0.0) < SAME for c in comps[1:]):
            continue
        Lc = np.linalg.cholesky(np.linalg.inv(-r["H"])) if len(c0) else np.zeros((0, 0))
        comps.append({"eta": r["eta"], "L": Lc, "g": r["g"], "J": 0})
    nm = len(comps) - 1
    J0 = J if nm == 0 else max(1, J // 16)
    comps[0]["J"] = J0
    if nm:
        lw = np.array([c["g"] + np.log(np.diag(c["L"])).sum() for c in comps[1:]])
        w = np.exp(lw - lw.max())
        w /= w.sum()
        Jc = np.minimum(np.floor((J - J0) * w).astype(int), J - J0)
        Jc[int(np.argmax(w))] += (J - J0) - Jc.sum()
        for c, j in zip(comps[1:], Jc):
            c["J"] = int(j)
    return comps, runs


def log_t4(eta, centre, L):
    """log density of the d-variate Student-t with 4 degrees of freedom, centre and scale L L', at the rows of eta (J, d)"""
    d = len(centre)
    dt = np.asarray(eta).dtype
    x = np.zeros_like(eta)
    dev = eta - centre
    for i in range(d):
        x[:, i] = (dev[:, i] - x[:, :i] @ L[i, :i]) / L[i, i]
    q2 = (x * x).sum(axis=1)
    const = math.lgamma(0.5 * (NU + d)) - math.lgamma(0.5 * NU) - 0.5 * d * math.log(NU * math.pi)
    return dt.type(const) - np.log(np.diag(L)).sum() - dt.type(0.5 * (NU + d)) * np.log1p(q2 / dt.type(NU))


def log_q(eta, comps, dtype=np.float64):
    """log sum_c (J_c / J) t4(eta; eta_c, L_c) over the components with J_c > 0"""
    eta = np.asarray(eta, dtype=dtype)
    J = sum(c["J"] for c in comps)
    terms = np.stack([np.log(dtype(c["J"]) / dtype(J)) + log_t4(eta, c["eta"].astype(dtype), c["L"].astype(dtype)) for c in comps if c["J"] > 0])
    mx = terms.max(axis=0)
    return mx + np.log(np.exp(terms - mx).sum(axis=0))


def draw(comps, rng):
    """J samples, contiguous by component in component order: eta = centre + L eps sqrt(4 / chi2), chi2 = -2 log(U1 U2)"""
    out = []
    for c in comps:
        d = len(c["eta"])
        eps = rng.standard_normal((c["J"], d))
        chi2 = -2.0 * np.log(rng.uniform(size=c["J"]) * rng.uniform(size=c["J"]))
        out.append(c["eta"] + (eps @ c["L"].T) * np.sqrt(NU / chi2)[:, None])
    return np.concatenate(out, axis=0)


def weigh(g, eta, comps):
    """the stage rule of predict_ref on lw = g - log q and z(eta)"""
    lw = np.asarray(g) - log_q(eta, comps)
    out = R.stage(lw, z_of_eta(eta))
    out["lw"] = lw
    return out


def estimate(case, J, rng):
    """the whole estimator of one (curve, draw) with numpy's variates"""
    comps, runs = components(case, J)
    eta = draw(comps, rng)
    out = weigh(g_batch(case, eta), eta, comps)
    out.update(comps=comps, runs=runs, eta=eta)
    return out


def k2_exact(case, lo=-25.0, hi=25.0, nodes=100001):
    """log of the integral of exp g over eta in [lo, hi] by the trapezoid rule (K = 2)"""
    x = np.linspace(lo, hi, nodes)
    g = g_batch(case, x[:, None])
    w = np.full(nodes, (hi - lo) / (nodes - 1))
    w[0] = w[-1] = 0.5 * w[0]
    mx = g.max()
    return mx + math.log(np.sum(w * np.exp(g - mx)))


# ---- cases and floors -----------------------------------------------------------------------------------------------------------
def random_laplace_case(rng, K=3, M=3, D=0, covariance_adj=False):
    """a predict_ref.random_case curve with a prior alpha_3 pi and an eta near the simplex's interior or out in a tail"""
    B, y, th, z, sig = R.random_case(rng, K=K, M=M, D=D, covariance_adj=covariance_adj)
    alpha = rng.choice([0.3, 1.0, 5.0]) * rng.uniform(0.2, 2.0, size=K)
    eta = rng.choice([0.5, 2.0, 6.0]) * rng.standard_normal(K - 1)
    return make_case(B, y, th, sig, alpha), eta


def rel(a, b):
    """max |a - b| / max(1, max |b|), b the long-double value"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b), initial=0.0) / max(1.0, float(np.max(np.abs(b), initial=0.0))))


def derivative_floor(cases=600, seed=30):
    """the worst float64 - longdouble difference over `cases` random inputs of g, grad g and H (relative to max(1, max |.|) of each),
    of the Newton decrement where -H is positive definite in both (relative to max(1, |.|)) and of log q of a two-component
    mixture: {"g", "grad", "H", "dec", "logq"}"""
    rng = np.random.default_rng(seed)
    worst = {"g": 0.0, "grad": 0.0, "H": 0.0, "dec": 0.0, "logq": 0.0}
    for i in range(cases):
        K = int(rng.choice([2, 3, 5]))
        D, cadj = [(0, False), (2, True)][i % 2]
        case, eta = random_laplace_case(rng, K=K, M=int(rng.choice([1, 2, 3])), D=D, covariance_adj=cadj)
        a, b = evaluate(case, eta), evaluate(case, eta, LD)
        if not (np.isfinite(a[0]) and np.isfinite(b[0])):
            continue
        worst["g"] = max(worst["g"], rel(a[0], b[0]))
        worst["grad"] = max(worst["grad"], rel(a[1], b[1]))
        worst["H"] = max(worst["H"], rel(a[2], b[2]))
        da, db = decrement(a[1], a[2]), decrement(b[1], b[2])
        if da is not None and db is not None:
            worst["dec"] = max(worst["dec"], rel(da, db))
        d = K - 1
        comps = [{"eta": rng.standard_normal(d), "L": np.linalg.cholesky(np.cov(rng.standard_normal((d, d + 3))) + 0.1 * np.eye(d)), "J": 16},
                 {"eta": eta, "L": np.linalg.cholesky(np.cov(rng.standard_normal((d, d + 3))) + 0.01 * np.eye(d)), "J": 240}]
        pts = eta + rng.standard_normal((20, d)) * rng.choice([0.1, 1.0, 10.0])
        worst["logq"] = max(worst["logq"], rel(log_q(pts, comps), log_q(pts, comps, LD)))
    return worst


# ---- the fixture of the comparison with the staged Dirichlet --------------------------------------------------------------------
SHARP = dict(n=4, K=3, M=2, n_pts=100, sigma_sq=0.0002, C=2, S=3, alpha_3=4.0, seed=71)


def sharp_fixture():
    """4 curves of 100 points (K = 3, M = 2, P = 8, sigma^2 = 0.0002) and 2 x 3 parameter draws around the simulation's truth, the
    same on the CPU and on the device (whose chain slots are set to them): (sim, draws[q][s] = {"nu", "Phi", "sigma_sq", "pi", "alpha_3"})"""
    from simdata import simulate_functional
    f = SHARP
    sim = simulate_functional(n=f["n"], M=f["M"], sigma_sq=f["sigma_sq"], seed=f["seed"], K=f["K"], n_pts=f["n_pts"])
    rng = np.random.default_rng(f["seed"] + 1)
    draws = [[{"nu": sim["nu"] + 0.05 * rng.standard_normal(sim["nu"].shape), "Phi": sim["Phi"] + 0.02 * rng.standard_normal(sim["Phi"].shape),
               "sigma_sq": f["sigma_sq"] * float(rng.uniform(0.8, 1.25)), "pi": sim["pi"], "alpha_3": f["alpha_3"]}
              for s in range(f["S"])] for q in range(f["C"])]
    return sim, draws


def sharp_cases(sim, draws):
    """the cases [r][q][s] of the fixture"""
    return [[[make_case(sim["B"][r], sim["y"][r], R.directions(d["nu"], d["Phi"]), d["sigma_sq"], d["alpha_3"] * d["pi"]) for d in row]
             for row in draws] for r in range(len(sim["y"]))]


def staged_dirichlet_ess(case, J, stages, rng):
    """the ess of predict_ref's staged Dirichlet estimator on the case"""
    ell = lambda z: g_batch(case, eta_of_z(z)) - np.log(z) @ case["alpha"] + case["lB"]
    return R.staged_estimate(ell, case["alpha"], J, stages, rng)["ess"]
