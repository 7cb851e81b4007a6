"""numpy restatement of the pooled per-curve covariance surfaces of chain slots (kernels_curve_cov.hip):

    V_im      = sum_k Z_ik (phi_km + sum_d x_id xi_kmd)            (xi only when covariance-adjusted)
    C_i(g, h) = sum_m (E1_g . V_im)(E2_h . V_im),    mean and two-pass sd (N - 1) over the N = C S draws, per-chain means

from get_chain copies in the layouts tests/curve_fit_ref.py reads (Z (n, K, T), Phi (K, P, M, T), xi (P, D, M, K, T)) plus X
(n, D), the same expression with every factor replaced by its absolute value (A >= |d| per draw), and the tolerance a device
result is held to.  The tolerance is derived, not measured.  With u = 2^-52 (twice the unit roundoff, which absorbs the
second-order terms) and D the number of covariates that enter V:

    W[g][m] = sum_k Z_ik (E_g . phi_km + sum_d x_id E_g . xi_kmd) is P products and P - 1 additions per projection, D products
    and additions for the covariates, one product and one addition per k: a computed W is within (P + K (1 + D) + 1) u of its
    absolute-valued form, in any order of the sums;
    d = sum_m W1 W2 adds one product and at most M additions: within c_d u A, c_d = 2 (P + K (1 + D)) + M + 3;
    summing N of them adds (N - 1) u sum A; the sd is Lipschitz in the draws with constant sqrt(N / (N - 1)) in the max-norm.

Device against the float64 restatement, each side rounding once:

    |mean - mean_ref| <= 2 (N + c_d) u mean_t(A)                   (chain_mean: S for N and the chain's own draws)
    |sd - sd_ref|     <= 4 N u sd_ref + 2 c_d u sqrt(N / (N - 1)) max_t A
"""
import numpy as np

U = 2.0 ** -52


def c_d(P, K, M, D):
    return 2 * (P + K * (1 + D)) + M + 3


def _prep(absolute, dtype):
    return (lambda a: np.abs(np.asarray(a, dtype=dtype))) if absolute else (lambda a: np.asarray(a, dtype=dtype))


def _w(E, Z, Phi, X, xi, f):
    """(n, G, M, S): E_g . V_im of every draw"""
    w = np.einsum("iks,gkms->igms", Z, np.einsum("gp,kpms->gkms", E, Phi))
    if X is not None:
        w = w + np.einsum("iks,id,gdmks->igms", Z, X, np.einsum("gp,pdmks->gdmks", E, f(xi)))
    return w


def draw_values(E1, E2, Z, Phi, X=None, xi=None, diagonal=False, dtype=np.float64, absolute=False):
    """d of S draws: (n, G1, G2, S), or (n, G1, S) with diagonal.  Z (n, K, S), Phi (K, P, M, S), xi (P, D, M, K, S); X (n, D)
    only where xi enters V (covariance-adjusted).  E2 None: E2 = E1.  absolute: every factor replaced by its absolute value."""
    f = _prep(absolute, dtype)
    Z, Phi = f(Z), f(Phi)
    Xf = None if X is None else f(X)
    w1 = _w(f(E1), Z, Phi, Xf, xi, f)
    w2 = w1 if E2 is None else _w(f(E2), Z, Phi, Xf, xi, f)
    return np.einsum("igms,igms->igs", w1, w2) if diagonal else np.einsum("igms,ihms->ighs", w1, w2)


def draws(chains, E1, E2, first, n_slots, X=None, covariance_adj=False, curves=None, diagonal=False, absolute=False):
    """(m, [G1, G2] or [G1], C, S) from the get_chain copies of every chain"""
    sl = slice(first, first + n_slots)
    idx = slice(None) if curves is None else np.asarray(curves, dtype=np.int64)
    use_x = X is not None and covariance_adj
    out = []
    for ch in chains:
        kw = dict(X=np.asarray(X)[idx], xi=ch["xi"][..., sl]) if use_x else {}
        out.append(draw_values(E1, E2, ch["Z"][idx][..., sl], ch["Phi"][..., sl], diagonal=diagonal, absolute=absolute, **kw))
    return np.stack(out, axis=-2)


def summarise(d):
    """mean, two-pass sd (NaN for one draw) over the last two axes (C, S) pooled, and per-chain means moved to axis 1"""
    C, S = d.shape[-2:]
    flat = d.reshape(d.shape[:-2] + (C * S,))
    mean = flat.mean(axis=-1)
    sd = np.full(mean.shape, np.nan) if C * S < 2 else flat.std(axis=-1, ddof=1)
    return mean, sd, np.ascontiguousarray(np.moveaxis(d.mean(axis=-1), -1, 1))


def surfaces(chains, E1, E2, first, n_slots, X=None, covariance_adj=False, curves=None, diagonal=False):
    """what Sampler.curve_cov(sd=True, per_chain=True) returns, and the bounds of its three results under "bound_*" """
    d = draws(chains, E1, E2, first, n_slots, X, covariance_adj, curves, diagonal)
    A = draws(chains, E1, E2, first, n_slots, X, covariance_adj, curves, diagonal, absolute=True)
    mean, sd, cm = summarise(d)
    K, P, M = chains[0]["Phi"].shape[:3]
    D = np.asarray(X).shape[1] if (X is not None and covariance_adj) else 0
    C, S = d.shape[-2:]
    N = C * S
    cd = c_d(P, K, M, D)
    out = {"mean": mean, "sd": sd, "chain_mean": cm}
    out["bound_mean"] = mean_bound(A.reshape(A.shape[:-2] + (N,)).mean(axis=-1), N, cd)
    out["bound_chain_mean"] = mean_bound(np.ascontiguousarray(np.moveaxis(A.mean(axis=-1), -1, 1)), S, cd)
    out["bound_sd"] = None if N < 2 else sd_bound(sd, A.reshape(A.shape[:-2] + (N,)).max(axis=-1), N, cd)
    return out


def mean_bound(mean_A, N, cd):
    return 2.0 * (N + cd) * U * np.asarray(mean_A, dtype=np.float64)


def sd_bound(sd_ref, max_A, N, cd):
    return 4.0 * N * U * np.asarray(sd_ref, dtype=np.float64) + 2.0 * cd * U * np.sqrt(N / (N - 1.0)) * np.asarray(max_A, dtype=np.float64)


# ---- cases of one (curve, g, h) each, for the CPU tests: e1, e2 (c, P), Z (c, N, K), Phi (c, N, K, P, M), xi (c, N, K, P, M, D)
# or None, x (c, D) ----
def pair_draws(e1, e2, Z, Phi, xi=None, x=None, dtype=np.float64, absolute=False):
    """(c, N): d of every draw of every case, numpy's own summation order"""
    f = _prep(absolute, dtype)
    e1, e2, Z, Phi = f(e1), f(e2), f(Z), f(Phi)

    def w(e):
        t = np.einsum("cp,cnkpm->cnkm", e, Phi)
        if xi is not None:
            t = t + np.einsum("cd,cp,cnkpmd->cnkm", f(x), e, f(xi))
        return np.einsum("cnk,cnkm->cnm", Z, t)
    return np.einsum("cnm,cnm->cn", w(e1), w(e2))


def pair_draws_sequential(e1, e2, Z, Phi, xi=None, x=None):
    """the same in float64 in the kernel's order: p in order, then d, then k, then m, one operation at a time"""
    e1, e2, Z, Phi = (np.asarray(a, dtype=np.float64) for a in (e1, e2, Z, Phi))
    c, N, K, P, M = Phi.shape
    D = 0 if xi is None else xi.shape[-1]

    def proj(e, th):          # th (c, N, P)
        s = np.zeros((c, N))
        for p in range(P):
            s = s + e[:, None, p] * th[:, :, p]
        return s

    def w(e, m):
        acc = np.zeros((c, N))
        for k in range(K):
            b = proj(e, Phi[:, :, k, :, m])
            for dd in range(D):
                b = b + np.asarray(x, dtype=np.float64)[:, None, dd] * proj(e, np.asarray(xi, dtype=np.float64)[:, :, k, :, m, dd])
            acc = acc + Z[:, :, k] * b
        return acc
    d = np.zeros((c, N))
    for m in range(M):
        d = d + w(e1, m) * w(e2, m)
    return d


def pair_draws_cluster(e1, e2, Z, Phi, xi=None, x=None, dtype=np.float64):
    """sum_k sum_k' Z_k Z_k' C^(k,k'), C^(k,k') = sum_m (e1 . phi_km)(e2 . phi_k'm) the cluster-level surfaces (with the curve's
    covariates in phi where they enter)"""
    f = _prep(False, dtype)
    e1, e2, Z, Phi = f(e1), f(e2), f(Z), f(Phi)

    def t(e):
        v = np.einsum("cp,cnkpm->cnkm", e, Phi)
        if xi is not None:
            v = v + np.einsum("cd,cp,cnkpmd->cnkm", f(x), e, f(xi))
        return v
    Ckk = np.einsum("cnkm,cnlm->cnkl", t(e1), t(e2))
    return np.einsum("cnk,cnl,cnkl->cn", Z, Z, Ckk)


def moments(d):
    """mean and two-pass sd (N - 1) along the last axis, numpy's own order, in d's dtype"""
    N = d.shape[-1]
    mean = d.sum(axis=-1) / d.dtype.type(N)
    q = ((d - mean[..., None]) ** 2).sum(axis=-1)
    return mean, np.sqrt(q / d.dtype.type(N - 1))


def moments_sequential(d):
    """the same in float64 with the draws in order, one addition at a time"""
    d = np.asarray(d, dtype=np.float64)
    N = d.shape[-1]
    s = np.zeros(d.shape[:-1])
    for t in range(N):
        s = s + d[..., t]
    mean = s / float(N)
    q = np.zeros(d.shape[:-1])
    for t in range(N):
        e = d[..., t] - mean
        q = q + e * e
    return mean, np.sqrt(q / float(N - 1))


def sd_one_pass(d):
    """the one-pass variance sum d^2 - (sum d)^2 / N in float64: what the device must not do"""
    d = np.asarray(d, dtype=np.float64)
    N = d.shape[-1]
    s1, s2 = d.sum(axis=-1), (d * d).sum(axis=-1)
    with np.errstate(invalid="ignore"):
        return np.sqrt((s2 - s1 * s1 / N) / (N - 1.0))
