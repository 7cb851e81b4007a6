"""numpy restatement of the cluster covariance surfaces of chain slots under aligned labels (DESIGN.md 7k;
kernels_cluster_cov.hip), the reference's FCovCI over a chain batch:

    theta_km(cs)   = phi_{perm[k], m}(cs) + sum_d x_d xi_{perm[k], m, d}(cs)        (no x: phi alone)
    W1_k[g][m](cs) = sum_p E1_gp theta_km,p(cs),   W2 likewise with E2
    c_r(g, h; cs)  = sum_m W1_{k_r}[g][m] W2_{l_r}[h][m]

from get_chain copies (Phi (K, P, M, T), xi (P, D, M, K, T)), a permutation row per draw (C, S, K), E1, E2 and x; the same
expression with every factor replaced by its absolute value (A >= |c| per draw); and the tolerance a device value is held to.

The tolerance is derived, not measured.  With u = 2^-52 (twice the unit roundoff, which absorbs the second-order terms; the
convention of tests/curve_cov_ref.py) and D the number of covariates that enter theta (0 without x):

    theta is D products and D additions, W = sum_p E_gp theta_p is P products and P additions (the first onto an exact zero):
    every term of the computed W carries at most P + D + 1 roundings, so W is within (P + D + 1) u / 2 of the exact value
    relative to its absolute-valued form, in any order of the sums;
    a value is one product of two such W per m and at most M additions of them (the device's fused products round less): the
    computed value is within (2 (P + D + 1) + M + 1) u / 2 A of the exact one;
    device against the float64 restatement, each side rounding on its own, is twice that, (2 (P + D + 1) + M + 1) u A.

The constant used, c_v = 2 (P + D + 1) + M + 3, is the derived one plus 2, the same allowance tests/curve_cov_ref.py makes for
what first order leaves out.

    |device - float64 restatement| <= b = c_v u A

The sum over m is taken one m at a time in order, as elementwise products, so that the restatement itself is exactly transposed
under (k, l, E1, E2) -> (l, k, E2, E1): the products commute and the additions come in the same order."""
import numpy as np

import curve_sim_ref as SR

U = 2.0 ** -52


def c_v(P, M, D):
    return 2 * (P + D + 1) + M + 3


def all_pairs(K):
    return [(k, l) for k in range(K) for l in range(k, K)]


def _prep(absolute, dtype):
    return (lambda a: np.abs(np.asarray(a, dtype=dtype))) if absolute else (lambda a: np.asarray(a, dtype=dtype))


def aligned_theta(Phi, perm, xi=None, x=None, dtype=np.float64, absolute=False):
    """theta (K, P, M, S) of one chain's S draws with the components relabelled: Phi (K, P, M, S), xi (P, D, M, K, S), perm (S, K)"""
    f = _prep(absolute, dtype)
    th = f(Phi)
    if x is not None:
        xv, xif = f(x), f(xi)
        for d in range(xv.shape[0]):                     # d in order from 0
            th = th + xv[d] * np.transpose(xif[:, d], (2, 0, 1, 3))
    K, P, M, S = th.shape
    idx = np.asarray(perm, dtype=np.int64).T             # (K, S)
    return th[idx[:, None, None, :], np.arange(P)[None, :, None, None], np.arange(M)[None, None, :, None], np.arange(S)[None, None, None, :]]


def draw_values(E1, E2, theta, pairs, diagonal=False, dtype=np.float64, absolute=False):
    """(m, G1, G2, S), or (m, G1, S) with diagonal, from the aligned theta (K, P, M, S).  E2 None: E2 = E1."""
    f = _prep(absolute, dtype)
    th = np.asarray(theta, dtype=dtype)
    w1 = np.einsum("gp,kpms->kgms", f(E1), th)
    w2 = w1 if E2 is None else np.einsum("gp,kpms->kgms", f(E2), th)
    ks = [int(p[0]) for p in pairs]
    ls = [int(p[1]) for p in pairs]
    a, b = w1[ks], w2[ls]                                # (m, G, M, S)
    M = th.shape[2]
    out = None
    for m in range(M):                                   # m in order from 0, one product and one addition at a time
        t = a[:, :, m, :] * b[:, :, m, :] if diagonal else a[:, :, None, m, :] * b[:, None, :, m, :]
        out = t if out is None else out + t
    return out


def values(chains, perm, E1, E2, first, n_slots, pairs=None, x=None, diagonal=False, dtype=np.float64, absolute=False):
    """what Sampler.cluster_cov_bands(trace=True)["trace"] holds: (m, G1, G2, N) or (m, G1, N), N = C S chain-major.
    chains: the get_chain copies of every chain ("Phi", and "xi" where x is given); perm (C, S, K)."""
    sl = slice(first, first + n_slots)
    K = chains[0]["Phi"].shape[0]
    if pairs is None:
        pairs = all_pairs(K)
    out = []
    for q, ch in enumerate(chains):
        kw = dict(xi=ch["xi"][..., sl], x=x) if x is not None else {}
        th = aligned_theta(ch["Phi"][..., sl], perm[q], dtype=dtype, absolute=absolute, **kw)
        out.append(draw_values(E1, E2, th, pairs, diagonal, dtype, absolute))
    return np.concatenate(out, axis=-1)


def bound(chains, perm, E1, E2, first, n_slots, pairs=None, x=None, diagonal=False):
    """b = c_v u A for every entry of `values`"""
    K, P, M = chains[0]["Phi"].shape[:3]
    D = 0 if x is None else len(x)
    return c_v(P, M, D) * U * values(chains, perm, E1, E2, first, n_slots, pairs, x, diagonal, absolute=True)


def sim_bands(trace, alpha, mean, sd):
    """curve_sim_ref.sim_bands per pair: trace (m, ..., N) with the pair's entries on the axes between, mean and sd (m, ...).
    Returns {"crit": (m,), "lower", "upper": (m, ...)}."""
    trace = np.asarray(trace, dtype=np.float64)
    m, N = trace.shape[0], trace.shape[-1]
    r = SR.sim_bands(trace.reshape(m, -1, N), alpha, np.asarray(mean).reshape(m, -1), np.asarray(sd).reshape(m, -1))
    return {"crit": r["crit"], "lower": r["lower"].reshape(np.shape(mean)), "upper": r["upper"].reshape(np.shape(mean))}
