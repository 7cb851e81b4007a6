"""CPU checks of the numpy restatement of the fitted function of held-out curves (tests/predict_fit_ref.py): the table
form of mu_j and s_j against the dense Gaussian conditional and against np.longdouble, which give the floors of the device tests'
tolerance; and the pooling identity and the path rule against a brute-force sample of the mixture."""
import math

import numpy as np

import predict_fit_ref as F
import predict_ref as R


def test_table_form_equals_dense_form_and_long_double():
    assert np.finfo(np.longdouble).eps < 1e-18
    w_dense, w_ld, big = F.fit_floor()
    print(f"mu_j, s_j: worst |dense - table| / max(1, |.|) over 2000 curves = {w_dense:.3e}; float64 against longdouble = {w_ld:.3e} "
          f"(largest |mu_j| = {big:.3e})")
    # both forms lose about cond(sigma^2 I + U U') <= 1 + |U|^2 / sigma^2 ~ 1e7 of the 1.1e-16 of a double at worst (as l does in 7m)
    assert w_dense < 1e-7 and w_ld < 1e-7


def _mixture_case(seed, M):
    """N = 4 draws of J = 6 samples on a grid of 3 rows: the tables of every (draw, sample), weights between 0.1 and 1"""
    rng = np.random.default_rng(seed)
    P, K, G, N, J = 12, 3, 3, 4, 6
    B = rng.uniform(0.0, 1.0, size=(9, P))
    E = rng.uniform(0.0, 1.0, size=(G, P))
    sig = 0.3
    draws = []
    y = None
    for t in range(N):
        th = R.directions(0.3 * rng.standard_normal((K, P)), 0.4 * rng.standard_normal((K, P, M)))
        if y is None:
            y = B @ (np.full(K, 1.0 / K) @ th[:, 0]) + math.sqrt(sig) * rng.standard_normal(B.shape[0])
        G_, s_, yy, n = R.record(B, y)
        Gam, tau = R.gamma_tables(G_, s_, th)
        draws.append(dict(Gam=Gam, tau=tau, e=F.e_table(E, th), z=rng.dirichlet(np.ones(K), size=J), w=rng.uniform(0.1, 1.0, size=J)))
    return draws, sig, G, M


def _check_moments(x, mean, sd, label):
    n = x.shape[0]
    se = sd / math.sqrt(n)
    dm = np.abs(x.mean(axis=0) - mean) / se
    dv = np.abs(x.var(axis=0) / sd ** 2 - 1.0) / math.sqrt(2.0 / n)
    print(f"{label}: |mean - ref| / se = {np.round(dm, 2)}, |var / ref - 1| / sqrt(2 / n) = {np.round(dv, 2)} (bound 5)")
    assert np.all(dm <= 5.0) and np.all(dv <= 5.0), label


def test_pooling_identity_and_path_rule_against_a_brute_force_mixture():
    n = 200_000
    for seed, M in ((1, 1), (2, 3)):
        draws, sig, G, M = _mixture_case(seed, M)
        N, J = len(draws), len(draws[0]["w"])
        mu = np.zeros((N, J, G)); s = np.zeros((N, J, G))
        for t, d in enumerate(draws):
            for j in range(J):
                mu[t, j], s[t, j] = F.fit_table(d["Gam"], d["tau"], d["e"], d["z"][j], sig)
        mt, vt = zip(*(F.mixture(d["w"], mu[t], s[t]) for t, d in enumerate(draws)))
        mean, sd = F.pooled_fit(np.array(mt), np.array(vt))
        # (i) samples of sum_t sum_j w~_j N(mu_j, s_j), the draws equally weighted
        rng = np.random.default_rng(100 + seed)
        tt = rng.integers(0, N, size=n)
        jj = np.zeros(n, dtype=np.int64)
        for t, d in enumerate(draws):
            sel = tt == t
            jj[sel] = rng.choice(J, size=int(sel.sum()), p=d["w"] / d["w"].sum())
        x = mu[tt, jj] + np.sqrt(s[tt, jj]) * rng.standard_normal((n, 1)) * np.ones(G)      # one normal a row: the marginals are what is pooled
        _check_moments(x, mean, sd, f"M = {M}, mixture samples")
        # (ii) the path rule: U picks j* in the cumulative weights, xi moves the scores
        rng = np.random.default_rng(200 + seed)
        tt = rng.integers(0, N, size=n)
        U = rng.uniform(size=n)
        xi = rng.standard_normal((n, M))
        paths = np.zeros((n, G))
        for t, d in enumerate(draws):
            sel = np.nonzero(tt == t)[0]
            js = np.searchsorted(np.cumsum(d["w"]), U[sel] * d["w"].sum(), side="right")
            assert all(js[i] == F.path_index(d["w"], U[sel[i]]) for i in range(50))
            for j in range(J):
                rows = sel[js == j]
                # the path is affine in xi: two evaluations a column give it for every row at once
                base = F.path_table(d["Gam"], d["tau"], d["e"], d["z"][j], sig, np.zeros(M))
                lin = np.stack([F.path_table(d["Gam"], d["tau"], d["e"], d["z"][j], sig, np.eye(M)[m]) - base for m in range(M)])
                paths[rows] = base + xi[rows] @ lin
        _check_moments(paths, mean, sd, f"M = {M}, path rule")


def test_single_sample_is_the_single_gaussian():
    """all samples equal: the mixture is the sample's Gaussian whatever the weights"""
    draws, sig, G, M = _mixture_case(3, 2)
    d = draws[0]
    mu, s = F.fit_table(d["Gam"], d["tau"], d["e"], d["z"][0], sig)
    mt, vt = F.mixture(d["w"], np.tile(mu, (6, 1)), np.tile(s, (6, 1)))
    np.testing.assert_allclose(mt, mu, rtol=1e-15, atol=0)
    np.testing.assert_allclose(vt, s, rtol=1e-14, atol=0)
