"""The long-double restatement of the slot log-likelihood (tests/slot_ll_ref.py) against what is independent of
it: the oracle's post_llik (oracle/post.c, the reference's loops) on the chain the reference ships and on a simulated chain with
and without covariates, its own fp64 record route (what the kernel evaluates), and the multivariate formula's integer division."""
import os

import numpy as np
import pytest

import oracle_lib as O
import slot_ll_ref as R
from simdata import simulate_functional, truth_chain

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRACE = os.path.join(GOLD, "Functional_trace") + "/"


def _chain_dict(ch, D):
    d = dict(nu=ch.nu, Phi=ch.Phi, Z=ch.Z, chi=ch.chi, sigma_sq=ch.sigma)
    if D:
        d.update(eta=ch.eta, xi=ch.xi)
    return d


def _perturbed(sim, T, seed):
    """the truth chain with every draw moved a little, so that the draws differ"""
    model, ch = truth_chain(sim, T)
    rng = np.random.default_rng(seed)
    for a, s in ((ch.nu, 0.05), (ch.Phi, 0.02), (ch.chi, 0.1)) + (((ch.eta, 0.02), (ch.xi, 0.01)) if sim["D"] else ()):
        a += s * rng.standard_normal(a.shape)
    ch.Z[:] = rng.dirichlet(np.ones(sim["K"]), size=(sim["n"], T)).transpose(0, 2, 1)
    ch.sigma[:] = sim["sigma_sq"] * rng.uniform(0.5, 2.0, T)
    return model, ch


@pytest.mark.parametrize("D", [0, 2])
def test_matches_oracle_on_a_simulated_chain(D):
    __import__("__graft_entry__").build()
    sim = simulate_functional(n=17, M=2, sigma_sq=0.01, seed=12, ragged=True, D=D)
    T = 4
    model, ch = _perturbed(sim, T, 3)
    X = sim["X"] if D else None
    cur = R.curve_matrix(sim["y"], sim["B"], [_chain_dict(ch, D)], 0, T, X=X, covariance_adj=True)
    ref = O.post_llik(model, ch)
    got = R.totals(cur)[0].astype(np.float64)
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    # the fp64 record route against the dense form, curve by curve: yy - 2 theta's + theta'G theta cancels to rss, which costs
    # eps yy / (2 sigma^2) a curve at most (a few times: three terms of that size)
    rec = R.curve_matrix(sim["y"], sim["B"], [_chain_dict(ch, D)], 0, T, X=X, covariance_adj=True, route=R.record_curve)
    yy = np.array([float(np.dot(y, y)) for y in sim["y"]])
    tol = 16 * np.finfo(np.float64).eps * (yy[:, None, None] / (2 * ch.sigma[None, None, :]) + np.abs(cur.astype(np.float64)))
    assert np.all(np.abs((rec - cur).astype(np.float64)) <= tol)
    if D:      # eta and xi enter: without them the value moves
        plain = R.curve_matrix(sim["y"], sim["B"], [_chain_dict(ch, 0)], 0, T)
        mean_only = R.curve_matrix(sim["y"], sim["B"], [_chain_dict(ch, D)], 0, T, X=X, covariance_adj=False)
        assert np.abs((plain - cur).astype(np.float64)).max() > 1.0 and np.abs((mean_only - cur).astype(np.float64)).max() > 1e-3


@pytest.mark.parametrize("with_x,cov_adj", [(False, False), (True, False), (True, True)])
def test_matches_oracle_on_the_shipped_chain(with_x, cov_adj):
    __import__("__graft_entry__").build()
    from rds_reader import read_rds
    from test_gpu_post import _oracle_chain
    Y = [np.asarray(v).reshape(-1) for v in read_rds(os.path.join(GOLD, "Sim_data.RDS"))]
    t = [np.asarray(v).reshape(-1) for v in read_rds(os.path.join(GOLD, "time.RDS"))]
    e = dict(y=Y, t=t, boundary_knots=[0.0, 1000.0], internal_knots=[250.0, 500.0, 750.0], n=40)
    X = np.random.default_rng(7).standard_normal((40, 1)) if with_x else None
    model, ch, B = _oracle_chain(e, X, TRACE, 1, cov_adj)
    T = 150
    cur = R.curve_matrix(Y, B, [_chain_dict(ch, 1 if with_x else 0)], 0, T, X=X, covariance_adj=cov_adj)
    ref = O.post_llik(model, ch)
    got = R.totals(cur)[0].astype(np.float64)
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"shipped chain with_x={with_x} cov_adj={cov_adj}: largest relative difference to the oracle {rel.max():.2e}")
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    rec = R.totals(R.curve_matrix(Y, B, [_chain_dict(ch, 1 if with_x else 0)], 0, T, X=X, covariance_adj=cov_adj, route=R.record_curve))
    diff = np.abs((rec[0] - R.totals(cur)[0]).astype(np.float64))
    print(f"  record route (fp64) against the dense form: largest relative difference {(diff / np.abs(ref)).max():.2e}")
    # what the record route may lose: its three terms yy, 2 theta's and theta'G theta, each rounded (a few eps: sums of n_i and of
    # P products), cancel to rss and are divided by 2 sigma^2; |theta's| <= sqrt(yy ff), theta'G theta = ff = |B theta|^2
    chd = _chain_dict(ch, 1 if with_x else 0)
    eps = np.finfo(np.float64).eps
    for s in range(T):
        th = R.theta(X=X, dtype=np.float64, **R._draw(chd, s, with_x, cov_adj))
        mag = sum(float(y @ y) + 2 * np.sqrt(float(y @ y) * float((b @ h) @ (b @ h))) + float((b @ h) @ (b @ h)) for y, b, h in zip(Y, B, th))
        assert diff[s] <= 16 * eps * mag / (2 * ch.sigma[s]) + 4 * eps * abs(ref[s]), s


def test_multivariate_integer_division_bites_for_odd_P():
    rng = np.random.default_rng(5)
    n, P, K, M, T = 6, 5, 2, 2, 3
    Y = rng.standard_normal((n, P))
    ch = dict(nu=rng.standard_normal((K, P, T)), Phi=0.1 * rng.standard_normal((K, P, M, T)),
              Z=rng.dirichlet(np.ones(K), size=(n, T)).transpose(0, 2, 1), chi=rng.standard_normal((n, M, T)),
              sigma_sq=rng.uniform(0.5, 2.0, T))
    cur = R.curve_matrix(list(Y), None, [ch], 0, T)
    for s in range(T):
        th = R.theta(ch["nu"][..., s], ch["Phi"][..., s], ch["Z"][..., s], ch["chi"][..., s], dtype=np.float64)
        s2 = ch["sigma_sq"][s]
        for i in range(n):
            rss = np.sum((Y[i] - th[i]) ** 2)
            want = -(2 * np.log(2 * np.pi * s2)) - rss / (2 * s2)            # P // 2 = 2, not 2.5
            density = -(2.5 * np.log(2 * np.pi * s2)) - rss / (2 * s2)
            assert abs(float(cur[i, 0, s]) - want) <= 1e-13 * (1 + abs(want))
            assert abs(float(cur[i, 0, s]) - density) > 0.1
    rec = R.curve_matrix(list(Y), None, [ch], 0, T, route=R.record_curve)
    assert np.abs((rec - cur).astype(np.float64)).max() <= 1e-12 * np.abs(cur.astype(np.float64)).max()
