"""CPU checks of the numpy restatement of the prediction of held-out curves (tests/predict_ref.py): the Gamma form of
l(z) against the dense one, which gives the floor of the device tests' tolerance; the stage rule in float64 against np.longdouble,
which gives the floor of the proposal check; and the staged estimator against a quadrature where K = 2."""
import math

import numpy as np

import predict_ref as R


def test_gamma_form_equals_dense_form():
    worst, big = R.ell_floor()
    print(f"l(z): worst |dense - Gamma| / max(1, |l|) over 2000 curves = {worst:.3e} (largest |l| = {big:.3e})")
    # both forms lose about cond(sigma^2 I + U U') <= 1 + |U|^2 / sigma^2 ~ 1e7 of the 1.1e-16 of a double at worst
    assert worst < 1e-8


def test_stage_rule_float64_against_long_double():
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = R.rule_floor()
    print(f"stage rule: worst |float64 - longdouble| / max(1, |.|) over 600 inputs = {worst:.3e}")
    assert worst < 1e-9


def _k2_case():
    """K = 2, M = 2, P = 6, a curve of 6 points: l as a function of u = z_0, and the prior alpha_3 pi = (2, 3)"""
    rng = np.random.default_rng(5)
    K, M, P, n, sig = 2, 2, 6, 6, 0.25
    B = rng.uniform(0.0, 1.0, size=(n, P))
    th = R.directions(rng.standard_normal((K, P)), 0.4 * rng.standard_normal((K, P, M)))
    y = B @ (np.array([0.35, 0.65]) @ th[:, 0]) + math.sqrt(sig) * rng.standard_normal(n)
    G, s, yy, n = R.record(B, y)
    Gam, tau = R.gamma_tables(G, s, th)
    prior = np.array([2.0, 3.0])
    ell = lambda z: np.array([R.ell_gamma(Gam, tau, yy, n, zj, sig) for zj in z])
    return ell, prior


def test_staged_estimator_against_quadrature_k2():
    ell, prior = _k2_case()
    # log int_0^1 exp(l(u, 1 - u)) Beta(u; 2, 3) du by Gauss-Legendre (the integrand is smooth: polynomial prior, analytic l)
    x, w = np.polynomial.legendre.leggauss(400)
    u = 0.5 * (x + 1.0)
    lp = ell(np.stack([u, 1.0 - u], axis=1)) + (prior[0] - 1) * np.log(u) + (prior[1] - 1) * np.log1p(-u) - R.log_beta(prior)
    mx = lp.max()
    exact = mx + math.log(np.sum(0.5 * w * np.exp(lp - mx)))
    x2, w2 = np.polynomial.legendre.leggauss(200)
    u2 = 0.5 * (x2 + 1.0)
    lp2 = ell(np.stack([u2, 1.0 - u2], axis=1)) + (prior[0] - 1) * np.log(u2) + (prior[1] - 1) * np.log1p(-u2) - R.log_beta(prior)
    assert abs(exact - (lp2.max() + math.log(np.sum(0.5 * w2 * np.exp(lp2 - lp2.max()))))) < 1e-10      # the quadrature has converged
    J = 256
    for stages in (1, 3):
        devs = []
        for seed in range(8):
            out = R.staged_estimate(ell, prior, J, stages, np.random.default_rng(100 + seed))
            se = math.sqrt(max(1.0 / out["ess"] - 1.0 / J, 0.0))      # delta method: var(mean w) / mean(w)^2
            devs.append(abs(out["lpd"] - exact) / se)
            print(f"R = {stages}, seed {seed}: lpd = {out['lpd']:.6f} (exact {exact:.6f}), ess = {out['ess']:.1f}, |dev| / se = {devs[-1]:.2f}")
            assert out["ess"] > 20.0
        # room to spare: the bound is 5
        assert max(devs) < 5.0 and np.median(devs) < 2.0
