"""The restatements of the observation-level leave-one-out quantities (tests/loo_pointwise_ref.py) against each other on the CPU:
explicit conditioning on the dense n_i x n_i covariance and the leverage form k_loo_pointwise evaluates.  The worst
differences are the floors the forms themselves impose; the GPU tests hold the kernel to ten times them (GPU_TOL_*).  The device is
not consulted here."""
import numpy as np

import curve_ll_ref as CL
import loo_pointwise_ref as R
import psis_ref
from test_curve_ll_ref import _random_curve


def test_leverage_and_dense_forms_agree():
    rng = np.random.default_rng(20250)
    P, M, K = 12, 3, 3
    names = ("l", "m", "sqrt v", "z")
    worst, at = [0.0] * 4, [None] * 4
    for it in range(2000):
        D = 0 if it % 2 == 0 else 2
        y, B, sigma_sq, z, nu, Phi, x, eta, xi = _random_curve(rng, P, M, K, D)
        c, V = CL.coefficients(z, nu, Phi, x, eta, xi)
        dl, dm, dv, dz = R.dense(y, B, c, V, sigma_sq)
        ll, lm, lv, lz = R.leverage(y, B, c, V, sigma_sq, B.T @ B, B.T @ y)
        assert np.all(lv > 0) and np.all(dv > 0)
        for q, (a, b) in enumerate(((ll, dl), (lm, dm), (np.sqrt(lv), np.sqrt(dv)), (lz, dz))):
            e = float(R.rel_diff(a, b).max())
            if e > worst[q]:
                worst[q], at[q] = e, (it, len(y), sigma_sq)
    for q in range(4):
        print(f"worst |leverage - dense| / max(1, |.|) of {names[q]} over 2000 curves: {worst[q]:.3e} at (index, n_i, sigma^2) = {at[q]}")
    # The dense covariance without row and column j has condition number up to (sigma^2 + lambda_max(UU')) / sigma^2, about 1e7 here,
    # and its solve loses that factor times the unit roundoff in m and v; l and z divide the residual by sqrt(v) >= sigma >= 1e-2 and
    # square it: 1e7 x 1.1e-16 x 1e2 = 1e-7 bounds all four.
    assert max(worst) < 1e-7
    # the recorded floors are what this run measures (same seed, same order of magnitude)
    for w, floor in zip(worst, (R.FORM_FLOOR_L, R.FORM_FLOOR_M, R.FORM_FLOOR_SD, R.FORM_FLOOR_Z)):
        assert floor / 3.0 < w < 3.0 * floor, (worst, floor)
    assert (R.GPU_TOL_L, R.GPU_TOL_M, R.GPU_TOL_SD, R.GPU_TOL_Z) == tuple(10.0 * f for f in (R.FORM_FLOOR_L, R.FORM_FLOOR_M, R.FORM_FLOOR_SD,
                                                                                             R.FORM_FLOOR_Z))


def test_single_observation_curve_is_the_curve_density():
    """n_i = 1: nothing is left to condition on, so l is the marginal log-density of the curve"""
    rng = np.random.default_rng(7)
    seen = 0
    while seen < 20:
        y, B, sigma_sq, z, nu, Phi, x, eta, xi = _random_curve(rng, 12, 3, 3, 2 if seen % 2 else 0)
        y, B = y[:1], B[:1]
        c, V = CL.coefficients(z, nu, Phi, x, eta, xi)
        ref = CL.dense(y, B, c, V, sigma_sq)
        for form in (R.dense, R.leverage):
            l, m, v, zz = form(y, B, c, V, sigma_sq)
            assert l.shape == (1,)
            # omega = 1 - h = sigma^2 / (sigma^2 + |w|^2) >= 1e-4 / 100 here (|w|^2 stays below 100), and the subtraction loses
            # eps / omega of it: 1.1e-16 x 1e6, doubled for the quadratic term
            assert float(R.rel_diff(l[0], ref)) < 2.2e-10
            # the conditional mean is the marginal one; the leverage form reaches it as y - e / omega, to its floor
            assert float(R.rel_diff(m[0], (B @ c)[0])) < 3.0 * R.FORM_FLOOR_M
        seen += 1


def test_expect_of_a_constant_and_of_the_likelihood():
    rng = np.random.default_rng(3)
    for S in (24, 400, 5000):                           # S = 24: no smoothing (L < 5)
        for ll in (rng.standard_normal(S) * 0.7 - 3.0, -np.log(((1 - rng.random(S)) ** -0.7 - 1) / 0.7) - 4.0):
            assert abs(R.expect(ll, np.full(S, 2.5)) - 2.5) < 1e-12
            e = R.expect(ll, np.vstack([np.exp(ll), np.ones(S)]))
            assert e.shape == (2,)
            assert abs(np.log(e[0]) - psis_ref.psis_row(ll)["elpd_loo"]) < 1e-12


def test_norm_cdf():
    np.testing.assert_allclose(R.norm_cdf([0.0, 1.959963984540054, -1.959963984540054]), [0.5, 0.975, 0.025], rtol=0, atol=1e-15)
