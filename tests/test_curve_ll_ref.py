"""The two restatements of the per-curve marginal log-density (tests/curve_ll_ref.py) against each other on the CPU: the
dense n_i x n_i form and the sufficient-statistic form k_chain_curve_ll evaluates.  The worst difference is
the floor the forms themselves impose; the GPU tests hold the kernel to ten times it (curve_ll_ref.GPU_TOL)."""
import numpy as np

import curve_ll_ref as R


def _random_curve(rng, P, M, K, D):
    ni = int(rng.integers(1, 121))                      # includes n_i < M
    B = np.zeros((ni, P))
    for l in range(ni):                                 # sparse rows: a window of at most four basis functions
        lo = int(rng.integers(0, P - 3))
        B[l, lo:lo + 4] = rng.uniform(0.0, 1.0, 4) * (rng.uniform(size=4) < 0.85)
    sigma_sq = float(10.0 ** rng.uniform(-4.0, 0.0))
    z = rng.dirichlet(np.full(K, 0.7))
    if rng.uniform() < 0.3:                             # exact zeros on the simplex
        z[int(rng.integers(0, K))] = 0.0
        z = z / z.sum() if z.sum() > 0 else np.eye(K)[0]
    nu = rng.standard_normal((K, P)) * 2.0
    Phi = rng.standard_normal((K, P, M)) * np.array([1.0, 0.5, 0.25])[:M]
    x = eta = xi = None
    if D > 0:
        x = rng.standard_normal(D)
        eta = rng.standard_normal((P, D, K))
        xi = 0.3 * rng.standard_normal((P, D, M, K))
    y = B @ rng.standard_normal(P) * 2.0 + np.sqrt(sigma_sq) * rng.standard_normal(ni)
    return y, B, sigma_sq, z, nu, Phi, x, eta, xi


def test_dense_and_sufficient_statistic_forms_agree():
    rng = np.random.default_rng(20240)
    P, M, K = 12, 3, 3
    worst, worst_at = 0.0, None
    for it in range(2000):
        D = 0 if it % 2 == 0 else 2
        y, B, sigma_sq, z, nu, Phi, x, eta, xi = _random_curve(rng, P, M, K, D)
        c, V = R.coefficients(z, nu, Phi, x, eta, xi)
        a = R.dense(y, B, c, V, sigma_sq)
        b = R.suffstat(B.T @ B, B.T @ y, float(y @ y), len(y), c, V, sigma_sq)
        e = float(R.rel_diff(b, a))
        if e > worst:
            worst, worst_at = e, (it, len(y), sigma_sq, a)
    print(f"worst |dense - suffstat| / max(1, |l|) over 2000 curves: {worst:.3e} at (index, n_i, sigma^2, l) = {worst_at}")
    # The dense covariance has condition number (sigma^2 + lambda_max(UU')) / sigma^2, up to about 1e7 here; slogdet and solve
    # lose that factor times the unit roundoff in the quadratic form, which dominates l: 1e7 x 1.1e-16 = 1e-9.
    assert worst < 1e-9
    # the recorded floor is what this run measures (same seed, same order of magnitude)
    assert worst < 3.0 * R.FORM_FLOOR, worst


def test_mean_adjusted_only_ignores_xi():
    rng = np.random.default_rng(5)
    y, B, sigma_sq, z, nu, Phi, x, eta, xi = _random_curve(rng, 12, 3, 3, 2)
    c0, V0 = R.coefficients(z, nu, Phi, x, eta, None)
    c1, V1 = R.coefficients(z, nu, Phi, x, eta, xi)
    np.testing.assert_array_equal(c0, c1)
    assert np.max(np.abs(V0 - V1)) > 0
    np.testing.assert_allclose(V0, np.einsum("k,kpm->pm", z, Phi), rtol=1e-14, atol=1e-14)
