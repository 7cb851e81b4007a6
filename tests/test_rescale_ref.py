"""The long-double restatement of the rescale step (tests/rescale_ref.py) on the shipped Functional_trace (K = 2,
n = 40, 150 draws) with the identity permutation, against the numpy restatement of the reference's credible-interval functions
(oracle/post_ci.py, imported read-only): the transform is post_ci.transform_mat exactly; the rescaled memberships, cluster mean
functions and covariance values reproduce z_ci, f_mean_ci(rescale=True) and f_cov_ci(rescale=True) at the tolerance the project
uses for those functions (rtol 1e-11, atol 1e-12); Z~ nu~ = Z nu; rows of Z~ sum to 1; K = 2 keeps Z~ in the simplex; a relabelled
draw with the matching perm gives the same pure curves and the same A up to the column map.  No device."""
import os
import sys

import numpy as np
import pytest

import rescale_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import post_ci as O      # noqa: E402

TRACE = os.path.join(os.path.dirname(__file__), "golden", "Functional_trace") + "/"
RTOL, ATOL = 1e-11, 1e-12
LDEPS = float(np.finfo(np.longdouble).eps)


@pytest.fixture(scope="module")
def trace():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import api
    Z, nu = api.ReadCube(TRACE + "Z0.txt"), api.ReadCube(TRACE + "Nu0.txt")
    f = api.ReadFieldCube(TRACE + "Phi0.txt")
    Phi = np.stack([f[l, 0] for l in range(nu.shape[2])], axis=-1)      # (K, P, M, T)
    assert Z.shape == (40, 2, 150) and nu.shape == (2, 7, 150) and Phi.shape == (2, 7, 3, 150)
    draws = [R.draw(Z[:, :, j]) for j in range(Z.shape[2])]
    assert not any(d["singular"] for d in draws)
    rng = np.random.default_rng(12)
    return dict(Z=Z, nu=nu, Phi=Phi, draws=draws, B1=rng.standard_normal((9, 7)), B2=rng.standard_normal((5, 7)))


def test_transform_is_the_oracles_exactly(trace):
    for j, d in enumerate(trace["draws"]):
        assert d["A"].tobytes() == np.ascontiguousarray(O.transform_mat(trace["Z"][:, :, j])).tobytes(), j
        assert np.array_equal(d["curve"], [int(np.argmax(trace["Z"][:, k, j])) for k in range(2)]), j


def test_rescaled_memberships_reproduce_zci(trace):
    Z = trace["Z"]
    ref = O.z_ci(Z, 0.05, True, 0.0)
    zt = np.stack([np.asarray(R.z_tilde(Z[:, :, j], d["Ainv"]), dtype=np.float64) for j, d in enumerate(trace["draws"])], axis=-1)
    np.testing.assert_allclose(zt, ref["Z_trace"], rtol=RTOL, atol=ATOL)
    for i in range(Z.shape[0]):
        for k in range(2):
            q = O.arma_quantile(zt[i, k], [0.025, 0.5, 0.975])
            np.testing.assert_allclose(q, [ref["CI_Lower"][i, k], ref["CI_50"][i, k], ref["CI_Upper"][i, k]], rtol=RTOL, atol=ATOL)
    # rows sum to 1 and, for K = 2, stay in the simplex.  The stored rows of Z, and so those of A, sum to 1 within K u only:
    # A 1 = 1 + delta gives Z~ 1 = Z 1 - Z A^-1 delta, within K u (1 + |A^-1|_inf) of 1
    worst = 0.0
    for j, d in enumerate(trace["draws"]):
        ztl = R.z_tilde(Z[:, :, j], d["Ainv"])
        ninf = float(np.max(np.sum(np.abs(d["Ainv"]), axis=1)))
        assert np.all(np.abs(ztl.sum(axis=1) - 1) <= 2 * R.U * (1 + ninf)), j
        worst = min(worst, float(ztl.min()))
        assert d["z_min"] >= -4 * R.U, (j, d["z_min"])
    print(f"smallest rescaled membership over the trace {worst:.3e}, rcond from {min(d['rcond'] for d in trace['draws']):.3e} to "
          f"{max(d['rcond'] for d in trace['draws']):.3e}")


def test_mean_functions_reproduce_fmeanci(trace):
    Z, nu, B = trace["Z"], trace["nu"], trace["B1"]
    v = np.stack([np.asarray(R.mean_values(B, nu[:, :, j], d["A"])[0], dtype=np.float64) for j, d in enumerate(trace["draws"])])      # (T, K, G)
    for k in (1, 2):
        ref = O.f_mean_ci(nu, B, k, 0.05, True, False, 0.0, Z=Z)
        np.testing.assert_allclose(v[:, k - 1, :], ref["mean_trace"], rtol=RTOL, atol=ATOL)
        q = np.array([O.arma_quantile(v[:, k - 1, g], [0.025, 0.5, 0.975]) for g in range(B.shape[0])])
        for c, nm in enumerate(("CI_Lower", "CI_50", "CI_Upper")):
            np.testing.assert_allclose(q[:, c], ref[nm], rtol=RTOL, atol=ATOL, err_msg=nm)


def test_covariance_values_reproduce_fcovci(trace):
    Z, Phi, B1, B2 = trace["Z"], trace["Phi"], trace["B1"], trace["B2"]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    c = np.stack([np.asarray(R.cov_values(B1, B2, Phi[..., j], d["A"], pairs)[0], dtype=np.float64) for j, d in enumerate(trace["draws"])],
                 axis=-1)                                                                                  # (pairs, G1, G2, T)
    for r, (k, l) in enumerate(pairs):
        ref = O.f_cov_ci(Phi, B1, B2, k + 1, l + 1, 0.05, True, False, 0.0, Z=Z)
        np.testing.assert_allclose(c[r], ref["cov_trace"], rtol=RTOL, atol=ATOL)
        flat = c[r].reshape(B1.shape[0] * B2.shape[0], -1, order="F")
        q = np.array([O.arma_quantile(row, [0.025, 0.5, 0.975]) for row in flat])
        for col, nm in enumerate(("CI_Lower", "CI_50", "CI_Upper")):
            np.testing.assert_allclose(q[:, col].reshape(B1.shape[0], B2.shape[0], order="F"), ref[nm], rtol=RTOL, atol=ATOL, err_msg=nm)


def test_the_fit_does_not_change(trace):
    """Z~ nu~ = Z A^-1 A nu = Z nu, to the long-double inverse's error"""
    for j, d in enumerate(trace["draws"]):
        Z, nu = trace["Z"][:, :, j], trace["nu"][:, :, j]
        lhs = R.mix(Z, "Z", d["A"], d["Ainv"]) @ R.mix(nu, "nu", d["A"], d["Ainv"])
        rhs = np.asarray(Z, dtype=R.LD) @ np.asarray(nu, dtype=R.LD)
        scale = (np.abs(np.asarray(Z, dtype=R.LD)) @ np.abs(d["Ainv"])) @ (np.abs(np.asarray(d["A"], dtype=R.LD)) @ np.abs(np.asarray(nu, dtype=R.LD)))
        assert np.all(np.abs(lhs - rhs) <= 64 * LDEPS / d["rcond"] * scale), j


def test_inverse_is_an_inverse_and_singular_draws_are_flagged():
    rng = np.random.default_rng(3)
    for K in (1, 2, 3, 5, 8):
        A = rng.dirichlet(np.ones(K), size=K)
        Ai, sing = R.inverse(A)
        assert not sing
        assert np.max(np.abs(np.asarray(A, dtype=R.LD) @ Ai - np.eye(K))) <= 64 * K * LDEPS / R.rcond(A, Ai)
        np.testing.assert_allclose(np.asarray(Ai, dtype=np.float64), np.linalg.inv(A), rtol=0, atol=R.inverse_bound(A, Ai))
    A = rng.dirichlet(np.ones(3), size=3)
    A[2] = A[0]                                   # two components share their pure curve
    d = R.draw(rng.dirichlet(np.ones(3), size=10), given=A)
    assert d["singular"] and d["rcond"] == 0.0 and np.isnan(d["z_min"]) and np.all(np.isnan(np.asarray(d["Ainv"], dtype=np.float64)))
    A[1, 1] = np.inf
    assert R.inverse(A)[1]
    # a zero on the diagonal is not singular: the pivot search finds the row
    Ai, sing = R.inverse(np.array([[0.0, 1.0], [1.0, 0.0]]))
    assert not sing and np.array_equal(np.asarray(Ai, dtype=np.float64), [[0.0, 1.0], [1.0, 0.0]])


def test_first_maximum_and_nan():
    Z = np.array([[0.2, 0.5, 0.3], [0.6, 0.1, 0.3], [0.6, 0.5, np.nan], [0.1, 0.2, 0.7]])
    assert np.array_equal(R.curve_rule(Z), [1, 0, 3])
    assert np.array_equal(R.curve_rule(Z, [2, 0, 1]), [3, 1, 0])


def test_relabelled_draw_with_matching_perm(trace):
    """b's column j is a's column sigma[j]; with perm_b = argsort(sigma) b's aligned component k is a's k: the same pure curves, and
    A_b[k][c] = A_a[k][sigma[c]]; the rescaled memberships agree entry for entry in the aligned labelling"""
    rng = np.random.default_rng(5)
    for K in (2, 3, 5):
        Za = rng.dirichlet(np.ones(K) * 0.4, size=37)
        sigma = rng.permutation(K)
        Zb = Za[:, sigma]
        pb = np.argsort(sigma)
        a, b = R.draw(Za), R.draw(Zb, pb)
        assert np.array_equal(a["curve"], b["curve"])
        assert b["A"].tobytes() == np.ascontiguousarray(a["A"][:, sigma]).tobytes()
        za, zb = R.z_tilde(Za, a["Ainv"]), R.z_tilde(Zb, b["Ainv"])
        assert np.max(np.abs(za - zb)) <= 64 * K * LDEPS / a["rcond"] * max(1.0, float(np.max(np.abs(za))))
