"""The long-double restatement of stacking (tests/stacking_ref.py) against what the method promises: the certificate
f(w*) - f(w) <= n gap(w) at every iterate the stopping rule looks at, the optimum against scipy's SLSQP, equivariance under a
permutation of the candidates, a per-unit constant, a dominating and a duplicated candidate; the wrong forms (`mutate`) fail those
checks; and the bound tests/test_gpu_stacking.py puts on the device's weights, measured here from the two float64 twins."""
import numpy as np
import pytest

import stacking_ref as R

LD = R.LD


def _plain(n, Q, seed):
    """finite columns of differing quality: no offsets, so that SLSQP and the mutations see an ordinary problem"""
    rng = np.random.default_rng(seed)
    return -1.0 + rng.standard_normal((n, Q)) * rng.uniform(0.3, 1.5, size=Q) - rng.uniform(0.0, 0.5, size=Q)


@pytest.mark.parametrize("n,Q,seed", [(200, 3, 1), (257, 8, 2), (64, 17, 3)])
def test_certificate_holds_at_every_checked_iterate(n, Q, seed):
    L, init = R.simulate(n, Q, seed)
    long_run = R.em(L, init, max_iter=200000, check_every=16, tol=1e-13)
    assert long_run["converged"]
    run = R.em(L, init, max_iter=long_run["n_iter"], check_every=16, tol=0.0)
    assert len(run["history"]) >= 2
    for t, gap, f in run["history"]:
        short = long_run["objective"] - f
        assert -1e-15 * abs(float(f)) <= short <= n * gap, (t, float(short), float(n * gap))
    # monotone in f, the weights on the simplex
    fs = [float(h[2]) for h in run["history"]]
    assert all(b >= a - 1e-12 * abs(a) for a, b in zip(fs, fs[1:]))
    assert abs(float(np.sum(long_run["weights"])) - 1.0) < 1e-15 * Q and np.all(long_run["weights"] >= 0)


def test_optimum_matches_slsqp():
    from scipy.optimize import minimize
    L = _plain(300, 3, 5)
    ref = R.em(L, max_iter=200000, tol=1e-13)
    E = np.exp(L - L.max(axis=1, keepdims=True))
    res = minimize(lambda w: -np.sum(np.log(E @ w)), np.full(3, 1 / 3), jac=lambda w: -(E / (E @ w)[:, None]).sum(axis=0), method="SLSQP",
                   bounds=[(0, 1)] * 3, constraints=[{"type": "eq", "fun": lambda w: w.sum() - 1, "jac": lambda w: np.ones(3)}],
                   options={"ftol": 1e-14, "maxiter": 500})
    assert res.success
    f_slsqp = -res.fun + np.sum(L.max(axis=1))
    # SLSQP cannot beat the certified optimum by more than the certificate, and reaches it to its own accuracy
    assert f_slsqp - float(ref["objective"]) <= 300 * float(ref["gap"]) + 1e-9
    assert float(ref["objective"]) - f_slsqp <= 1e-6
    np.testing.assert_allclose(res.x, ref["weights"].astype(float), atol=2e-4)


def test_permutation_constant_dominating_and_duplicated_columns():
    L = _plain(150, 4, 7)
    base = R.em(L, max_iter=64, tol=0.0)
    perm = np.array([2, 0, 3, 1])
    p = R.em(L[:, perm], max_iter=64, tol=0.0)
    np.testing.assert_allclose(p["weights"].astype(float), base["weights"][perm].astype(float), rtol=0, atol=1e-17)
    assert abs(float(p["objective"] - base["objective"])) <= 1e-15 * abs(float(base["objective"]))
    # a constant per unit moves pointwise by that constant and nothing else (the constants are exact in float64)
    c = np.round(np.random.default_rng(8).uniform(-50, 50, size=150))
    s = R.em(L + c[:, None], max_iter=64, tol=0.0)
    np.testing.assert_allclose(s["weights"].astype(float), base["weights"].astype(float), rtol=0, atol=1e-13)
    np.testing.assert_allclose((s["pointwise"] - base["pointwise"]).astype(float), c, rtol=0, atol=1e-11)
    assert abs(float(s["gap"] - base["gap"])) < 1e-12
    # a candidate that is best on every unit takes all the weight
    D = L.copy()
    D[:, 1] = L.max(axis=1) + 0.5
    d = R.em(D, max_iter=100000, tol=1e-10)
    assert d["converged"] and float(d["weights"][1]) > 1 - 1e-6
    # two identical candidates share the weight the single one gets; the objective does not move
    one = R.em(L, max_iter=100000, tol=1e-12)
    two = R.em(np.concatenate([L, L[:, :1]], axis=1), max_iter=100000, tol=1e-12)
    assert abs(float(two["weights"][0] + two["weights"][4] - one["weights"][0])) < 1e-5
    assert abs(float(two["objective"] - one["objective"])) <= 150 * 2e-12


def test_mutations_are_caught():
    L, init = R.simulate(90, 3, 11)          # rows near -1e5 and +700
    good = R.em(L, init, max_iter=400, tol=0.0)
    assert np.all(np.isfinite(good["weights"].astype(float))) and abs(float(np.sum(good["weights"])) - 1) < 1e-15
    # no row maximum: exp(-1e5) is 0 in every format, the rows near -1e5 have d = 0
    with np.errstate(all="ignore"):
        bad = R.em(L, init, max_iter=4, tol=0.0, mutate="no_row_max")
    assert not np.all(np.isfinite(bad["weights"].astype(float)))
    # division by Q in place of n: the iterate leaves the simplex
    bad = R.em(L, init, max_iter=1, tol=0.0, mutate="div_by_Q")
    assert abs(float(np.sum(bad["weights"])) - 90 / 3) < 1e-9
    # the gap of the iterate before the returned one: it is not the gap of the returned weights
    P = _plain(120, 3, 12)
    right = R.em(P, max_iter=16, check_every=16, tol=0.0)
    wrong = R.em(P, max_iter=16, check_every=16, tol=0.0, mutate="gap_before")
    at = R.evaluate(P, right["weights"])
    assert right["gap"] == at["gap"] and wrong["gap"] != at["gap"] and wrong["gap"] > right["gap"]
    # se_diff from unpaired variances: two candidates that differ by a constant have a paired se of 0
    M = np.stack([P[:, 0], P[:, 0] - 0.25, P[:, 1]], axis=1)
    tab, mut = R.compare_table(M), R.compare_table(M, mutate="unpaired")
    assert tab["best"] == 0 and float(tab["se_diff"][1]) < 1e-12 and abs(float(tab["elpd_diff"][1]) + 0.25 * 120) < 1e-10
    assert float(mut["se_diff"][1]) > 1.0
    assert tab["se_diff"][0] == 0 and tab["elpd_diff"][0] == 0 and abs(float(np.sum(tab["pseudo_bma"])) - 1) < 1e-15


def test_the_refusals_name_the_first_offender():
    L = _plain(10, 3, 13)
    for val, at in ((np.nan, (4, 1)), (np.inf, (2, 2))):
        B = L.copy()
        B[at] = val
        B[7, 0] = val
        with pytest.raises(ValueError, match=f"2 offending entries or units, the first at unit {at[0]}, candidate {at[1]}"):
            R.prepare(B)
    B = L.copy()
    B[6] = -np.inf
    with pytest.raises(ValueError, match="1 offending entries or units, the first at unit 6, candidate 0"):
        R.prepare(B)
    B = L.copy()
    B[6, :2] = -np.inf          # -inf is an entry like any other
    assert np.all(R.prepare(B)[1][6] == [0, 0, 1])


def test_the_bound_of_the_gpu_test():
    """The twins' errors, and so the bound, at the GPU test's shapes: the device may differ from long double by 8 x what two
    float64 orders of the same sum differ by.  A sum of n terms in [0, 1 / w] of float64 carries at most n eps / 2 relative
    error in any order, an iterate after t steps at most t times that and its own roundings: the bound must stay below
    8 t (n + 8) eps, or the twins are not what they claim to be."""
    for n, Q, seed in [(257, 3, 0), (65, 17, 1), (63, 64, 2), (R.SMALL_N[0], 2, 3), (4099, 8, 4)]:
        L, init = R.simulate(n, Q, seed)
        for t, (w, bound) in R.weights_bound(L, init).items():
            print(f"n={n} Q={Q} iterations={t}: bound {bound:.3e} ({bound / R.EPS:.0f} eps)")
            assert 64 * R.EPS <= bound <= max(64.0, 8.0 * t * (n + 8)) * R.EPS
            assert abs(float(np.sum(w)) - 1) < 1e-15
