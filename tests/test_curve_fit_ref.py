"""CPU checks of the restatement the device tests of the pooled per-curve fitted functions compare with (tests/curve_fit_ref.py;
DESIGN.md 7e): its float64 form against np.longdouble within its own bound, the two invariances that let the chains pool, the
quantile rule on k_bands_quantiles' documented cases, and the two new entries of the C ABI."""
import os
import re

import numpy as np
import pytest

import curve_fit_ref as R

P, K, M = 12, 3, 3


def _draws(D, seed, n=10, S=10, G=10):
    rng = np.random.default_rng(seed)
    Z = rng.dirichlet(np.full(K, 0.7), size=(n, S)).transpose(0, 2, 1)          # (n, K, S)
    Z[rng.uniform(size=Z.shape) < 0.3] = 0.0                                     # exact zeros, as the sampler's Z rows have
    d = dict(E=rng.standard_normal((G, P)), Z=Z, chi=rng.standard_normal((n, M, S)), nu=rng.standard_normal((K, P, S)),
             Phi=0.5 * rng.standard_normal((K, P, M, S)))
    if D:
        d.update(X=rng.standard_normal((n, D)), eta=rng.standard_normal((P, D, K, S)), xi=0.3 * rng.standard_normal((P, D, M, K, S)),
                 covariance_adj=True)
    return d


@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("which", ["mean", "fit"])
def test_float64_restatement_is_within_its_bound_of_longdouble(D, which):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    d = _draws(D, 5 + D)
    v = R.draw_values(which=which, **d)
    assert v.size == 1000                                                        # x 2 values of D: 2000 (curve, grid point, draw) cases
    ref = R.draw_values(which=which, dtype=np.longdouble, **d)
    b = 2.0 * R.n_terms(P, K, M, D) * 2.0 ** -52 * R.draw_values(which=which, absolute=True, **d)
    err = np.abs(v.astype(np.longdouble) - ref).astype(np.float64)
    print(f"D={D} {which}: worst |float64 - longdouble| / bound = {np.max(err[b > 0] / b[b > 0]):.3e}")
    assert np.count_nonzero(b > 0) > 900                                         # (a Z row of zeros alone gives an exact 0)
    assert np.all(err <= b)
    # the reference alone uses only half of the bound's factor 2 at the very most
    assert np.all(err <= 0.5 * b)


@pytest.mark.parametrize("D", [0, 2])
def test_label_permutation_within_bound_and_sign_flip_exact(D):
    d = _draws(D, 11 + D)
    for which in ("mean", "fit"):
        v = R.draw_values(which=which, **d)
        b = 2.0 * R.n_terms(P, K, M, D) * 2.0 ** -52 * R.draw_values(which=which, absolute=True, **d)
        perm = [2, 0, 1]
        p = dict(d, Z=d["Z"][:, perm], nu=d["nu"][perm], Phi=d["Phi"][perm])
        if D:
            p.update(eta=d["eta"][:, :, perm], xi=d["xi"][:, :, :, perm])
        vp = R.draw_values(which=which, **p)
        assert np.all(np.abs(vp - v) <= b)
        f = dict(d, chi=d["chi"].copy(), Phi=d["Phi"].copy())
        f["chi"][:, 1] *= -1.0
        f["Phi"][:, :, 1] *= -1.0
        if D:
            f["xi"] = d["xi"].copy()
            f["xi"][:, :, 1] *= -1.0
        vf = R.draw_values(which=which, **f)
        assert np.array_equal(vf, v)
    # the fit does depend on chi: the flip of chi alone changes it
    g = dict(d, chi=-d["chi"])
    assert not np.array_equal(R.draw_values(which="fit", **g), R.draw_values(which="fit", **d))


def test_quantile_rule_documented_cases():
    rng = np.random.default_rng(3)
    # N = 1: every probability gives the draw
    one = np.array([[2.5]])
    assert np.array_equal(R.quantiles(one, [0.0, 0.3, 0.5, 1.0]), [[2.5, 2.5, 2.5, 2.5]])
    for N in (2, 5, 8, 92, 4000):
        v = rng.standard_normal((3, N))
        s = np.sort(v, axis=-1)
        q = R.quantiles(v, [0.0, 0.5 / N * 0.999, 0.5, 1.0 - 0.5 / N * 0.999, 1.0])
        # the extremes: below 0.5 / N the smallest draw, above (N - 0.5) / N the largest
        assert np.array_equal(q[:, 0], s[:, 0]) and np.array_equal(q[:, 1], s[:, 0])
        assert np.array_equal(q[:, 4], s[:, -1]) and np.array_equal(q[:, 3], s[:, -1])
        # the median: the middle draw (odd N), the mean of the middle two (even N; w = 1/2 up to the rounding of p_k)
        if N % 2:
            np.testing.assert_allclose(q[:, 2], s[:, N // 2], rtol=0, atol=1e-13)
        else:
            np.testing.assert_allclose(q[:, 2], 0.5 * s[:, N // 2 - 1] + 0.5 * s[:, N // 2], rtol=0, atol=1e-13)
        # p_k = (k - 0.5) / N is the k-th smallest draw; linear in between
        for k in (1, 2, N // 2 + 1, N):
            np.testing.assert_allclose(R.quantiles(v, [(k - 0.5) / N])[:, 0], s[:, k - 1], rtol=0, atol=1e-13)
        if N >= 3:
            p = (1.25 - 0.5) / N * 1.0 + 0.0                                   # a quarter of the way from s[0] to s[1]
            np.testing.assert_allclose(R.quantiles(v, [p])[:, 0], 0.75 * s[:, 0] + 0.25 * s[:, 1], rtol=0, atol=1e-13)
        # Hyndman and Fan definition 5 is numpy's "hazen"
        pr = [0.025, 0.1, 0.37, 0.5, 0.9, 0.975]
        np.testing.assert_allclose(R.quantiles(v, pr), np.quantile(v, pr, axis=-1, method="hazen").T, rtol=0, atol=1e-12)


def test_moments_of_one_draw():
    m, s = R.moments(np.array([[1.5], [2.0]]))
    assert np.array_equal(m, [1.5, 2.0]) and np.all(np.isnan(s))


def test_new_symbols_are_declared():
    from bayesfmmm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    declared = set(re.findall(r"\b(bfmmm_[a-z_0-9]+)\s*\(", hdr))
    for name in ("bfmmm_chain_curve_fit", "bfmmm_chain_curve_bands"):
        assert name in _lib.SYMBOLS, name
        assert name in declared, name
