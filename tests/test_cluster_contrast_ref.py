"""The restatement of the contrast call (tests/cluster_contrast_ref.py) against what is already tested, and
sampler.contrast_plan on every spelling with its refusals.  No device."""
import numpy as np
import pytest

import cluster_contrast_ref as CR
import rescale_ref as R
from bayesfmmm_amd.sampler import contrast_plan


def _draw(rng, K=3, P=8, D=2, G=5):
    A = rng.dirichlet(np.full(K, 1.5), size=K) + np.eye(K)
    return dict(A=A, nu=rng.standard_normal((K, P)), eta=rng.standard_normal((P, D, K)), E=rng.standard_normal((G, P)))


# ---- contrast_plan ---------------------------------------------------------------------------------------------------------------
def test_plan_pairwise_and_effects():
    wn, we = contrast_plan(4, 0, "pairwise")
    assert we is None and wn.shape == (6, 4)
    pairs = [(k, l) for k in range(4) for l in range(k + 1, 4)]
    for r, (k, l) in enumerate(pairs):
        want = np.zeros(4)
        want[k], want[l] = 1.0, -1.0
        assert np.array_equal(wn[r], want)
    wn, we = contrast_plan(3, 2, "pairwise")
    assert wn.shape == (3, 3) and we.shape == (3, 3, 2) and not we.any()
    wn, we = contrast_plan(3, 2, "effects")
    assert wn.shape == (6, 3) and not wn.any() and we.shape == (6, 3, 2) and we.sum() == 6.0
    for k in range(3):
        for d in range(2):
            assert we[k * 2 + d, k, d] == 1.0
    assert contrast_plan(2, 0)[0].tolist() == [[1.0, -1.0]]      # the default spelling


def test_plan_lists_and_dicts():
    x, x2 = np.array([0.5, -2.0]), np.array([1.5, 0.25])
    wn, we = contrast_plan(3, 2, [[(1, 0), (-1, 2)], [(1, 1, x), (-1, 1, x2)], [(2.0, 0, x), (-1, 1), (-1, 2, x2)], [(1, 0), (1, 0)]])
    assert wn.tolist() == [[1, 0, -1], [0, 0, 0], [2, -1, -1], [2, 0, 0]]
    assert not we[0].any() and np.array_equal(we[1, 1], x - x2) and not we[1, [0, 2]].any()
    assert np.array_equal(we[2, 0], 2.0 * x) and np.array_equal(we[2, 2], -x2) and not we[2, 1].any()
    wn, we = contrast_plan(3, 0, [[(1, 2)]])
    assert wn.tolist() == [[0, 0, 1]] and we is None
    a, b = np.arange(6.0).reshape(2, 3), np.arange(12.0).reshape(2, 3, 2)
    wn, we = contrast_plan(3, 2, {"nu": a, "eta": b})
    assert np.array_equal(wn, a) and np.array_equal(we, b) and wn.flags.c_contiguous and we.flags.c_contiguous
    wn, we = contrast_plan(3, 2, {"eta": b})
    assert wn.shape == (2, 3) and not wn.any() and np.array_equal(we, b)
    wn, we = contrast_plan(3, 2, {"nu": a})
    assert np.array_equal(wn, a) and we.shape == (2, 3, 2) and not we.any()
    assert contrast_plan(3, 0, {"nu": a})[1] is None


@pytest.mark.parametrize("K,D,contrasts,msg", [
    (3, 0, "effects", "requires covariates"),
    (3, 2, "differences", "must be 'pairwise', 'effects'"),
    (3, 2, [], "no contrasts"),
    (1, 0, "pairwise", "no contrasts"),
    (3, 2, [[(1, 0, [0.0, 1.0], 4)]], r"a term is \(weight, k\) or \(weight, k, x\), got 4 entries"),
    (3, 2, [[(1,)]], "got 1 entries"),
    (3, 2, [[(1, 0)], [(1, 3)]], "contrast 1: cluster 3 outside 0 .. 2"),
    (3, 2, [[(1, -1)]], "cluster -1 outside"),
    (3, 0, [[(1, 0, [1.0])]], "a term has an x but the sampler has no covariates"),
    (3, 2, [[(1, 0, [1.0, 2.0, 3.0])]], "x must have 2 entries, one per covariate, got 3"),
    (3, 2, {"nu": np.zeros((2, 4))}, r"contrasts\['nu'\] must have shape \(R, 3\)"),
    (3, 2, {"nu": np.zeros((2, 3)), "eta": np.zeros((3, 3, 2))}, r"contrasts\['eta'\] must have shape \(2, 3, 2\)"),
    (3, 0, {"nu": np.zeros((2, 3)), "eta": np.zeros((2, 3, 0))}, "the sampler has no covariates"),
    (3, 2, {"mu": np.zeros((2, 3))}, "the keys 'nu' and 'eta'"),
    (3, 2, {}, "the keys 'nu' and 'eta'"),
])
def test_plan_refusals(K, D, contrasts, msg):
    with pytest.raises(ValueError, match=msg):
        contrast_plan(K, D, contrasts)


# ---- the values against what is already restated ------------------------------------------------------------------------------
def test_pairwise_is_the_difference_of_mean_value_rows():
    rng = np.random.default_rng(3)
    d = _draw(rng)
    wn, _ = contrast_plan(3, 0, "pairwise")
    v = CR.values(d["E"], d["nu"], d["A"], wn)
    m, _ = R.mean_values(d["E"], d["nu"], d["A"])                      # (K, G)
    for r, (k, l) in enumerate([(0, 1), (0, 2), (1, 2)]):
        assert np.max(np.abs(v[r] - (m[k] - m[l]))) <= 2.0 ** -58 * float(np.max(np.abs(m)))
    # at a covariate setting: f_k(x) - f_l(x)
    x = np.array([0.3, -1.2])
    wn, we = contrast_plan(3, 2, [[(1, 0, x), (-1, 2, x)]])
    v = CR.values(d["E"], d["nu"], d["A"], wn, d["eta"], we)
    m, ma = R.mean_values(d["E"], d["nu"], d["A"], d["eta"], x)
    assert np.max(np.abs(v[0] - (m[0] - m[2]))) <= 2.0 ** -58 * float(np.max(ma))
    # abar of a single term is mean_values' own companion
    wn, we = contrast_plan(3, 2, [[(1, 1, x)]])
    va = CR.values(d["E"], d["nu"], d["A"], wn, d["eta"], we, absolute=True)
    assert np.max(np.abs(va[0] - ma[1])) <= 2.0 ** -58 * float(np.max(ma))


def test_effects_with_the_identity_are_E_eta():
    rng = np.random.default_rng(4)
    d = _draw(rng)
    wn, we = contrast_plan(3, 2, "effects")
    v = CR.values(d["E"], d["nu"], np.eye(3), wn, d["eta"], we)
    for k in range(3):
        for dd in range(2):
            want = np.asarray(d["E"], dtype=CR.LD) @ np.asarray(d["eta"][:, dd, k], dtype=CR.LD)
            assert np.array_equal(v[k * 2 + dd], want)
    # a permutation matrix picks the permuted component exactly
    perm = np.array([2, 0, 1])
    v = CR.values(d["E"], d["nu"], CR.perm_matrix(perm), wn, d["eta"], we)
    want = np.asarray(d["E"], dtype=CR.LD) @ np.asarray(d["eta"][:, 1, perm[0]], dtype=CR.LD)
    assert np.array_equal(v[1], want)


# ---- p_sim is the level of the band --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 1.0, 2.0, 4.0])
def test_p_sim_below_alpha_exactly_where_the_band_excludes_zero(shift):
    """at the levels alpha = (i + 1 / 2) / N the (1 - alpha) quantile is an order statistic (the module docstring of the restatement),
    and continuous draws have no ties"""
    rng = np.random.default_rng(11)
    R_, G, N = 4, 7, 50
    V = rng.standard_normal((R_, G, N)) + shift * np.arange(R_)[:, None, None] / (R_ - 1.0)
    V[0, 3] = 0.0                                           # a grid point that does not vary: skipped
    seen = set()
    for i in range(0, N - 1):
        alpha = (i + 0.5) / N
        s = CR.summary(V, alpha)
        assert len(np.unique(s["dev"][0])) == N              # no ties
        excl = s["excludes_zero"].any(axis=-1)
        assert not s["excludes_zero"][0, 3]
        assert np.array_equal(s["p_sim"] < alpha, excl), (alpha, s["p_sim"], excl)
        seen.update(excl.tolist())
    if shift >= 2.0:      # a mean two sd from zero lies outside the narrow bands and inside the wide ones; row 0 is never excluded
        assert seen == {True, False}
    # a contrast that does not vary at all: nothing to standardise, p_sim 1, crit 0, never excluded
    Z = np.zeros((1, G, N))
    s = CR.summary(Z, 0.05)
    assert s["p_sim"][0] == 1.0 and s["crit"][0] == 0.0 and not s["excludes_zero"].any() and not s["prob_positive"].any()


def test_norm_and_prob_positive():
    rng = np.random.default_rng(12)
    V = rng.standard_normal((2, 5, 9))
    w = rng.uniform(0.0, 2.0, 5)
    assert np.allclose(CR.norm(V, w), np.sqrt((w[None, :, None] * V ** 2).sum(axis=1)))
    assert np.allclose(CR.norm(V), np.sqrt((V ** 2).mean(axis=1)))
    assert np.array_equal(CR.prob_positive(V), (V > 0).mean(axis=-1))
    assert CR.prob_positive(np.zeros((1, 2, 3))).tolist() == [[0.0, 0.0]]      # strictly
