"""Properties of the numpy restatement of PSIS-LOO / WAIC (tests/psis_ref.py), the yardstick of the device pass
k_post_psis.  CPU only."""
import math

import numpy as np
import pytest

import psis_ref as R


def _gpd(k, S, seed):
    u = np.random.default_rng(seed).random(S)
    return ((1 - u) ** (-k) - 1) / k


def test_constant_row_uniform_weights():
    for S in (1, 7, 100, 4000):
        r = R.psis_row(np.full(S, -3.25))
        assert r["lppd"] == pytest.approx(-3.25, abs=1e-13)
        assert r["elpd_loo"] == pytest.approx(-3.25, abs=1e-13)
        assert r["elpd_waic"] == pytest.approx(-3.25, abs=1e-13)
        assert abs(r["p_loo"]) < 1e-12 and r["p_waic"] == 0.0
        assert np.all(r["lw"] == r["lw"][0])
        assert r["pareto_k"] == math.inf          # a constant tail is flat


def test_short_rows_are_not_smoothed():
    rng = np.random.default_rng(3)
    for S in (1, 2, 5, 20):
        ll = rng.standard_normal(S)
        r = R.psis_row(ll)
        assert r["pareto_k"] == math.inf
        lw = np.minimum(-ll - np.max(-ll), 0.0)
        np.testing.assert_array_equal(r["lw"], lw)
    # S = 21 is the first length with a tail of five draws
    assert math.isfinite(R.psis_row(rng.standard_normal(21))["pareto_k"])


def test_flat_tail_gives_infinite_k():
    ll = np.concatenate([np.linspace(-5.0, -1.0, 80), np.full(20, -6.0)])      # the 20 largest log-ratios are equal
    r = R.psis_row(ll)
    assert r["pareto_k"] == math.inf
    np.testing.assert_array_equal(r["lw"], np.minimum(-ll - np.max(-ll), 0.0))


def test_ties_follow_draw_order():
    """the stable sort: of equal log-ratios, the later draws enter the tail first; the cutoff is a tied draw"""
    S = 100                                     # L = 20
    ll = -np.linspace(0.0, 3.0, S)
    ll[[10, 40, 70]] = ll[81]                   # four equal entries at ranks 19..22 from the top: two in the tail
    r = R.psis_row(ll)
    lw0 = -ll - np.max(-ll)
    order = np.argsort(lw0, kind="stable")
    tail = set(order[S - 20:].tolist())
    tied = [10, 40, 70, 81]
    inside = [t for t in tied if t in tail]
    assert inside == [70, 81]
    assert order[S - 21] == 40                  # the cutoff
    changed = set(np.nonzero(r["lw"] != np.minimum(lw0, 0.0))[0].tolist())
    assert changed <= tail


@pytest.mark.parametrize("k", [0.2, 0.5, 0.8])
def test_gpd_shape_recovered(k):
    ll = -np.log(_gpd(k, 4000, 0))              # log-ratios -ll drawn from a GPD with shape k
    r = R.psis_row(ll)
    assert abs(r["pareto_k"] - k) < 0.1, r["pareto_k"]


def test_gpd_fit_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for k in (0.2, 0.5, 0.8):
        e = np.sort(_gpd(k, 400, 1))
        khat, sigma = R.gpdfit(e)
        c, loc, scale = stats.genpareto.fit(e, floc=0.0)
        assert np.sign(khat) == np.sign(c)
        assert abs(khat - c) < 0.35 and 0.5 < sigma / scale < 2.0


def test_totals():
    ll = np.random.default_rng(5).standard_normal((7, 50)) - 2.0
    out = R.psis_loo(ll)
    pw = out["pointwise_elpd_loo"]
    assert out["elpd_loo"] == pytest.approx(np.sum(pw), rel=1e-14)
    assert out["se_elpd_loo"] == pytest.approx(math.sqrt(7 * np.var(pw, ddof=1)), rel=1e-12)
    assert out["looic"] == -2 * out["elpd_loo"] and out["waic"] == -2 * out["elpd_waic"]
    assert out["khat_threshold"] == pytest.approx(min(1 - 1 / math.log10(50), 0.7))
    assert out["n_khat_above"] == int(np.sum(out["pareto_k"] > out["khat_threshold"]))
    np.testing.assert_allclose(out["pointwise_p_loo"], out["lppd"] - pw)
    assert math.isnan(R.psis_loo(ll[:1])["se_elpd_loo"])
