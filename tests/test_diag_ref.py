"""CPU checks of the numpy restatement of the convergence diagnostics (tests/diag_ref.py) against hand-worked
values and known properties of R-hat and ESS; the restatement is the yardstick of the device kernel."""
import math

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

import diag_ref as R


def _rhat_by_hand(z):
    m, n = z.shape
    means = z.mean(axis=1)
    B = n * np.sum((means - means.mean()) ** 2) / (m - 1)
    W = np.mean([np.sum((r - r.mean()) ** 2) / (n - 1) for r in z])
    return math.sqrt((B / W + n - 1) / n)


def test_hand_worked_two_chains_five_draws():
    x = np.array([[1.0, 3.0, 100.0, 2.0, 5.0],
                  [3.0, 4.0, -50.0, 6.0, 0.0]])
    xs = R.split(x)
    np.testing.assert_array_equal(xs, [[1, 3], [2, 5], [3, 4], [6, 0]])     # the middle draws 100 and -50 are dropped
    ranks = rankdata(xs).reshape(xs.shape)
    np.testing.assert_array_equal(ranks, [[2, 4.5], [3, 7], [4.5, 6], [8, 1]])     # the two 3s share 4.5
    z = R.z_scale(xs)
    np.testing.assert_array_equal(z, ndtri((ranks - 0.375) / 8.25))
    v = np.sort(xs.reshape(-1))
    assert R.quantile7(v, 0.5) == 3.0
    assert R.quantile7(v, 0.05) == 7 * 0.05 and R.quantile7(v, 0.95) == 5.0 + (7 * 0.95 - 6)
    folded_ranks = rankdata(np.abs(xs - 3.0)).reshape(xs.shape)
    np.testing.assert_array_equal(folded_ranks, [[5.5, 1.5], [3.5, 5.5], [1.5, 3.5], [7.5, 7.5]])
    out = R.diag_row(x)
    expect = max(_rhat_by_hand(z), _rhat_by_hand(ndtri((folded_ranks - 0.375) / 8.25)))
    assert out["rhat"] == expect
    for k in ("ess_bulk", "ess_tail", "ess_mean", "mcse_mean"):
        assert math.isnan(out[k]), k                                         # n = 2 < 3
    assert out["mean"] == 7.4
    assert out["sd"] == math.sqrt(np.sum((x - 7.4) ** 2) / 9)
    x2 = x.copy()
    x2[:, 2] = [7.0, 8.0]                                                    # other middle draws: the same R-hat
    assert R.diag_row(x2)["rhat"] == out["rhat"]


def test_iid_normal():
    x = np.random.default_rng(1).standard_normal((1000, 4))
    d = R.diagnostics(x)
    assert abs(d["rhat"] - 1.0) < 0.01
    assert abs(d["ess_bulk"] - 4000) < 400
    assert abs(d["ess_tail"] - 4000) < 800
    assert d["mcse_mean"] == d["sd"] / math.sqrt(d["ess_mean"])


def _ar1(rho, S, C, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((S, C))
    x = np.empty((S, C))
    x[0] = e[0] / math.sqrt(1 - rho * rho)
    for t in range(1, S):
        x[t] = rho * x[t - 1] + e[t]
    return x


def test_ar1_ess_of_the_mean():
    x = _ar1(0.9, 4000, 4, 2)
    N = x.size
    assert abs(R.diagnostics(x)["ess_mean"] / (N * 0.1 / 1.9) - 1) < 0.15


def test_shifted_chain_raises_rhat():
    x = np.random.default_rng(3).standard_normal((1000, 4))
    x[:, 2] += 1.0
    assert R.diagnostics(x)["rhat"] > 1.1


def test_scale_difference_is_caught_by_the_folded_rhat():
    x = np.random.default_rng(4).standard_normal((1000, 4))
    x[:, 0] *= 3.0
    x[:, 1] *= 3.0
    xs = R.split(x.T)
    assert abs(R.rhat_seq(R.z_scale(xs)) - 1.0) < 0.02                        # the bulk R-hat sees equal locations
    assert R.diagnostics(x)["rhat"] > 1.05


def test_antithetic_chain_is_capped():
    x = _ar1(-0.9, 1000, 4, 5)
    N = 2 * 4 * 500
    d = R.diagnostics(x)
    assert d["ess_mean"] == N * math.log10(N)
    assert d["ess_bulk"] == N * math.log10(N)


def test_constant_and_nan_rows():
    x = np.random.default_rng(6).standard_normal((100, 3, 3))
    x[:, :, 1] = 2.5
    x[7, 1, 2] = np.nan
    d = R.diagnostics(x)
    for k in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean"):
        assert np.isfinite(d[k][0]) and math.isnan(d[k][1]) and math.isnan(d[k][2]), k
    assert d["mean"][1] == 2.5 and d["sd"][1] == 0.0
    assert math.isnan(d["mean"][2])


def test_bulk_and_tail_ess_depend_on_ranks_only():
    x = _ar1(0.5, 600, 4, 7)
    a, b = R.diagnostics(x), R.diagnostics(np.exp(x))
    assert a["ess_bulk"] == b["ess_bulk"]
    assert a["ess_tail"] == b["ess_tail"]
    assert a["ess_mean"] != b["ess_mean"]
