"""The restatement of the pooled per-curve covariance surfaces (tests/curve_cov_ref.py) against np.longdouble on
2000 random cases of one (curve, g, h) each: the float64 restatement and its sequential-order variant (the kernel's order) stay
within half of the derived bounds, the sum over cluster-level surfaces within the bounds, and a one-pass variance breaks the
sd bound on nearly constant rows."""
import itertools

import numpy as np

import curve_cov_ref as R

P = 6
NS = (2, 3, 23, 500)
MS = (1, 4, 5, 16)


def _cases(rng, c, N, K, M, D, kind):
    """c cases.  kind 0: Dirichlet rows of Z; 1: rows with exact zeros; 2: nearly cancelling phi"""
    e1, e2 = rng.standard_normal((c, P)), rng.standard_normal((c, P))
    Z = rng.dirichlet(np.full(K, 0.5), size=(c, N))
    Phi = rng.standard_normal((c, N, K, P, M))
    if kind == 1:
        Z[:, :, rng.integers(K)] = 0.0
        Z[:, ::2] = np.eye(K)[rng.integers(K, size=(c, (N + 1) // 2))]
        Z = Z / Z.sum(axis=-1, keepdims=True)
    if kind == 2:
        Z[:, :, :2] = Z[:, :, :2].mean(axis=-1, keepdims=True)
        Phi[:, :, 1] = -Phi[:, :, 0] * (1.0 + 1e-8 * rng.standard_normal((c, N, 1, 1)))
    xi = 0.3 * rng.standard_normal((c, N, K, P, M, D)) if D else None
    x = rng.standard_normal((c, D)) if D else None
    return e1, e2, Z, Phi, xi, x


def test_restatement_and_sequential_variant_against_longdouble():
    rng = np.random.default_rng(20260)
    configs = list(itertools.product(range(2, 9), MS, (0, 2), NS))      # 224
    per = [8] * len(configs)
    for j in range(2000 - 8 * len(configs)):
        per[j] += 1
    assert sum(per) == 2000
    worst = {"mean": 0.0, "sd": 0.0, "seq_mean": 0.0, "seq_sd": 0.0, "cluster_mean": 0.0, "cluster_sd": 0.0, "A/|d|": 0.0}
    total = 0
    for j, ((K, M, D, N), c) in enumerate(zip(configs, per)):
        args = _cases(rng, c, N, K, M, D, j % 3)
        ld = R.pair_draws(*args, dtype=np.longdouble)
        A = R.pair_draws(*args, absolute=True)
        assert np.all(A >= np.abs(np.asarray(ld, dtype=np.float64)) * (1 - 1e-12))
        mean_ld, sd_ld = R.moments(ld)
        cd = R.c_d(P, K, M, D)
        bm = R.mean_bound(A.mean(axis=-1), N, cd)
        bs = R.sd_bound(np.asarray(sd_ld, dtype=np.float64), A.max(axis=-1), N, cd)
        assert np.all(bm > 0) and np.all(bs > 0)
        worst["A/|d|"] = max(worst["A/|d|"], float(np.max(A.mean(axis=-1) / np.abs(np.asarray(mean_ld, dtype=np.float64)))))
        for name, d, mom, frac in (("", R.pair_draws(*args), R.moments, 0.5), ("seq_", R.pair_draws_sequential(*args), R.moments_sequential, 0.5),
                                   ("cluster_", R.pair_draws_cluster(*args), R.moments, 1.0)):
            mean, sd = mom(d)
            rm = float(np.max(np.abs(mean - mean_ld) / bm))
            rs = float(np.max(np.abs(sd - sd_ld) / bs))
            worst[name + "mean"], worst[name + "sd"] = max(worst[name + "mean"], rm), max(worst[name + "sd"], rs)
            assert rm <= frac and rs <= frac, (name, K, M, D, N, rm, rs)
        total += c
    assert total == 2000
    print("worst |float64 - longdouble| / bound over 2000 cases: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["A/|d|"] > 1e3      # the nearly cancelling cases are among them


def test_one_pass_variance_breaks_the_sd_bound_on_nearly_constant_rows():
    rng = np.random.default_rng(7)
    c, N, K, M = 50, 500, 2, 4
    e1, e2, Z, Phi, xi, x = _cases(rng, c, N, K, M, 0, 0)
    e2 = e1
    Z[:] = np.array([1.0, 0.0])
    Phi[:] = Phi[:, :1] * (1.0 + 1e-9 * rng.standard_normal((c, N, 1, 1, 1)))      # d moves in its ninth digit
    args = (e1, e2, Z, Phi, None, None)
    ld = R.pair_draws(*args, dtype=np.longdouble)
    mean_ld, sd_ld = R.moments(ld)
    A = R.pair_draws(*args, absolute=True)
    cd = R.c_d(P, K, M, 0)
    bs = R.sd_bound(np.asarray(sd_ld, dtype=np.float64), A.max(axis=-1), N, cd)
    assert np.all(np.asarray(sd_ld / mean_ld, dtype=np.float64) < 1e-7)
    d = R.pair_draws(*args)
    two = np.abs(R.moments(d)[1] - sd_ld) / bs
    seq = np.abs(R.moments_sequential(R.pair_draws_sequential(*args))[1] - sd_ld) / bs
    one = np.abs(np.nan_to_num(R.sd_one_pass(d), nan=0.0) - np.asarray(sd_ld, dtype=np.float64)) / bs
    print(f"nearly constant rows: two-pass {two.max():.3e}, sequential {seq.max():.3e}, one-pass {np.median(one):.3e} (median) of the bound")
    assert two.max() <= 0.5 and seq.max() <= 0.5
    assert np.median(one) > 10.0 and np.mean(one > 1.0) > 0.9
