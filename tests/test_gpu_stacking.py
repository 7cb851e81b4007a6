"""Stacking weights on the device (k_stack_prepare, k_stack_em, k_stack_final, bfmmm_post_stacking) against the
long-double restatement (tests/stacking_ref.py) at the shapes where the kernels can go wrong: units below, at and above a wave, a
workgroup and one grid-stride pass; every instance of the accumulator count; rows near -1e5 and +700, -inf entries and a given
start in every case.  The bound on the weights at a fixed iteration count is stacking_ref.weights_bound: 8 x what two float64
orders of the row sum differ from long double by, at least 64 eps, computed from the restatement and never from the device."""
import numpy as np
import pytest

import stacking_ref as R

pytestmark = pytest.mark.gpu

LD = R.LD


def _geometry():
    from bayesfmmm_amd import api
    threads, groups = api.stacking_geometry()
    return threads * groups


def _cases():
    out = [(n, Q) for n in R.SMALL_N for Q in R.QS]
    return out + [("pass+1", Q) for Q in R.BIG_QS]


@pytest.mark.parametrize("n,Q", _cases())
def test_weights_at_a_fixed_iteration_count(n, Q):
    from bayesfmmm_amd import api
    n = _geometry() + 1 if n == "pass+1" else n
    L, init = R.simulate(n, Q, seed=1000 * Q + n % 997)
    ref = R.weights_bound(L, init)
    for t in R.ITERS:
        w_ld, bound = ref[t]
        res = api.stacking(L, init=init, max_iter=t, check_every=16, tol=0.0)
        assert res["n_iter"] == t and res["weights"].shape == (Q,) and res["pointwise"].shape == (n,)
        err = float(np.max(np.abs(res["weights"].astype(LD) - w_ld)))
        print(f"n={n} Q={Q} iterations={t}: worst |w_device - w_ld| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert err <= bound, (n, Q, t, err, bound)
        assert abs(float(np.sum(res["weights"])) - 1.0) <= Q * (R.EPS + bound)
    # At the last count also what goes with the weights, in long double at the device's weights.  d_i is a sum of Q positive products
    # of a weight and an exp good to 2 ulp, so log d_i moves by at most (Q + 8) eps and l_i = m_i + log d_i by that on its own scale;
    # a sum of such terms by the additions on its longest path (the rows of a thread, the butterfly, the waves, the workgroups).
    at = R.evaluate(L, res["weights"])
    scale = np.maximum(1.0, np.abs(at["pointwise"].astype(float)))
    assert np.all(np.abs(res["pointwise"] - at["pointwise"].astype(float)) <= (Q + 8) * R.EPS * scale)
    threads, groups = api.stacking_geometry()
    depth = -(-n // (threads * groups)) + 6 + threads // 64 + min(groups, -(-n // threads))
    assert abs(res["objective"] - float(at["objective"])) <= (depth + Q + 8) * R.EPS * float(np.sum(scale))
    assert abs(res["gap"] - float(at["gap"])) <= (depth + Q + 10) * R.EPS * (1 + float(at["gap"]))
    assert res["elpd"] == api._total_se(res["pointwise"])[0] and res["converged"] == (res["gap"] <= 0.0)


def _gap_at_device_weights(L, res, tol):
    """gap_ld at the device's weights is within tol, up to the rounding of a gap: what the two float64 orders of the sum make of it at
    these weights, times 8, at least 64 eps"""
    at = R.evaluate(L, res["weights"])
    tw = [float(abs(R.evaluate(L, res["weights"], dtype=dt, row_sum=fn)["gap"].astype(LD) - at["gap"])) for dt, fn in R.SUMS.values()]
    rounding = max(8.0 * max(tw), 64 * R.EPS)
    print(f"n={L.shape[0]} Q={L.shape[1]}: {res['n_iter']} iterations, device gap {res['gap']:.3e}, long-double gap at its weights "
          f"{float(at['gap']):.3e}, rounding allowed {rounding:.1e}")
    assert float(at["gap"]) <= tol + rounding
    return at


@pytest.mark.parametrize("n,Q,seed", [(257, 3, 4), (64, 17, 5), (255, 1, 7), (1000, 8, 8)])
def test_convergence_is_certified_in_long_double(n, Q, seed):
    """the default tol: f and gap evaluated in long double at the device's weights"""
    from bayesfmmm_amd import api
    L, init = R.simulate(n, Q, seed)
    res = api.stacking(L, init=init)
    assert res["converged"] and res["n_iter"] % 16 == 0 and 0 < res["n_iter"] <= 10000 and res["gap"] <= 1e-8
    at = _gap_at_device_weights(L, res, 1e-8)
    ref = R.em(L, init)
    assert ref["converged"]
    short = ref["objective"] - at["objective"]
    print(f"  f_ld(w_ref) - f_ld(w_device) = {float(short):.3e}, n gap_ld(w_ref) = {float(n * ref['gap']):.3e}")
    assert short <= n * ref["gap"]
    assert short <= n * at["gap"] and -short <= n * ref["gap"]          # the certificate, both ways round


def test_convergence_above_one_grid_stride_pass():
    """the same certificate where every workgroup runs and some threads own two rows (the long-double loop would take too long here:
    the weights are judged by their own long-double gap alone)"""
    from bayesfmmm_amd import api
    L, init = R.simulate(_geometry() + 1, 8, 6)
    res = api.stacking(L, init=init)
    assert res["converged"] and res["n_iter"] % 16 == 0 and res["gap"] <= 1e-8
    _gap_at_device_weights(L, res, 1e-8)


def test_check_every_and_repetition_give_identical_bits():
    from bayesfmmm_amd import api
    L, init = R.simulate(_geometry() + 1, 8, 21)
    runs = [api.stacking(L, init=init, max_iter=112, check_every=ce, tol=0.0) for ce in (1, 16, 7, 16)]
    small, sinit = R.simulate(65, 17, 22)
    runs2 = [api.stacking(small, init=sinit, max_iter=112, check_every=ce, tol=0.0) for ce in (1, 16, 7, 16)]
    for rr in (runs, runs2):
        for r in rr[1:]:
            assert r["n_iter"] == 112
            for k in ("weights", "pointwise"):
                assert r[k].tobytes() == rr[0][k].tobytes(), k
            for k in ("objective", "gap", "elpd", "se_elpd"):
                assert r[k] == rr[0][k], k
    # a loop that stops early returns the iterate a fixed count gives
    early = api.stacking(small, init=sinit, check_every=7, tol=1e-4)
    assert early["converged"] and early["n_iter"] % 7 == 0
    fixed = api.stacking(small, init=sinit, max_iter=early["n_iter"], tol=0.0)
    assert early["weights"].tobytes() == fixed["weights"].tobytes() and early["gap"] == fixed["gap"]
    before = api.stacking(small, init=sinit, max_iter=early["n_iter"] - 7, tol=0.0)
    assert early["n_iter"] == 7 or before["gap"] > 1e-4


def test_refusals():
    from bayesfmmm_amd import _lib, api
    L, _ = R.simulate(300, 4, 31)
    with pytest.raises(_lib.BfmmmError, match="at most 64 candidates"):
        api.stacking(np.zeros((5, 65)))
    for val, name in ((np.nan, "NaN"), (np.inf, r"\+inf")):
        B = L.copy()
        B[259, 2] = val
        B[290, 0] = val
        B[290, 3] = val
        with pytest.raises(_lib.BfmmmError, match=rf"3 offending entries or units, the first at unit 259, candidate 2 \({name}\)"):
            api.stacking(B)
    B = L.copy()
    B[70] = -np.inf
    with pytest.raises(_lib.BfmmmError, match=r"1 offending entries or units, the first at unit 70, candidate 0 \(-inf for every"):
        api.stacking(B)
    with pytest.raises(_lib.BfmmmError, match="'init' must lie on the simplex"):
        api.stacking(L, init=[0.5, 0.5, 0.5, 0.5])
    with pytest.raises(_lib.BfmmmError, match=r"'init'\[3\]"):
        api.stacking(L, init=[0.5, 0.25, 0.25, 0.0])
    with pytest.raises(ValueError, match="'init' must have 4 entries"):
        api.stacking(L, init=[0.5, 0.5])
    with pytest.raises(ValueError, match="n x Q"):
        api.stacking(np.zeros(5))


def test_stack_models_table():
    from bayesfmmm_amd import api
    rng = np.random.default_rng(41)
    base = -1.0 + 0.5 * rng.standard_normal(400)
    vecs = [base + 0.3 * rng.standard_normal(400) - 0.2, {"pointwise_elpd_loo": base + 0.1 * rng.standard_normal(400)},
            base + 0.6 * rng.standard_normal(400) - 0.5]
    res = api.stack_models(vecs, names=["a", "b", "c"])
    L = np.stack([vecs[0], vecs[1]["pointwise_elpd_loo"], vecs[2]], axis=1)
    ref = R.compare_table(L)
    assert res["best"] == ref["best"] == 1 and res["names"] == ["a", "b", "c"]
    for k in ("elpd", "se", "elpd_diff", "se_diff", "pseudo_bma"):
        np.testing.assert_allclose(res[k], ref[k].astype(float), rtol=1e-12, atol=0, err_msg=k)
    assert res["elpd_diff"][1] == 0 and res["se_diff"][1] == 0 and np.all(res["elpd_diff"] <= 0)
    assert abs(res["pseudo_bma"].sum() - 1) < 1e-15 and np.argmax(res["pseudo_bma"]) == 1
    direct = api.stacking(L)
    assert res["weights"].tobytes() == direct["weights"].tobytes() and res["converged"]
    assert res["elpd"].shape == (3,) and api.stack_models(vecs)["names"] == ["model0", "model1", "model2"]
    # the stacked mixture predicts at least as well as the best single candidate, up to the certificate and the rounding of two sums
    # of 400 terms (here the optimum is that candidate alone, and the certificate is tight to the last digits)
    assert res["objective"] >= res["elpd"][1] - 400 * res["gap"] - 64 * R.EPS * float(np.sum(np.abs(L[:, 1])))
