"""CPU checks of the numpy restatement of the marginal PSIS-LOO over curves (tests/loo_marginal_ref.py): the floor of
the refinement's stage 0 -- the only arithmetic 7m does not have: the Dirichlet correction with a proposal that is not the prior --
in float64 against np.longdouble, which the device test's proposal tolerance is built on; the estimator (first pass from the prior,
refinement from its last proposal) against a quadrature where K = 2; and the selection rule with its list order."""
import math

import numpy as np

import loo_marginal_ref as L
import predict_ref as R


def test_refinement_stage0_float64_against_long_double():
    assert np.finfo(np.longdouble).eps < 1e-18
    for x in (0.3, 1.0, 7.5, 77.7, 480.0):
        # the long-double lgamma itself, against the C library's, which is good to a few ulp of a double (8 here)
        assert abs(float(L.lgamma_ld(x)) - math.lgamma(x)) <= 8 * 2.3e-16 * max(1.0, abs(math.lgamma(x)))
    worst = L.stage0_floor()
    print(f"refinement stage 0: worst |float64 - longdouble| / max(1, |.|) over 600 inputs = {worst:.3e}")
    assert worst < 1e-9
    # where the start is the prior the correction is zero: stage 0 of the refinement is stage 0 of the first pass
    rng = np.random.default_rng(1)
    prior = np.array([0.4, 1.5, 3.0])
    z = np.maximum(rng.dirichlet(prior, size=50), R.TINY)
    ell = rng.standard_normal(50)
    assert np.max(np.abs(R.log_weights(ell, z, prior, prior) - R.log_weights(ell, z, prior, None))) == 0.0


def test_first_pass_then_refinement_against_quadrature_k2():
    """the curve of loo_marginal_ref.k2_case: 20 points, sigma^2 = 0.05, memberships (0.7, 0.3), prior (2, 3)"""
    ell, prior = L.k2_case()
    exact = L.k2_exact(ell, prior, 400)
    assert abs(exact - L.k2_exact(ell, prior, 200)) < 1e-10      # the quadrature has converged
    J, J2, R2 = 256, 1024, 2
    for stages in (1, 3):
        devs, err_first, err_ref = [], [], []
        for seed in range(8):
            first, ref = L.staged_then_refined(ell, prior, J, stages, J2, R2, np.random.default_rng(100 + seed))
            assert np.array_equal(ref["proposals"][0], first["proposals"][-1])
            se = math.sqrt(max(1.0 / ref["ess"] - 1.0 / J2, 0.0))      # delta method, as tests/test_predict_ref.py
            devs.append(abs(ref["lpd"] - exact) / se)
            err_first.append(abs(first["lpd"] - exact))
            err_ref.append(abs(ref["lpd"] - exact))
            print(f"R = {stages}, seed {seed}: first lpd = {first['lpd']:.6f} (ess {first['ess']:.1f}), refined lpd = {ref['lpd']:.6f} "
                  f"(ess {ref['ess']:.1f}), exact {exact:.6f}, |dev| / se = {devs[-1]:.2f}")
        print(f"R = {stages}: mean |error| first {np.mean(err_first):.4f}, refined {np.mean(err_ref):.4f}")
        # the multiples of tests/test_predict_ref.py's K = 2 check
        assert max(devs) < 5.0 and np.median(devs) < 2.0
        assert np.mean(err_ref) <= np.mean(err_first)


def test_selection_rule_and_list_order():
    nan, inf = np.nan, np.inf
    # 2 curves x 2 chains x 3 slots
    ess = np.array([[[12.0, 9.999, 10.0], [nan, 1.0, 200.0]],
                    [[50.0, 50.0, 50.0], [3.0, nan, 0.0]]])
    lpd = np.array([[[-1.0, -2.0, -3.0], [-4.0, -5.0, -inf]],
                    [[nan, -7.0, inf], [-9.0, -1.0, -2.0]]])
    sel = L.selected(lpd, ess, 10.0)
    # below the floor: (0,0,1), (0,1,1), (1,1,0), (1,1,2); not finite lpd: (0,1,2), (1,0,0), (1,0,2); a NaN ess alone: not selected
    want = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 2], [1, 0, 0], [1, 0, 2], [1, 1, 0], [1, 1, 2]], dtype=np.int32)
    idx, cnt = L.select_list(lpd, ess, 10.0)
    assert idx.dtype == np.int32 and np.array_equal(idx, want) and np.array_equal(cnt, [3, 4])
    assert sel.sum() == 7 and not sel[0, 1, 0] and not sel[1, 1, 1] and not sel[0, 0, 2]      # 10.0 is not below 10.0
    # increasing cs = chain * S + slot within a curve, curves in order
    key = (idx[:, 0] * 2 + idx[:, 1]) * 3 + idx[:, 2]
    assert np.all(np.diff(key) > 0)
    # floor 0 selects the pairs without a finite lpd alone
    idx0, cnt0 = L.select_list(lpd, ess, 0.0)
    assert np.array_equal(idx0, [[0, 1, 2], [1, 0, 0], [1, 0, 2]]) and np.array_equal(cnt0, [1, 2])
    # the pipeline: rows of equal values have p_loo = 0 and elpd_loo = the value
    out = L.loo_from_traces(np.full((3, 2, 12), -1.25))
    assert np.allclose(out["pointwise_elpd_loo"], -1.25) and np.allclose(out["lppd"], -1.25)
