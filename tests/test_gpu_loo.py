"""PSIS-LOO and WAIC over curves on the device (include/bfmmm_post.h): the pointwise log-likelihood matrix of
the CPO pass (bfmmm_post_curve_loglik) against the oracle's dense marginal density, the PSIS / WAIC kernel (k_post_psis)
against the numpy restatement tests/psis_ref.py, and the file-based entry points FLOO / MVLOO."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O
import psis_ref as R
from test_gpu_post import _mv_trace_chain, _oracle_chain, _run_and_save

pytestmark = pytest.mark.gpu

_PW = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pointwise_elpd_waic", "pointwise_p_waic")
_TOT = ("elpd_loo", "p_loo", "looic", "elpd_waic", "p_waic", "waic", "se_elpd_loo", "se_p_loo", "se_looic", "se_elpd_waic",
        "se_p_waic", "se_waic")


def _assert_loo_equal(got, ref, rtol=1e-9, katol=1e-8):
    """elpd / p / lppd to rtol (with an absolute floor of rtol x the row's scale for the differences p_loo, p_waic); finite
    Pareto k to katol, infinite k exactly"""
    scale = max(1.0, float(np.max(np.abs(ref["lppd"]))))
    for k in _PW:
        np.testing.assert_allclose(got[k], ref[k], rtol=rtol, atol=rtol * scale, err_msg=k)
    kg, kr = np.asarray(got["pareto_k"]), np.asarray(ref["pareto_k"])
    np.testing.assert_array_equal(np.isinf(kg), np.isinf(kr))
    fin = np.isfinite(kr)
    np.testing.assert_allclose(kg[fin], kr[fin], rtol=0, atol=katol)
    n = len(ref["lppd"])
    for k in _TOT:
        if n == 1 and k.startswith("se_"):
            assert math.isnan(got[k]) and math.isnan(ref[k])
        else:
            np.testing.assert_allclose(got[k], ref[k], rtol=rtol, atol=rtol * scale * n, err_msg=k)
    assert got["khat_threshold"] == ref["khat_threshold"]
    assert got["n_khat_above"] == ref["n_khat_above"]


def _rows(S, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(S) * 0.7 - 3.0,                                   # light tail
            -np.log(((1 - rng.random(S)) ** -0.7 - 1) / 0.7) - 40.0,               # heavy-tailed ratios (GPD, shape 0.7)
            np.round(rng.standard_normal(S) * 2.0) - 5.0,                         # many ties
            np.full(S, -2.5)]                                                     # constant
    return np.ascontiguousarray(np.array(rows))


@pytest.mark.parametrize("S", [1, 5, 20, 21, 100, 4000, 100000])
def test_psis_matches_restatement(S):
    from bayesfmmm_amd import api
    ll = _rows(S, S)
    got = api.psis_loo(ll)
    _assert_loo_equal(got, R.psis_loo(ll))
    again = api.psis_loo(ll)
    for k in ("pareto_k",) + _PW:
        assert np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes(), k


def test_psis_longest_rows():
    """S = 2^22 (the build's bound): a tail of 6144 draws, the largest on-chip table"""
    from bayesfmmm_amd import api
    rng = np.random.default_rng(9)
    S = 1 << 22
    ll = np.ascontiguousarray(np.array([-np.log(((1 - rng.random(S)) ** -0.5 - 1) / 0.5), rng.standard_normal(S)]))
    _assert_loo_equal(api.psis_loo(ll), R.psis_loo(ll))


def _one_draw(model, ch, t):
    c1 = O.Chain(model, 1)
    for f in ("nu", "Z", "chi", "sigma", "Phi") + (("eta", "xi") if model.D > 0 else ()):
        getattr(c1, f)[..., 0] = getattr(ch, f)[..., t]
    return c1


def _check_matrix(mat, model, ch, first, draws):
    """row i of the device matrix against the oracle: a one-draw chain's log CPO is that draw's own marginal log-density"""
    for t in draws:
        ref = O.post_cpo(model, _one_draw(model, ch, t), 0.0)
        np.testing.assert_allclose(mat[:, t - first], ref, rtol=1e-9, atol=1e-9, err_msg=f"draw {t}")


@pytest.mark.parametrize("D,cov_adj", [(0, False), (1, False), (2, True)])
def test_curve_loglik_and_floo_match_oracle(tmp_path, D, cov_adj):
    from bayesfmmm_amd import api
    sim, X, dirn = _run_and_save(tmp_path, D, cov_adj)
    model, ch, B = _oracle_chain(sim, X, dirn, 3, cov_adj)
    T, burn = 120, 0.1
    first = int(math.floor(burn * T))
    mat = api.post_curve_loglik(sim["y"], B, ch.nu, ch.Phi, ch.Z, ch.chi, ch.sigma, first_kept=first, X=X,
                                eta=ch.eta if D else None, xi=ch.xi if cov_adj else None)
    assert mat.shape == (sim["n"], T - first)
    _check_matrix(mat, model, ch, first, (first, first + 37, first + 71, T - 1))
    S = T - first
    log_cpo = math.log(S) - np.array([R._lse(-r) for r in mat])      # the harmonic mean over the same draws
    np.testing.assert_allclose(log_cpo, O.post_cpo(model, ch, burn), rtol=1e-8)
    args = (dirn, 3, 3, sim["boundary_knots"], sim["internal_knots"], sim["t"], sim["y"])
    kw = dict(X=X, cov_adj=cov_adj) if D else {}
    got = api.FLOO(*args, burnin_prop=burn, **kw)
    _assert_loo_equal(got, R.psis_loo(mat))
    assert got["pareto_k"].shape == (sim["n"],)
    # the CPO pass behind the matrix is unchanged
    cpo = api.ConditionalPredictiveOrdinates(*args, burnin_prop=burn, **kw)
    np.testing.assert_allclose(cpo, log_cpo, rtol=1e-12)


@pytest.mark.parametrize("with_x,cov_adj", [(False, False), (True, True)])
def test_mvloo_on_the_reference_trace(with_x, cov_adj):
    """the identity basis (multivariate model, full (P / 2) log 2 pi): every kept draw against the oracle"""
    from bayesfmmm_amd import api
    X = np.random.default_rng(4).standard_normal((20, 1)) if with_x else None
    dirn, Y, model, ch = _mv_trace_chain(X, cov_adj)
    n, P = Y.shape
    T, burn = ch.T, 0.1
    first = int(math.floor(burn * T))
    ref_mat = np.zeros((n, T - first))
    for t in range(first, T):
        ref_mat[:, t - first] = O.post_cpo(model, _one_draw(model, ch, t), 0.0)
    mat = api.post_curve_loglik([Y[i] for i in range(n)], [np.eye(P)] * n, ch.nu, ch.Phi, ch.Z, ch.chi, ch.sigma, first_kept=first,
                                X=X, eta=ch.eta if with_x else None, xi=ch.xi if cov_adj else None)
    np.testing.assert_allclose(mat, ref_mat, rtol=1e-9, atol=1e-9)
    kw = dict(X=X, cov_adj=cov_adj) if with_x else {}
    got = api.MVLOO(dirn, 1, Y, burnin_prop=burn, **kw)
    _assert_loo_equal(got, R.psis_loo(ref_mat), rtol=1e-8, katol=1e-6)


def test_loo_argument_checks():
    from bayesfmmm_amd import _lib, api
    t = [np.linspace(0, 1, 5)] * 3
    y = [np.zeros(5)] * 3
    a = (3, [0.0, 1.0], [0.5], t, y)
    with pytest.raises(_lib.BfmmmError, match="'n_files' must be greater than 0"):
        api.FLOO("nowhere/", 0, *a)
    with pytest.raises(_lib.BfmmmError, match="'burnin_prop' must be between 0 and 1"):
        api.FLOO("nowhere/", 1, *a, burnin_prop=1.0)
    with pytest.raises(_lib.BfmmmError, match="'n_files' must be greater than 0"):
        api.MVLOO("nowhere/", 0, np.zeros((3, 4)))
    with pytest.raises(_lib.BfmmmError, match="'burnin_prop' must be between 0 and 1"):
        api.MVLOO("nowhere/", 1, np.zeros((3, 4)), burnin_prop=-0.1)
    lib = api._lib_entry()
    res = C.c_void_p()
    assert lib.bfmmm_FLOO(None, C.byref(res)) != 0
    assert "null argument" in lib.bfmmm_entry_last_error().decode()
    assert lib.bfmmm_MVLOO(None, C.byref(res)) != 0
    assert "null argument" in lib.bfmmm_entry_last_error().decode()
    z = np.zeros(1)
    p = z.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.bfmmm_post_psis(None, 1, 1, 0, p, p, p, p, p, p) != 0
    assert "null argument" in lib.bfmmm_entry_last_error().decode()
    with pytest.raises(_lib.BfmmmError, match=r"at most 4194304 \(2\^22\) kept draws"):
        api.psis_loo(np.zeros((1, (1 << 22) + 1)))
