"""Expectations under the Pareto-smoothed weights on the device (k_post_psis<NAUX>, bfmmm_post_psis_expect): the six
arrays of api.psis_expect against api.psis_loo bit for bit, and "expect" against the numpy restatement
(tests/loo_pointwise_ref.expect over psis_ref.psis_row) to rtol 1e-8 with an absolute floor of 1e-8 x max|h| of the row."""
import numpy as np
import pytest

import loo_pointwise_ref as R
import psis_ref

pytestmark = pytest.mark.gpu

LOO_ARRAYS = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic")


def _rows(S, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.standard_normal(S) * 0.7 - 3.0,                                   # light tail
            -np.log(((1 - rng.random(S)) ** -0.7 - 1) / 0.7) - 40.0,               # heavy-tailed ratios (GPD, shape 0.7)
            np.round(rng.standard_normal(S) * 2.0) - 5.0,                         # many ties
            np.full(S, -2.5)]                                                     # constant
    return np.ascontiguousarray(np.array(rows))


_REF = {}


def _case(S):
    """the matrix, its auxiliaries and the restatement's expectations, computed once per S"""
    if S not in _REF:
        ll = _rows(S, S)
        rng = np.random.default_rng(S + 1)
        n = ll.shape[0]
        h = np.stack([np.exp(ll), rng.standard_normal((n, S)) * 3.0 + 1.0, rng.random((n, S)), np.full((n, S), 7.25),
                      np.cos(ll) * 1e3])                                         # five: a second launch of one
        ref = np.array([[R.expect(ll[i], h[a, i]) for i in range(n)] for a in range(h.shape[0])])
        _REF[S] = (ll, h, ref)
    return _REF[S]


def _assert_expect(got, ref, h):
    assert got.shape == ref.shape
    for a in range(h.shape[0]):
        for i in range(h.shape[1]):
            tol = 1e-8 * abs(ref[a, i]) + 1e-8 * float(np.max(np.abs(h[a, i])))
            assert abs(got[a, i] - ref[a, i]) <= tol, (a, i, got[a, i], ref[a, i])


@pytest.mark.parametrize("S", [24, 100, 4000, 8193])
def test_expect_matches_restatement_and_psis_loo_bitwise(S):
    """S = 24: L < 5, no smoothing; S = 8193: one past a multiple of the workgroup"""
    from bayesfmmm_amd import api
    ll, h, ref = _case(S)
    plain = api.psis_loo(ll)
    for n_aux in (1, 3, 5):
        got = api.psis_expect(ll, h[:n_aux])
        for k in LOO_ARRAYS:
            assert np.asarray(got[k]).tobytes() == np.asarray(plain[k]).tobytes(), (k, n_aux)
        for k in plain:
            if k not in LOO_ARRAYS:
                assert got[k] == plain[k] or (np.isnan(got[k]) and np.isnan(plain[k])), k
        _assert_expect(got["expect"], ref[:n_aux], h[:n_aux])
    # the likelihood as auxiliary reproduces elpd_loo; a constant comes back
    got = api.psis_expect(ll, h)
    np.testing.assert_allclose(np.log(got["expect"][0]), plain["pointwise_elpd_loo"], rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(got["expect"][3], 7.25, rtol=1e-12)
    # a single matrix in place of a stack, and the same bits twice
    one = api.psis_expect(ll, h[1])
    assert one["expect"].shape == (ll.shape[0],)
    assert one["expect"].tobytes() == np.ascontiguousarray(got["expect"][1]).tobytes()
    again = api.psis_expect(ll, h)
    assert again["expect"].tobytes() == got["expect"].tobytes()
    # against the restatement's own six values too (test_gpu_loo's comparison, at this file's rtol)
    r = psis_ref.psis_loo(ll)
    np.testing.assert_allclose(got["pointwise_elpd_loo"], r["pointwise_elpd_loo"], rtol=1e-8, atol=1e-8 * max(1.0, np.abs(r["lppd"]).max()))


def test_argument_checks():
    from bayesfmmm_amd import _lib, api
    ll = np.zeros((3, 10))
    with pytest.raises(ValueError, match="'h'"):
        api.psis_expect(ll, np.zeros((3, 9)))
    with pytest.raises(ValueError, match="'h'"):
        api.psis_expect(ll, np.zeros((0, 3, 10)))
    with pytest.raises(ValueError, match="'ll'"):
        api.psis_expect(np.zeros(10), np.zeros(10))
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_post_psis_expect: at most 4194304 \(2\^22\) kept draws"):
        api.psis_expect(np.zeros((1, (1 << 22) + 1)), np.zeros((1, (1 << 22) + 1)))
