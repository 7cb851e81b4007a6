"""Convergence diagnostics on the device: the matrix route (bfmmm_post_diagnostics) and the chain-slot route
(bfmmm_chain_diagnostics) against the numpy restatement tests/diag_ref.py, determinism, and the argument checks."""

import numpy as np
import pytest

import diag_ref as R
from test_gpu_chain_batch import _states, make_sampler_batch
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

_SETS = {"ess_bulk": ("bulk",), "ess_mean": ("mean",), "ess_tail": ("q05", "q95")}


def _ar1(rho, S, C, rng):
    e = rng.standard_normal((S, C))
    x = np.empty((S, C))
    x[0] = e[0] / np.sqrt(1 - rho * rho)
    for t in range(1, S):
        x[t] = rho * x[t - 1] + e[t]
    return x


def _draws(S, C, seed):
    """(S, C, 7): normal, heavy ties, constant, NaN, +inf, -inf, AR(1) with rho = 0.995"""
    rng = np.random.default_rng(seed)
    d = np.empty((S, C, 7))
    d[:, :, 0] = rng.standard_normal((S, C)) * 3.0 + 10.0
    d[:, :, 1] = np.round(rng.standard_normal((S, C)) * 1.5)
    d[:, :, 2] = -4.25
    d[:, :, 3] = rng.standard_normal((S, C))
    d[S // 3, C - 1, 3] = np.nan
    d[:, :, 4] = rng.standard_normal((S, C))
    d[0, 0, 4] = np.inf
    d[:, :, 5] = rng.standard_normal((S, C))
    d[S - 1, 0, 5] = -np.inf
    d[:, :, 6] = _ar1(0.995, S, C, rng)
    return d


def _assert_match(got, draws):
    traces = []
    ref = R.diagnostics(draws, traces)
    for k in R.STATS:
        g, r = np.asarray(got[k]).reshape(-1), np.asarray(ref[k]).reshape(-1)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=k)
        fin = ~np.isnan(r)
        rtol = 1e-10 if k == "rhat" else 1e-9
        scale = np.abs(np.asarray(ref["sd"])) + np.abs(np.asarray(ref["mean"]))
        scale = float(np.max(scale[np.isfinite(scale)], initial=1.0))
        atol = 1e-12 * scale if k in ("mean", "sd", "mcse_mean") else 0.0
        np.testing.assert_allclose(g[fin], r[fin], rtol=rtol, atol=atol, err_msg=k)
    # Geyer's truncation is a discrete decision: the restatement must not sit on its edge
    for i, tr in enumerate(traces):
        for k, sets in _SETS.items():
            if np.isnan(np.asarray(ref[k]).reshape(-1)[i]):
                continue
            for s in sets:
                t = tr[s]
                assert t["hit_end"] or t["margin"] > 1e-9, (i, s, t)
    return ref


@pytest.mark.parametrize("C", [1, 2, 4, 32])
@pytest.mark.parametrize("S", [4, 5, 6, 101, 1000, 4097])
def test_matrix_route_matches_restatement(C, S):
    from bayesfmmm_amd import api
    d = _draws(S, C, 1000 * C + S)
    got = api.diagnostics(d)
    _assert_match(got, d)
    assert got["rhat"].shape == (7,)


def test_rows_beyond_the_lds_tier():
    from bayesfmmm_amd import api
    rng = np.random.default_rng(5)
    d = np.stack([rng.standard_normal((20001, 8)), _ar1(0.9, 20001, 8, rng), np.round(rng.standard_normal((20001, 8)))], axis=2)
    _assert_match(api.diagnostics(d), d)


def test_shapes_and_determinism():
    from bayesfmmm_amd import api
    rng = np.random.default_rng(8)
    x = _ar1(0.7, 999, 4, rng)[:, :, None, None] + rng.standard_normal((999, 4, 3, 2))
    a, b = api.diagnostics(x), api.diagnostics(x)
    for k in R.STATS:
        assert a[k].shape == (3, 2)
        assert a[k].tobytes() == b[k].tobytes(), k
    big = rng.standard_normal((3000, 4, 2))      # the global tier too
    a, b = api.diagnostics(big), api.diagnostics(big)
    for k in R.STATS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_bulk_and_tail_ess_depend_on_ranks_only():
    from bayesfmmm_amd import api
    rng = np.random.default_rng(9)
    x = np.stack([_ar1(0.5, 600, 4, rng), _ar1(0.9, 3000, 4, rng)[:600]], axis=2)
    a, b = api.diagnostics(x), api.diagnostics(np.exp(x))
    for k in ("ess_bulk", "ess_tail"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_matrix_argument_checks():
    from bayesfmmm_amd import api
    lib = api._lib_entry()
    buf = np.zeros(64)
    outs = [np.zeros(4) for _ in range(7)]
    p = [o.ctypes.data_as(api.c_double_p) for o in outs]
    x = buf.ctypes.data_as(api.c_double_p)

    def err(*args):
        assert lib.bfmmm_post_diagnostics(*args) != 0
        return lib.bfmmm_entry_last_error().decode()

    assert "'draws'" in err(None, 1, 2, 4, 0, *p)
    assert "'ess_tail'" in err(x, 1, 2, 4, 0, p[0], p[1], None, *p[3:])
    assert "'n_chains'" in err(x, 1, 0, 4, 0, *p)
    assert "'n_draws'" in err(x, 1, 2, 0, 0, *p)
    assert "'n_param'" in err(x, 0, 2, 4, 0, *p)
    with pytest.raises(api._lib.BfmmmError, match=r"2\^22"):
        api.diagnostics(np.zeros(((1 << 21) + 1, 2)))
    with pytest.raises(ValueError):
        api.diagnostics(np.zeros(10))


# ---- chain slots of a sampler batch ----------------------------------------------------------------------------------
def _gathered(smp, name, first, n_slots):
    """(n_slots, C, *draw shape) from the per-chain get_chain copies (draw order of the returned statistics)"""
    per = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        ch = smp.get_chain(name)
        if name == "tau":
            ch = ch.T                                   # (T, K) -> (K, T)
        ch = ch[..., first:first + n_slots]
        per.append(np.moveaxis(ch.reshape(-1, ch.shape[-1], order="F"), -1, 0))
    return np.stack(per, axis=1)


def _check_names(smp, names, first):
    T = smp.T
    for nm in names:
        got = smp.diagnostics(nm, first_slot=first)
        d = _gathered(smp, nm, first, T - first)
        ref = _assert_match({k: np.asarray(v).reshape(-1, order="F") for k, v in got.items()}, d)
        assert got["rhat"].size == d.shape[2], nm
        del ref


CHAIN_NAMES = ["nu", "Phi", "chi", "Z", "pi", "alpha_3", "delta", "A", "gamma", "tau", "sigma_sq", "loglik"]
COV_NAMES = ["eta", "xi", "tau_eta", "gamma_xi", "delta_xi", "A_xi"]


def test_chain_route_functional_with_covariates():
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=60, M=2, sigma_sq=0.01, seed=33)
    X = np.random.default_rng(2).standard_normal((sim["n"], 2))
    T, NCH = 200, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    smp.set_covariates(X, covariance_adj=True)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(S.SWEEP_WARM | S.COV_MEAN | S.COV_XI, T, seed=3, chain=0)
    smp.select_chain(2)                                 # ignored: every chain counts
    _check_names(smp, CHAIN_NAMES + COV_NAMES, 37)
    # chunks: a workspace of a few rows gives the same bits as one chunk
    one = smp.diagnostics("Z", first_slot=10)
    per_row = 8 * (NCH * (T - 10) + 7)
    small = smp.diagnostics("Z", first_slot=10, max_workspace_bytes=per_row * 7)      # n K rows in chunks of 7
    for k in R.STATS:
        assert one[k].tobytes() == small[k].tobytes(), k
    assert one["rhat"].shape == (sim["n"], sim["K"])
    smp.close()


def test_chain_route_multivariate_and_one_chain():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T = 150, 10, 3, 2, 200
    Y = rng.standard_normal((n, P))
    for NCH in (4, 1):
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, Y, n_chains=NCH)
        for q in range(NCH):
            smp.select_chain(q)
            smp.init_state(1, 17, chain=q)
        smp.run(bf.SWEEP_WARM, T, seed=17, chain=0)
        _check_names(smp, CHAIN_NAMES, 50 if NCH == 4 else 0)
        smp.close()


def test_chain_argument_checks():
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    sim = simulate_functional(n=24, M=2, sigma_sq=0.01, seed=1)
    b = make_sampler_batch(sim, 8, 2)
    for q in range(2):
        b.select_chain(q)
        b.init_state(1, 1, chain=q)
    b.run(bf.SWEEP_WARM, 8, seed=1)
    with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
        b.diagnostics("nu", first_slot=8)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        b.diagnostics("nu", first_slot=2, n_slots=7)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        b.diagnostics("nu", n_slots=0)
    with pytest.raises(_lib.BfmmmError, match="unknown name"):
        b.diagnostics("bogus")
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'"):
        b.diagnostics("nu", max_workspace_bytes=64)
    lib = b.lib
    outs = [np.zeros(64) for _ in range(7)]
    p = [o.ctypes.data_as(_lib.c_double_p) for o in outs]
    assert lib.bfmmm_chain_diagnostics(b.h, b"nu", 0, 8, 0, *p, 1) != 0
    assert "'capacity'" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_diagnostics(b.h, None, 0, 8, 0, *p, 64) != 0
    assert "'name'" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_diagnostics(b.h, b"nu", 0, 8, 0, p[0], None, *p[2:], 64) != 0
    assert "'ess_bulk'" in lib.bfmmm_last_error().decode()
    b.close()
