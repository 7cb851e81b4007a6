"""Observation-level PSIS-LOO and LOO-PIT of chain slots on the device (k_loo_pointwise, bfmmm_chain_loo_pointwise):
the four traces of Sampler.loo_pointwise against explicit Gaussian conditioning on the dense n_i x n_i covariance
(tests/loo_pointwise_ref.dense, fed the get_chain copies), every row; the pooled outputs against psis_ref / expect run on the
device's own traces; single-observation curves against curve_loglik; label and sign invariance; chunking, subsets, repeatability
and the argument checks.  The tolerances are loo_pointwise_ref.GPU_TOL_*: ten times the floors the two forms impose on each other
(tests/test_loo_pointwise_ref.py), not figures taken from the kernel."""
import re

import numpy as np
import pytest

import curve_ll_ref as CL
import loo_pointwise_ref as R
import psis_ref

pytestmark = pytest.mark.gpu

NAMES = ["nu", "Phi", "Z", "chi", "sigma_sq"]
LOO_ARRAYS = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic")
TRACES = ("loglik_trace", "pit_trace", "mean_trace", "var_trace")
# every tile boundary of a curve: below, at and above 16 (an MFMA row tile) and 64 (a row tile), and three tiles
EDGE_LENS = [1, 2, 15, 16, 17, 63, 64, 65, 130]


def _chains(smp, cov=False):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in NAMES + (["eta", "xi"] if cov else [])})
    return out


def _ragged(lens, seed):
    rng = np.random.default_rng(seed)
    ts = [np.sort(rng.uniform(0.0, 990.0, size=m)) for m in lens]
    ys = [np.sin(t / 150.0 + rng.uniform(0, 3)) * rng.uniform(0.5, 3) + 0.1 * rng.standard_normal(len(t)) for t in ts]
    return ts, ys


def _lens(n, edge, seed):
    """n curve lengths: the edge cases spread among short curves"""
    lens = [int(v) for v in np.random.default_rng(seed).integers(3, 13, size=n)]
    for j, m in enumerate(edge):
        lens[(j * n) // len(edge)] = m
    return lens


def _spline_sampler(lens, degree, n_knots, K, M, T, NCH, seed, X=None, covariance_adj=False):
    import bayesfmmm_amd as bf
    S = bf.sampler
    ts, ys = _ragged(lens, seed)
    ik = np.linspace(0.0, 990.0, n_knots + 2)[1:-1]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=degree, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, ys, ts, ik, [0.0, 990.0], n_chains=NCH)
    mask = S.SWEEP_WARM
    if X is not None:
        smp.set_covariates(X, covariance_adj=covariance_adj)
        mask |= S.COV_MEAN | (S.COV_XI if covariance_adj else 0)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, seed, chain=q)
    smp.run(mask, T, seed=seed)
    return smp, ys


def _check(smp, Y, B, first, S, X=None, covariance_adj=False, curves=None, label=""):
    """the traces against `dense`, every row; the pooled outputs against the restatements run on the device's traces"""
    from bayesfmmm_amd import api
    res = smp.loo_pointwise(curves=curves, first_slot=first, n_slots=S, trace=True)
    sel = list(range(smp.n)) if curves is None else list(curves)
    lens = [len(Y[i]) for i in sel]
    N, C = sum(lens), smp.n_chains
    np.testing.assert_array_equal(res["offsets"], np.concatenate([[0], np.cumsum(lens)]))
    for k in TRACES:
        assert res[k].shape == (N, C, S), k
    l, pit, m, v, z = R.dense_traces(Y, B, _chains(smp, X is not None), first, S, X, covariance_adj, curves)
    assert np.all(np.isfinite(l)) and np.all(v > 0), label
    errs = {"l": (R.rel_diff(res["loglik_trace"], l), R.GPU_TOL_L), "Phi(z)": (np.abs(res["pit_trace"] - pit), R.GPU_TOL_PIT),
            "m": (R.rel_diff(res["mean_trace"], m), R.GPU_TOL_M), "sqrt v": (R.rel_diff(np.sqrt(res["var_trace"]), np.sqrt(v)), R.GPU_TOL_SD)}
    for k, (e, tol) in errs.items():
        print(f"{label}: worst |device - dense| of {k} = {e.max():.3e} (tolerance {tol:.1e}) over {e.size} values")
    for k, (e, tol) in errs.items():
        assert e.max() <= tol, (label, k, float(e.max()), np.unravel_index(np.argmax(e), e.shape))
    # pooled: PSIS and the expectations of the device's own traces
    ll = res["loglik_trace"].reshape(N, C * S)
    ref = psis_ref.psis_loo(ll)
    scale = max(1.0, float(np.max(np.abs(ref["lppd"]))))
    for k in LOO_ARRAYS:
        if k != "pareto_k":
            np.testing.assert_allclose(res[k], ref[k], rtol=1e-8, atol=1e-8 * scale, err_msg=k)
    kg, kr = res["pareto_k"], ref["pareto_k"]
    np.testing.assert_array_equal(np.isinf(kg), np.isinf(kr))
    np.testing.assert_allclose(kg[np.isfinite(kr)], kr[np.isfinite(kr)], rtol=0, atol=1e-6)
    mt, second = res["mean_trace"].reshape(N, -1), (res["mean_trace"] ** 2 + res["var_trace"]).reshape(N, -1)
    e = np.array([R.expect(ll[r], np.vstack([res["pit_trace"].reshape(N, -1)[r], mt[r], second[r]])) for r in range(N)])
    np.testing.assert_allclose(res["pit"], e[:, 0], rtol=1e-8, atol=1e-8)
    assert np.all(np.abs(res["mean"] - e[:, 1]) <= 1e-8 * np.abs(e[:, 1]) + 1e-8 * np.max(np.abs(mt), axis=1))
    # sd^2 = E2 - E1^2 with both expectations good to 1e-8 (relative): sd^2 moves by at most 1e-8 (E2 + 2 E1^2), sd by that over 2 sd
    sd_ref = np.sqrt(np.maximum(0.0, e[:, 2] - e[:, 1] ** 2))
    assert np.all(sd_ref > 0)
    assert np.all(np.abs(res["sd"] - sd_ref) <= 1e-8 * (e[:, 2] + 2.0 * e[:, 1] ** 2) / (2.0 * sd_ref) + 1e-8 * sd_ref)
    # totals and per-curve sums
    tot = api.loo_totals({k: res[k] for k in LOO_ARRAYS}, C * S)
    for k, val in tot.items():
        if k not in LOO_ARRAYS:
            assert res[k] == val or (np.isnan(res[k]) and np.isnan(val)), k
    off = res["offsets"]
    np.testing.assert_array_equal(res["curve_elpd_loo"], [res["pointwise_elpd_loo"][off[j]:off[j + 1]].sum() for j in range(len(sel))])
    assert np.all((res["pit"] >= 0) & (res["pit"] <= 1))
    # a curve of one observation: nothing to condition on, l is the curve's marginal log-density (k_chain_curve_ll)
    ones = [j for j, n_i in enumerate(lens) if n_i == 1]
    if ones:
        cl = smp.curve_loglik(first_slot=first, n_slots=S)
        for j in ones:
            assert R.rel_diff(res["loglik_trace"][off[j]], cl[sel[j]]).max() <= CL.GPU_TOL, j
    return res


@pytest.fixture(scope="module")
def batch():
    """P = 12, K = 3, M = 2, four chains of 30 slots, 40 ragged curves with every edge length"""
    lens = _lens(40, EDGE_LENS, 1)
    smp, ys = _spline_sampler(lens, 3, 8, 3, 2, 30, 4, seed=11)
    yield smp, ys
    smp.close()


def test_ragged_functional_matches_dense(batch):
    smp, ys = batch
    assert smp.P == 12 and sorted(set(EDGE_LENS)) == sorted(set(EDGE_LENS) & {len(y) for y in ys})
    _check(smp, ys, smp.get_basis(), 22, 8, label="P=12 K=3 M=2 C=4")


@pytest.mark.parametrize("K,M,degree,n_knots,edge", [
    (2, 16, 2, 37, [1, 2, 17, 65]),       # P = 40: 64-lane records, ten k-steps; M + 1 = 17: the second column tile
    (2, 1, 3, 8, [1, 16, 64]),            # M = 1
])
def test_shapes_match_dense(K, M, degree, n_knots, edge):
    smp, ys = _spline_sampler(_lens(12, edge, 2), degree, n_knots, K, M, 8, 1, seed=7)
    _check(smp, ys, smp.get_basis(), 2, 6, label=f"P={smp.P} K={K} M={M} C=1")
    smp.close()


@pytest.mark.parametrize("covariance_adj", [True, False])
def test_covariates_match_dense(covariance_adj):
    lens = _lens(12, [1, 17, 65], 3)
    X = np.random.default_rng(2).standard_normal((len(lens), 2))
    smp, ys = _spline_sampler(lens, 3, 8, 3, 2, 8, 2, seed=5, X=X, covariance_adj=covariance_adj)
    _check(smp, ys, smp.get_basis(), 3, 5, X=X, covariance_adj=covariance_adj, label=f"D=2 cov_adj={covariance_adj}")
    smp.close()


def test_tensor_product_basis_matches_dense():
    """a create_from_basis handle: the basis rows come from the handle's host copy, chunk by chunk"""
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    K, M, T, NCH = 2, 2, 8, 2
    sim = simulate_tensor(10, K, M, [2, 2], [2, 2], seed=311, n_pts=90)       # 25 basis functions, band 12; 45 to 90 points a curve
    assert max(len(y) for y in sim["y"]) > 64
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 5, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    one = _check(smp, sim["y"], sim["B"], 2, 6, label=f"tensor basis P={sim['P']} band={sim['band']}")
    few = smp.loo_pointwise(first_slot=2, n_slots=6, trace=True, max_workspace_bytes=_tile_budget(smp, 2, 6, 3))
    for k in LOO_ARRAYS + TRACES + ("pit", "mean", "sd"):
        assert one[k].tobytes() == few[k].tobytes(), k
    smp.close()


def test_multivariate_matches_dense():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T, NCH = 30, 10, 3, 2, 10, 2
    Y = rng.standard_normal((n, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    res = _check(smp, list(Y), None, 4, 6, label="multivariate")
    assert res["pit"].shape == (n * P,)
    smp.close()


def _tile_budget(smp, first, S, tiles):
    """max_workspace_bytes for chunks of `tiles` row tiles, from the plan the refusal of a one-byte budget states"""
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' below") as ei:
        smp.loo_pointwise(first_slot=first, n_slots=S, max_workspace_bytes=1)
    shared, per = (int(v) for v in re.search(r"\((\d+) shared by all tiles \+ (\d+) per tile\)", str(ei.value)).groups())
    return shared + tiles * per


def test_chunks_subsets_and_repeatability(batch):
    smp, ys = batch
    first, S = 5, 21
    one = smp.loo_pointwise(first_slot=first, n_slots=S, trace=True)
    again = smp.loo_pointwise(first_slot=first, n_slots=S, trace=True)
    few = smp.loo_pointwise(first_slot=first, n_slots=S, trace=True, max_workspace_bytes=_tile_budget(smp, first, S, 3))
    keys = LOO_ARRAYS + TRACES + ("pit", "mean", "sd", "curve_elpd_loo")
    for k in keys:
        assert one[k].tobytes() == again[k].tobytes(), k
        assert one[k].tobytes() == few[k].tobytes(), k       # chunks of three tiles split the curves of 130 and 65 observations
    assert one["elpd_loo"] == few["elpd_loo"] and one["n_khat_above"] == few["n_khat_above"]
    # without the traces the same values
    plain = smp.loo_pointwise(first_slot=first, n_slots=S)
    assert not any(k in plain for k in TRACES)
    for k in LOO_ARRAYS + ("pit", "mean", "sd"):
        assert one[k].tobytes() == plain[k].tobytes(), k
    # a subset, out of order and with a repeat: the rows of those curves
    long_ = int(np.argmax([len(y) for y in ys]))
    curves = [7, long_, 0, 7]
    sub = smp.loo_pointwise(curves=curves, first_slot=first, n_slots=S, trace=True)
    off = one["offsets"]
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in curves])
    assert sub["offsets"][-1] == len(rows)
    for k in LOO_ARRAYS + TRACES + ("pit", "mean", "sd"):
        assert sub[k].tobytes() == np.ascontiguousarray(one[k][rows]).tobytes(), k
    # another slot range, hence another grid and other staging batches
    other = smp.loo_pointwise(first_slot=first + 3, n_slots=10, trace=True)
    for k in TRACES:
        assert other[k].tobytes() == np.ascontiguousarray(one[k][:, :, 3:13]).tobytes(), k
    # the timers of the call
    import ctypes as C
    ms, cnt = C.c_double(0), C.c_int64(0)
    for name in (b"loo_pointwise", b"loo_pointwise_psis"):
        assert smp.lib.bfmmm_get_timing(smp.h, name, C.byref(ms), C.byref(cnt)) == 0
        assert ms.value > 0 and cnt.value >= 1, name


def test_label_and_sign_invariance():
    import bayesfmmm_amd as bf
    from simdata import simulate_functional
    from test_gpu_chain_batch import _states, make_sampler_batch
    S = bf.sampler
    sim = simulate_functional(n=20, M=2, sigma_sq=0.01, seed=36, ragged=True)
    st = _states(sim, 1)[0]
    perm = [2, 0, 1]
    cvals = [8.0, 10.0, 12.0]
    a = make_sampler_batch(sim, 2, 1, c=cvals)
    b = make_sampler_batch(sim, 2, 1, c=[cvals[k] for k in perm])
    a.set_state(**st)
    a.run(S.U_LOGLIK, 1, seed=1)
    pst = dict(st)
    for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
        pst[nm] = np.asarray(st[nm])[perm]
    pst["Z"] = np.asarray(st["Z"])[:, perm]
    b.set_state(**pst)
    b.run(S.U_LOGLIK, 1, seed=1)
    np.testing.assert_array_equal(b.get_chain("nu")[:, :, 0], a.get_chain("nu")[perm, :, 0])
    assert not np.array_equal(b.get_chain("nu")[:, :, 0], a.get_chain("nu")[:, :, 0])
    ra, rb = a.loo_pointwise(first_slot=0, n_slots=1, trace=True), b.loo_pointwise(first_slot=0, n_slots=1, trace=True)
    e = R.rel_diff(rb["loglik_trace"], ra["loglik_trace"])
    print(f"label permutation: worst relative difference of l {e.max():.3e}")
    assert e.max() <= R.GPU_TOL_L
    assert R.rel_diff(rb["mean_trace"], ra["mean_trace"]).max() <= R.GPU_TOL_M
    # against the dense form too, so that agreement is not two wrong answers
    l, pit, m, v, z = R.dense_traces(sim["y"], a.get_basis(), _chains(a), 0, 1)
    assert R.rel_diff(ra["loglik_trace"], l).max() <= R.GPU_TOL_L
    # the sign of one (Phi_.m, chi_.m) pair
    fst = dict(pst)
    fst["Phi"] = np.array(pst["Phi"], copy=True)
    fst["Phi"][:, :, 1] *= -1.0
    fst["chi"] = np.array(pst["chi"], copy=True)
    fst["chi"][:, 1] *= -1.0
    b.set_state(**fst)
    b.run(S.U_LOGLIK, 1, first_iter=1, seed=1)
    np.testing.assert_array_equal(b.get_chain("Phi")[:, :, 1, 1], -b.get_chain("Phi")[:, :, 1, 0])
    rf = b.loo_pointwise(first_slot=1, n_slots=1, trace=True)
    e = R.rel_diff(rf["loglik_trace"], rb["loglik_trace"])
    print(f"eigen-sign flip: worst relative difference of l {e.max():.3e}")
    assert e.max() <= R.GPU_TOL_L
    assert R.rel_diff(rf["mean_trace"], rb["mean_trace"]).max() <= R.GPU_TOL_M
    a.close()
    b.close()


def test_argument_checks(batch):
    from bayesfmmm_amd import _lib
    smp, ys = batch
    T = smp.T
    call = smp.loo_pointwise
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_pointwise: 'first_slot'"):
        call(first_slot=T)
    with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
        call(first_slot=-1, n_slots=4)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        call(first_slot=2, n_slots=T - 1)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        call(n_slots=0)
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' must not be negative"):
        call(max_workspace_bytes=-1)
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' below"):
        call(max_workspace_bytes=64)
    with pytest.raises(ValueError, match="'curves'"):
        call(curves=[0, smp.n])
    smp.REFINE_TRACE_BYTES = 1000                          # on the instance: the class keeps its cap
    try:
        with pytest.raises(ValueError, match="REFINE_TRACE_BYTES"):
            call(trace=True)
    finally:
        del smp.REFINE_TRACE_BYTES
    lib = smp.lib
    N = sum(len(y) for y in ys)
    outs = [np.zeros(N) for _ in range(9)]
    p = [o.ctypes.data_as(_lib.c_double_p) for o in outs]
    bad = np.array([0, smp.n], dtype=np.int32)

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    assert "'capacity' below " + str(N) in err(lib.bfmmm_chain_loo_pointwise(smp.h, None, 0, 0, 4, 0, *p, None, None, None, None, N - 1))
    assert "'pit' is null" in err(lib.bfmmm_chain_loo_pointwise(smp.h, None, 0, 0, 4, 0, *p[:6], None, p[7], p[8], None, None, None, None, N))
    assert "'h' is null" in err(lib.bfmmm_chain_loo_pointwise(None, None, 0, 0, 4, 0, *p, None, None, None, None, N))
    assert "'curves'[1]" in err(lib.bfmmm_chain_loo_pointwise(smp.h, bad.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), 2, 0, 4, 0, *p,
                                                              None, None, None, None, N))
    assert "'n_curves'" in err(lib.bfmmm_chain_loo_pointwise(smp.h, bad.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), 0, 0, 4, 0, *p,
                                                             None, None, None, None, N))
