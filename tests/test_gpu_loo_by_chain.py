"""PSIS-LOO chain by chain and the stacking weights of chains (bfmmm_chain_loo_by_chain, Sampler.loo_by_chain, Sampler.chain_stacking;
DESIGN.md 7v).  The entry hands the pooled calls' chunk matrix to the unchanged PSIS pass as rows x C rows of n_slots draws, so every
check is on bits: entry [r, c] against api.psis_loo of chain c's log-density matrix, chunks and selections against one chunk, one
chain against the pooled calls, and the pooled calls before and after.  The small batches are those of the other LOO tests: a
ragged spline sampler with every tile edge, the multivariate model with n = 30 and P = 10, and a tensor-product basis."""
import re

import numpy as np
import pytest

import stacking_ref as R

pytestmark = pytest.mark.gpu

LOO_ARRAYS = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic")
EDGE_LENS = [1, 2, 15, 16, 17, 63, 64, 65, 130]
STATE = ["nu", "Phi", "Z", "chi", "sigma_sq"]


def _spline_sampler(n, T, NCH, seed):
    """P = 12, K = 3, M = 2: n ragged curves with every tile edge among short ones"""
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(3, 13, size=n)]
    for j, m in enumerate(EDGE_LENS):
        lens[(j * n) // len(EDGE_LENS)] = m
    ts = [np.sort(rng.uniform(0.0, 990.0, size=m)) for m in lens]
    ys = [np.sin(t / 150.0 + rng.uniform(0, 3)) * rng.uniform(0.5, 3) + 0.1 * rng.standard_normal(len(t)) for t in ts]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=3, n_eigen=2, basis_degree=3, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, ys, ts, np.linspace(0.0, 990.0, 10)[1:-1], [0.0, 990.0], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, seed, chain=q)
    smp.run(bf.sampler.SWEEP_WARM, T, seed=seed)
    return smp, ys


def _same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _against_psis(smp, first, S, label):
    """both units of loo_by_chain against api.psis_loo of each chain's matrix, bit for bit; returns the two results"""
    from bayesfmmm_amd import api
    C = smp.n_chains
    cl = smp.curve_loglik(first_slot=first, n_slots=S)
    tr = smp.loo_pointwise(first_slot=first, n_slots=S, trace=True)
    out = []
    for unit, ll in (("curve", cl), ("observation", tr["loglik_trace"])):
        by = smp.loo_by_chain(unit=unit, first_slot=first, n_slots=S)
        rows = ll.shape[0]
        for c in range(C):
            ref = api.psis_loo(np.ascontiguousarray(ll[:, c, :]))
            for k in LOO_ARRAYS:
                assert by[k].shape == (rows, C)
                _same(np.ascontiguousarray(by[k][:, c]), ref[k], (label, unit, c, k))
            assert by["elpd_loo"][c] == ref["elpd_loo"] and by["n_khat_above"][c] == ref["n_khat_above"]
            assert by["se_elpd_loo"][c] == ref["se_elpd_loo"] or rows < 2
            assert by["khat_threshold"] == ref["khat_threshold"]
        if unit == "observation":
            np.testing.assert_array_equal(by["offsets"], tr["offsets"])
        out.append(by)
    return out


@pytest.fixture(scope="module")
def batch():
    """two chains of 30 slots, 24 ragged curves"""
    smp, ys = _spline_sampler(24, 30, 2, seed=11)
    yield smp, ys
    smp.close()


@pytest.mark.parametrize("first,S", [(21, 9), (4, 26)])      # a tail too short for the Pareto fit (k = inf), and one that is smoothed
def test_spline_batch_matches_psis_of_each_chain(batch, first, S):
    smp, ys = batch
    by_curve, by_obs = _against_psis(smp, first, S, "spline")
    assert np.all(np.isinf(by_obs["pareto_k"])) == (S < 21)
    assert by_curve["pareto_k"].shape == (smp.n, 2) and by_obs["pareto_k"].shape == (sum(len(y) for y in ys), 2)


def _budget(smp, tiles, **kw):
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_by_chain: 'max_workspace_bytes' below") as ei:
        smp.loo_by_chain(max_workspace_bytes=1, **kw)
    shared, per = (int(v) for v in re.search(r"\((\d+) shared by all tiles \+ (\d+) per tile\)", str(ei.value)).groups())
    return shared + tiles * per


def test_chunks_and_selections_give_the_same_bits(batch):
    smp, ys = batch
    first, S = 4, 26
    one = smp.loo_by_chain(unit="observation", first_slot=first, n_slots=S)
    few = smp.loo_by_chain(unit="observation", first_slot=first, n_slots=S, max_workspace_bytes=_budget(smp, 3, first_slot=first, n_slots=S))
    again = smp.loo_by_chain(unit="observation", first_slot=first, n_slots=S)
    long_ = int(np.argmax([len(y) for y in ys]))
    curves = [7, long_, 0, 7]
    sub = smp.loo_by_chain(unit="observation", curves=curves, first_slot=first, n_slots=S,
                           max_workspace_bytes=_budget(smp, 2, curves=curves, first_slot=first, n_slots=S))
    off = one["offsets"]
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in curves])
    assert sub["offsets"][-1] == len(rows)
    for k in LOO_ARRAYS:
        _same(one[k], few[k], k)             # chunks of three tiles split the curves of 130 and 65 observations
        _same(one[k], again[k], k)
        _same(sub[k], np.ascontiguousarray(one[k][rows]), k)
    cone = smp.loo_by_chain(unit="curve", first_slot=first, n_slots=S)
    cfew = smp.loo_by_chain(unit="curve", first_slot=first, n_slots=S, max_workspace_bytes=8 * 2 * S * 5)      # five curves a chunk
    for k in LOO_ARRAYS:
        _same(cone[k], cfew[k], k)


def test_the_pooled_calls_are_not_disturbed(batch):
    smp, ys = batch
    first, S = 4, 26
    calls = (lambda: smp.loo(first_slot=first, n_slots=S), lambda: smp.loo_pointwise(first_slot=first, n_slots=S),
             lambda: smp.loo_blocks(block_size=5, first_slot=first, n_slots=S))
    before = [f() for f in calls]
    smp.loo_by_chain(unit="curve", first_slot=first, n_slots=S)
    smp.loo_by_chain(unit="observation", first_slot=first, n_slots=S, max_workspace_bytes=_budget(smp, 3, first_slot=first, n_slots=S))
    for b, a in zip(before, [f() for f in calls]):
        assert sorted(a) == sorted(b)
        for k, v in b.items():
            if isinstance(v, np.ndarray):
                _same(v, a[k], k)
            else:
                assert v == a[k] or (v != v and a[k] != a[k]), k


def test_one_chain_is_the_pooled_call():
    smp, ys = _spline_sampler(12, 10, 1, seed=7)
    pooled = {"curve": smp.loo(first_slot=2, n_slots=8), "observation": smp.loo_pointwise(first_slot=2, n_slots=8)}
    for unit, ref in pooled.items():
        by = smp.loo_by_chain(unit=unit, first_slot=2, n_slots=8)
        for k in LOO_ARRAYS:
            _same(by[k][:, 0].copy(), ref[k], (unit, k))
        assert by["elpd_loo"][0] == ref["elpd_loo"] and by["khat_threshold"] == ref["khat_threshold"]
    smp.close()


def test_multivariate_matches_psis_of_each_chain():
    import bayesfmmm_amd as bf
    n, P, K, M, T, NCH = 30, 10, 3, 2, 10, 2
    Y = np.random.default_rng(4).standard_normal((n, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    by_curve, by_obs = _against_psis(smp, 4, 6, "multivariate")
    assert by_obs["lppd"].shape == (n * P, NCH)
    smp.close()


def test_tensor_product_basis_matches_psis_of_each_chain():
    """a create_from_basis handle: the basis rows come from the handle's host copy, chunk by chunk"""
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    K, M, T, NCH = 2, 2, 8, 2
    sim = simulate_tensor(10, K, M, [2, 2], [2, 2], seed=311, n_pts=90)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 5, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    by_curve, by_obs = _against_psis(smp, 2, 6, "tensor basis")
    few = smp.loo_by_chain(first_slot=2, n_slots=6, max_workspace_bytes=_budget(smp, 3, first_slot=2, n_slots=6))
    for k in LOO_ARRAYS:
        _same(by_obs[k], few[k], k)
    smp.close()


def test_chain_stacking_and_a_copied_chain():
    """chain_stacking is api.stacking of the by-chain matrix; a chain loaded as a copy of another shares the weight the single chain
    gets.  With the start (w_0, w_1 / 2, w_1 / 2) the sum of the two copies' weights follows, in exact arithmetic, the iterates of the
    two-candidate problem from (w_0, w_1): after t iterations the two differ by rounding alone, at most 64 eps an iteration by the
    bound of tests/test_gpu_stacking.py."""
    from bayesfmmm_amd import api
    smp, ys = _spline_sampler(16, 30, 3, seed=23)
    first, S = 4, 26
    smp.select_chain(1)
    copy = {nm: smp.get_chain(nm) for nm in STATE}
    smp.load_chain(copy, chain=2)
    res = smp.chain_stacking(first_slot=first, n_slots=S)
    by = res["by_chain"]
    Lm = by["pointwise_elpd_loo"]
    assert Lm.shape[1] == 3 and res["weights"].shape == (3,)
    _same(np.ascontiguousarray(Lm[:, 1]), np.ascontiguousarray(Lm[:, 2]), "the copied chain")
    direct = api.stacking(Lm)
    _same(res["weights"], direct["weights"], "weights")
    assert res["objective"] == direct["objective"] and res["gap"] == direct["gap"] and res["n_iter"] == direct["n_iter"]
    # certified, and as good as the two-candidate optimum
    n = Lm.shape[0]
    pair = api.stacking(Lm[:, :2])
    assert res["converged"] and pair["converged"] and res["gap"] <= 1e-8
    assert abs(res["objective"] - pair["objective"]) <= n * max(res["gap"], pair["gap"]) + 8 * R.EPS * abs(pair["objective"])
    at = R.evaluate(Lm, res["weights"])
    assert float(at["gap"]) <= 1e-8 + 64 * R.EPS * np.sqrt(n)
    # the sum of the two weights at a fixed count
    t = 64
    three = api.stacking(Lm, init=[0.5, 0.25, 0.25], max_iter=t, tol=0.0)
    two = api.stacking(Lm[:, :2], init=[0.5, 0.5], max_iter=t, tol=0.0)
    assert three["weights"][1] == three["weights"][2]
    assert abs(three["weights"][1] + three["weights"][2] - two["weights"][1]) <= t * 64 * R.EPS
    assert abs(three["weights"][0] - two["weights"][0]) <= t * 64 * R.EPS
    # f moves by at most sum_q g_q |dw_q| <= n (1 + gap) sum_q |dw_q|, and each of the two sums rounds
    assert abs(three["objective"] - two["objective"]) <= 64 * R.EPS * float(np.sum(np.abs(Lm[:, 0]))) + 4 * n * t * 64 * R.EPS
    cs = smp.chain_stacking(unit="curve", first_slot=first, n_slots=S, max_iter=32, tol=0.0)
    assert cs["weights"].shape == (3,) and cs["n_iter"] == 32 and cs["by_chain"]["lppd"].shape == (smp.n, 3)
    smp.close()


def test_argument_checks(batch):
    from bayesfmmm_amd import _lib
    smp, ys = batch
    T = smp.T
    call = smp.loo_by_chain
    with pytest.raises(ValueError, match="'unit' must be one of"):
        call(unit="block")
    with pytest.raises(ValueError, match="'curves' goes with unit"):
        call(unit="curve", curves=[0])
    with pytest.raises(ValueError, match="'curves'"):
        call(curves=[0, smp.n])
    for unit in ("curve", "observation"):
        with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_by_chain: 'first_slot'"):
            call(unit=unit, first_slot=T)
        with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
            call(unit=unit, first_slot=-1, n_slots=4)
        with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
            call(unit=unit, first_slot=2, n_slots=T - 1)
        with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
            call(unit=unit, n_slots=0)
        with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' must not be negative"):
            call(unit=unit, max_workspace_bytes=-1)
        with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' below"):
            call(unit=unit, max_workspace_bytes=64)
    lib = smp.lib
    N, C = sum(len(y) for y in ys), smp.n_chains
    outs = [np.zeros(N * C) for _ in range(6)]
    p = [o.ctypes.data_as(_lib.c_double_p) for o in outs]
    bad = np.array([0, smp.n], dtype=np.int32)
    ip = bad.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    assert "'unit' must be 0 (curve) or 1 (observation), got 2" in err(lib.bfmmm_chain_loo_by_chain(smp.h, 2, None, 0, 0, 4, 0, *p, N * C))
    assert "'unit' must be 0" in err(lib.bfmmm_chain_loo_by_chain(smp.h, -1, None, 0, 0, 4, 0, *p, N * C))
    assert "'curves' must be null with 'unit' 0" in err(lib.bfmmm_chain_loo_by_chain(smp.h, 0, ip, 1, 0, 4, 0, *p, N * C))
    assert "'capacity' below " + str(N * C) in err(lib.bfmmm_chain_loo_by_chain(smp.h, 1, None, 0, 0, 4, 0, *p, N * C - 1))
    assert "'capacity' below " + str(smp.n * C) in err(lib.bfmmm_chain_loo_by_chain(smp.h, 0, None, 0, 0, 4, 0, *p, smp.n * C - 1))
    assert "'pareto_k' is null" in err(lib.bfmmm_chain_loo_by_chain(smp.h, 1, None, 0, 0, 4, 0, *p[:3], None, *p[4:], N * C))
    assert "'h' is null" in err(lib.bfmmm_chain_loo_by_chain(None, 1, None, 0, 0, 4, 0, *p, N * C))
    assert "'curves'[1]" in err(lib.bfmmm_chain_loo_by_chain(smp.h, 1, ip, 2, 0, 4, 0, *p, N * C))
    assert "'n_curves'" in err(lib.bfmmm_chain_loo_by_chain(smp.h, 1, ip, 0, 0, 4, 0, *p, N * C))
