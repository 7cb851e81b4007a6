"""Pooled co-membership matrix of curves from chain slots on the device (kernels_similarity.hip):
Sampler.similarity against the numpy restatement (tests/similarity_ref.py) fed the get_chain("Z") copies, entry by entry within
the derived bounds |mean - ref| <= 2 (N + K + 2) 2^-52 ref and |sd - ref| <= 4 N 2^-52 ref + 4 (K + 1) 2^-52 sqrt(N / (N - 1))
(chain_mean: the first with S for N); edge tiles in both directions, K of one and two MFMAs padded and full, both block shapes,
symmetry bit for bit, row selection, one and two draws, chunking, repeatability, untouched state, argument checks, timing."""
import ctypes as C
import re

import numpy as np
import pytest

import similarity_ref as R
from test_gpu_chain_batch import _states, make_sampler_batch
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

STATE = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "tau", "gamma", "Phi", "loglik"]
KEYS = ("mean", "sd", "chain_mean")


def _chains(smp):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append(smp.get_chain("Z"))
    return out


def _check(got, ref, C_, S, K, label):
    """every entry of the device result within the bounds of the restatement; prints the worst ratio to the bound"""
    N = C_ * S
    assert got["mean"].shape == ref["mean"].shape and got["chain_mean"].shape == ref["chain_mean"].shape, label
    assert np.all(np.isfinite(ref["mean"])) and ref["mean"].max() > 0, label
    worst = {}
    for key, n_sum in (("mean", N), ("chain_mean", S)):
        b = R.mean_bound(ref[key], n_sum, K)
        err = np.abs(got[key] - ref[key])
        worst[key] = float(np.max(err[b > 0] / b[b > 0]))
        assert np.all(err <= b), (label, key, worst[key])
    if N < 2:
        assert np.all(np.isnan(got["sd"])), label
    else:
        b = R.sd_bound(ref["sd"], N, K)
        err = np.abs(got["sd"] - ref["sd"])
        worst["sd"] = float(np.max(err / b))
        assert np.all(err <= b), (label, "sd", worst["sd"])
    print(f"{label} N={N} K={K}: worst |device - numpy| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def _same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def func():
    """n = 61 ragged, K = 3, 4 chains, T = 30; slots 7 .. 29 are 92 draws.  The full result and its restatement, computed once."""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=33, ragged=True)
    T, NCH = 30, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(bf.SWEEP_WARM, T, seed=3)
    chains = _chains(smp)
    first, S = 7, T - 7
    d = dict(smp=smp, chains=chains, first=first, S=S, K=sim["K"], ref=R.similarity(chains, first, S),
             full=smp.similarity(per_chain=True, first_slot=first, n_slots=S))
    for v in d["ref"].values():
        v.setflags(write=False)
    yield d
    smp.close()


def test_functional_full_matrix_matches_restatement(func):
    smp = func["smp"]
    assert func["full"]["mean"].shape == (61, 61) and func["full"]["sd"].shape == (61, 61) and func["full"]["chain_mean"].shape == (61, 4, 61)
    assert func["K"] == 3
    _check(func["full"], func["ref"], smp.n_chains, func["S"], func["K"], "functional n=61")
    # co-memberships of rows on the simplex
    assert func["full"]["mean"].min() >= 0.0 and func["full"]["mean"].max() <= 1.0 + 1e-12


def test_matrix_is_symmetric_bit_for_bit(func):
    full = func["full"]
    for k in ("mean", "sd"):
        assert full[k].tobytes() == np.ascontiguousarray(full[k].T).tobytes(), k
    cm = full["chain_mean"]
    assert cm.tobytes() == np.ascontiguousarray(cm.transpose(2, 1, 0)).tobytes()


def test_both_block_shapes_give_the_same_bits(func):
    smp = func["smp"]
    try:
        for block in (1, 2):
            smp.lib.bfmmm_set_similarity_block(block)
            got = smp.similarity(per_chain=True, first_slot=func["first"], n_slots=func["S"])
            _same(got, func["full"])
            sel = smp.similarity(curves=[60, 3, 3, 17], per_chain=True, first_slot=func["first"], n_slots=func["S"])
            for k in KEYS:
                assert sel[k].tobytes() == np.ascontiguousarray(func["full"][k][[60, 3, 3, 17]]).tobytes(), (block, k)
    finally:
        smp.lib.bfmmm_set_similarity_block(0)


@pytest.mark.parametrize("K,M,degree,n_internal,n", [
    (2, 1, 1, 3, 32),      # one MFMA, k padded with zeros
    (4, 2, 2, 6, 48),      # one MFMA, full
    (5, 2, 3, 4, 48),      # two MFMAs, the second padded
    (7, 1, 3, 4, 80),      # test_gpu_shapes' K = 7 simulation
    (8, 2, 2, 5, 96),      # test_gpu_shapes' K = 8 simulation: two full MFMAs
])
def test_k_shapes(K, M, degree, n_internal, n):
    import bayesfmmm_amd as bf
    from test_gpu_shapes import simulate
    sim = simulate(n, K, M, degree, n_internal, seed=100 + K * 10 + M)
    T, NCH, first = 9, 2, 2
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=degree, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 40 + K, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    ref = R.similarity(_chains(smp), first, T - first)
    got = smp.similarity(per_chain=True, first_slot=first)
    _check(got, ref, NCH, T - first, K, f"K={K} n={n}")
    try:
        for block in (1, 2):
            smp.lib.bfmmm_set_similarity_block(block)
            _same(smp.similarity(per_chain=True, first_slot=first), got)
    finally:
        smp.lib.bfmmm_set_similarity_block(0)
    smp.close()


def test_multivariate_model():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T, NCH, first = 70, 10, 3, 2, 24, 2, 6
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    ref = R.similarity(_chains(smp), first, T - first)
    _check(smp.similarity(per_chain=True, first_slot=first), ref, NCH, T - first, K, "multivariate n=70")
    smp.close()


def test_functional_with_covariates():
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=60, M=2, sigma_sq=0.01, seed=34)
    X = np.random.default_rng(2).standard_normal((sim["n"], 2))
    T, NCH, first = 24, 3, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    smp.set_covariates(X, covariance_adj=True)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(S.SWEEP_WARM | S.COV_MEAN | S.COV_XI, T, seed=3)
    ref = R.similarity(_chains(smp), first, T - first)
    _check(smp.similarity(per_chain=True, first_slot=first), ref, NCH, T - first, sim["K"], "functional D=2")
    smp.close()


@pytest.mark.parametrize("curves", [[0], [60, 3, 3, 17], [44, 2, 59, 31, 7, 60, 0, 18, 25, 9, 53, 12, 38, 1, 47, 20, 5]])
def test_row_selection_equals_rows_of_the_full_result(func, curves):
    smp, full = func["smp"], func["full"]
    got = smp.similarity(curves=curves, per_chain=True, first_slot=func["first"], n_slots=func["S"])
    assert got["mean"].shape == (len(curves), 61) and got["chain_mean"].shape == (len(curves), 4, 61)
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(full[k][curves]).tobytes(), k


def test_draw_count_edges(func):
    import bayesfmmm_amd as bf
    smp, chains = func["smp"], func["chains"]
    # sd and per_chain separately and together
    a = smp.similarity(sd=False, first_slot=func["first"], n_slots=func["S"])
    assert set(a) == {"mean"}
    b = smp.similarity(sd=False, per_chain=True, first_slot=func["first"], n_slots=func["S"])
    assert set(b) == {"mean", "chain_mean"}
    c = smp.similarity(first_slot=func["first"], n_slots=func["S"])
    assert set(c) == {"mean", "sd"}
    _same(a, func["full"], ("mean",))
    _same(b, func["full"], ("mean", "chain_mean"))
    _same(c, func["full"], ("mean", "sd"))
    # two draws per chain, and one slot of four chains
    for first, S in ((11, 2), (5, 1)):
        _check(smp.similarity(per_chain=True, first_slot=first, n_slots=S), R.similarity(chains, first, S), 4, S, 3, f"slots {first}+{S}")
    # one draw and two draws in all: a single chain
    sim = simulate_functional(n=31, M=2, sigma_sq=0.01, seed=37, ragged=True)
    one = make_sampler_batch(sim, 6, 1)
    one.set_state(**_states(sim, 1)[0])
    one.run(bf.SWEEP_WARM, 6, seed=3)
    Z = one.get_chain("Z")
    got = one.similarity(per_chain=True, first_slot=4, n_slots=1)
    d = R.draws([Z], 4, 1)[:, :, 0, 0]
    assert np.all(np.isnan(got["sd"]))
    assert np.all(np.abs(got["mean"] - d) <= R.mean_bound(d, 1, 3))
    assert got["chain_mean"][:, 0].tobytes() == got["mean"].tobytes()
    _check(one.similarity(per_chain=True, first_slot=3, n_slots=2), R.similarity([Z], 3, 2), 1, 2, 3, "two draws")
    one.close()


def test_firmly_clustered_pair_meets_the_sd_bound(func):
    """the pair whose co-membership moves least: where a one-pass variance would lose its digits"""
    ref, full, N, K = func["ref"], func["full"], 4 * func["S"], func["K"]
    i, j = np.unravel_index(np.argmin(ref["sd"]), ref["sd"].shape)
    sd, mean = ref["sd"][i, j], ref["mean"][i, j]
    err, b = abs(full["sd"][i, j] - sd), R.sd_bound(sd, N, K)
    print(f"firmest pair ({i}, {j}): sd / mean = {sd:.3e} / {mean:.3e} = {sd / mean:.3e}; |device - numpy| / bound = {err / b:.3e}")
    assert err <= b
    assert abs(full["mean"][i, j] - mean) <= R.mean_bound(mean, N, K)


def test_chunks_and_repeatability(func):
    from bayesfmmm_amd import _lib
    smp, first, S, full = func["smp"], func["first"], func["S"], func["full"]
    n, C_ = smp.n, smp.n_chains
    per_row = 8 * n * (2 + C_)
    with pytest.raises(_lib.BfmmmError, match=r"'max_workspace_bytes' below the (\d+) bytes of one row") as ei:
        smp.similarity(per_chain=True, first_slot=first, n_slots=S, max_workspace_bytes=per_row - 1)
    assert re.search(r"below the (\d+) bytes", str(ei.value)).group(1) == str(per_row)
    for chunks, budget in ((1, 0), (3, per_row * 21), (n, per_row)):
        got = smp.similarity(per_chain=True, first_slot=first, n_slots=S, max_workspace_bytes=budget)
        _same(got, full)
        assert smp.timing("similarity")[1] == chunks
    _same(smp.similarity(per_chain=True, first_slot=first, n_slots=S), full)
    # selected rows in chunks: the curve list travels with its chunk
    sel = [60, 3, 3, 17, 0, 44, 9]
    got = smp.similarity(curves=sel, per_chain=True, first_slot=first, n_slots=S, max_workspace_bytes=(per_row + 4) * 3)
    assert smp.timing("similarity")[1] == 3
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(full[k][sel]).tobytes(), k


def test_state_and_slots_untouched():
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=31, M=2, sigma_sq=0.01, seed=37, ragged=True)
    T, NCH = 10, 2
    states = _states(sim, NCH)
    pair = []
    for _ in range(2):
        smp = make_sampler_batch(sim, T, NCH)
        for q in range(NCH):
            smp.select_chain(q)
            smp.set_state(**states[q])
        smp.run(bf.SWEEP_WARM, 7, seed=3)
        pair.append(smp)
    a, b = pair

    def slots(smp):
        out = []
        for q in range(NCH):
            smp.select_chain(q)
            out.append({nm: smp.get_chain(nm) for nm in STATE})
        return out

    before = slots(a)
    a.similarity(per_chain=True, first_slot=1, n_slots=6)
    a.similarity(curves=[3, 1], first_slot=0, n_slots=7)
    after = slots(a)
    for q in range(NCH):
        for nm in STATE:
            assert before[q][nm].tobytes() == after[q][nm].tobytes(), (q, nm)
    for smp in pair:
        smp.run(bf.SWEEP_WARM, 3, first_iter=7, seed=3)
    sa, sb = slots(a), slots(b)
    for q in range(NCH):
        for nm in STATE:
            assert sa[q][nm].tobytes() == sb[q][nm].tobytes(), (q, nm)
    a.close()
    b.close()


def test_argument_checks(func):
    from bayesfmmm_amd import _lib
    smp = func["smp"]
    lib, n, T = smp.lib, smp.n, smp.T
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    mean, sd, cm = np.zeros(n * n), np.zeros(n * n), np.zeros(n * n * smp.n_chains)
    pm, ps, pc = (v.ctypes.data_as(dp) for v in (mean, sd, cm))

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    def idx(v):
        a = np.array(v, dtype=np.int32)
        return a, a.ctypes.data_as(ip)

    call = lib.bfmmm_chain_similarity
    msg = err(call(None, None, 0, 0, 8, 0, pm, ps, pc, n * n))
    assert "bfmmm_chain_similarity" in msg and "'h'" in msg
    assert "'mean'" in err(call(smp.h, None, 0, 0, 8, 0, None, ps, pc, n * n))
    keep, p = idx([0, n])
    assert re.search(rf"'curves'\[1\] = {n} outside 0 \.\. {n - 1}", err(call(smp.h, p, 2, 0, 8, 0, pm, ps, pc, n * n)))
    keep, p = idx([-1])
    assert "'curves'[0] = -1" in err(call(smp.h, p, 1, 0, 8, 0, pm, ps, pc, n * n))
    keep, p = idx([0])
    assert "'n_curves'" in err(call(smp.h, p, -1, 0, 8, 0, pm, ps, pc, n * n))
    assert "'first_slot'" in err(call(smp.h, None, 0, T, 1, 0, pm, ps, pc, n * n))
    assert "'first_slot'" in err(call(smp.h, None, 0, -1, 4, 0, pm, ps, pc, n * n))
    assert "'n_slots'" in err(call(smp.h, None, 0, 2, T - 1, 0, pm, ps, pc, n * n))
    assert "'n_slots'" in err(call(smp.h, None, 0, 0, 0, 0, pm, ps, pc, n * n))
    assert "'max_workspace_bytes' must not be negative" in err(call(smp.h, None, 0, 0, 8, -1, pm, ps, pc, n * n))
    assert f"'capacity' below {n * n} entries" in err(call(smp.h, None, 0, 0, 8, 0, pm, ps, pc, n * n - 1))
    keep, p = idx([5, 6, 7])
    assert f"'capacity' below {3 * n} entries" in err(call(smp.h, p, 3, 0, 8, 0, pm, ps, pc, 3 * n - 1))
    assert f"below the {8 * n} bytes of one row" in err(call(smp.h, None, 0, 0, 8, 8 * n - 1, pm, None, None, n * n))
    # the optional results are optional, and an empty selection is an empty result
    assert call(smp.h, None, 0, 0, 8, 0, pm, None, None, n * n) == 0
    assert call(smp.h, p, 0, 0, 8, 0, pm, None, None, 0) == 0
    for bad in ([0, n], [-1]):
        with pytest.raises(_lib.BfmmmError, match="'curves'"):
            smp.similarity(curves=bad)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        smp.similarity(first_slot=3, n_slots=T)


def test_draw_count_bound():
    """2^22 draws: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.similarity()
    smp.close()


def test_timing_is_reported(func):
    smp = func["smp"]
    smp.similarity(first_slot=func["first"], n_slots=func["S"])
    ms, launches = smp.timing("similarity")
    assert ms > 0.0 and launches == 1
