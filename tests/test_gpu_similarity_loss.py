"""The least-squares draw of the clustering from chain slots on the device (k_similarity_loss, kernels_similarity.hip; DESIGN.md
7i): Sampler.similarity_loss against the numpy restatement (tests/similarity_loss_ref.py) fed the get_chain("Z") copies, every
entry within the derived bound |loss - ref| <= 2 [(n^2 + 2) u ref + 2 n delta sqrt(ref) + n^2 delta^2], delta = (2 N + 3 K + 7) u;
one block with edges, three block-rows at K of one and two MFMAs, the argmin and the draw it names, consistency with
Sampler.similarity's sd, one and two draws, label invariance, determinism and chunks, the diagnostics, get_slot, the multivariate
model, untouched state, argument checks and timing."""
import ctypes as C
import re

import numpy as np
import pytest

import similarity_loss_ref as R
from test_gpu_chain_batch import _states, make_sampler_batch
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

STATE = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "tau", "gamma", "Phi", "loglik"]
STATS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")


def _chains(smp):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append(smp.get_chain("Z"))
    smp.select_chain(0)
    return out


def _check(got, ref, n, K, label):
    """every entry of the device loss within the bound of the restatement; prints the worst ratio to the bound"""
    C_, S = ref.shape
    assert got.shape == ref.shape, label
    assert np.all(np.isfinite(ref)) and np.all(ref >= 0), label
    b = R.bound(ref, n, C_ * S, K)
    err = np.abs(got - ref)
    worst = float(np.max(err / b))
    print(f"{label} n={n} N={C_ * S} K={K}: worst |device - numpy| / bound {worst:.3e}, loss in [{ref.min():.3e}, {ref.max():.3e}]")
    assert np.all(err <= b), (label, worst)


@pytest.fixture(scope="module")
def func():
    """n = 61 ragged, K = 3, 4 chains, T = 30; slots 7 .. 29 are 92 draws: one block with edges.  Result and restatement, once."""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=33, ragged=True)
    T, NCH = 30, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=3)
    chains = _chains(smp)
    first, S = 7, T - 7
    ref = R.loss(chains, first, S)
    ref.setflags(write=False)
    d = dict(smp=smp, chains=chains, first=first, S=S, K=sim["K"], ref=ref, got=smp.similarity_loss(first_slot=first, n_slots=S))
    yield d
    smp.close()


def _k_sampler(K, M, degree, n_internal, n, T, NCH):
    import bayesfmmm_amd as bf
    from test_gpu_shapes import simulate
    sim = simulate(n, K, M, degree, n_internal, seed=100 + K * 10 + M)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=degree, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 40 + K, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    return smp


def test_one_block_with_edges_matches_restatement(func):
    got = func["got"]
    assert func["K"] == 3 and got["loss"].shape == (4, func["S"])
    _check(got["loss"], func["ref"], 61, 3, "functional, one block")
    assert set(got) == {"loss", "chain", "slot", "min"} | set(STATS)


@pytest.mark.parametrize("K,M,degree,n_internal", [
    (3, 2, 2, 5),      # one MFMA
    (5, 2, 3, 4),      # two MFMAs, the second padded
    (8, 2, 2, 5),      # two full MFMAs
])
def test_three_block_rows(K, M, degree, n_internal):
    """n = 130: blocks of 64 + 64 + 2 curves, six blocks of the upper triangle, a 2-wide edge; C = 2, S = 12"""
    n, T, NCH, first = 130, 14, 2, 2
    smp = _k_sampler(K, M, degree, n_internal, n, T, NCH)
    ref = R.loss(_chains(smp), first, T - first)
    got = smp.similarity_loss(first_slot=first)
    _check(got["loss"], ref, n, K, "three block-rows")
    assert smp.timing("similarity_loss")[1] == 1
    # one block per chunk and two: the same bytes; the launches the chunking implies
    N = NCH * (T - first)
    for per_chunk, chunks in ((1, 6), (2, 3), (4, 2)):
        again = smp.similarity_loss(first_slot=first, diagnostics=False, max_workspace_bytes=8 * N * (1 + per_chunk))
        assert again["loss"].tobytes() == got["loss"].tobytes(), per_chunk
        assert (again["chain"], again["slot"]) == (got["chain"], got["slot"])
        assert smp.timing("similarity_loss")[1] == chunks and smp.timing("similarity_loss_reduce")[1] == chunks
        assert smp.timing("similarity_loss")[0] > 0.0 and smp.timing("similarity_loss_reduce")[0] > 0.0
    smp.close()


def test_argmin_and_the_draw_it_names(func):
    smp, ref, got, first = func["smp"], func["ref"], func["got"], func["first"]
    apart, ratio = R.two_smallest_are_apart(ref, 61, 3)
    print(f"two smallest losses of the restatement: gap / sum of their bounds {ratio:.3e}")
    assert apart
    c, s = R.argmin(ref)
    assert (got["chain"], got["slot"]) == (c, first + s)
    assert got["min"] == got["loss"][got["chain"], got["slot"] - first]
    assert got["min"] == got["loss"].min()
    smp.select_chain(2)
    rep = smp.representative_draw(("Z", "nu"), first_slot=first, n_slots=func["S"])
    assert smp.get_chain("Z").tobytes() == func["chains"][2].tobytes()      # the selection is restored
    assert set(rep) == {"chain", "slot", "loss", "Z", "nu"}
    assert (rep["chain"], rep["slot"], rep["loss"]) == (got["chain"], got["slot"], got["min"])
    smp.select_chain(c)
    for nm in ("Z", "nu"):
        assert rep[nm].tobytes() == np.ascontiguousarray(smp.get_chain(nm)[..., first + s]).tobytes(), nm
    smp.select_chain(0)
    assert rep["Z"].shape == (61, 3)


def test_sum_of_losses_is_the_pooled_variance_of_similarity(func):
    """loss.sum() and (N - 1) (sd^2).sum() are the same non-negative terms in two orders"""
    smp, first, S = func["smp"], func["first"], func["S"]
    n, N = 61, 4 * S
    sd = smp.similarity(first_slot=first, n_slots=S)["sd"]
    a, b = float(func["got"]["loss"].sum()), float((N - 1) * (sd ** 2).sum())
    tol = 4.0 * (n * n + N + 2) * R.U
    print(f"sum of losses {a:.17g}, (N - 1) sum sd^2 {b:.17g}: relative difference {abs(a - b) / b:.3e} (tolerance {tol:.3e})")
    assert a >= 0.0 and b > 0.0
    assert abs(a - b) <= tol * b


def test_one_draw_and_two_draws():
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=31, M=2, sigma_sq=0.01, seed=37, ragged=True)
    one = make_sampler_batch(sim, 6, 1)
    one.set_state(**_states(sim, 1)[0])
    one.run(bf.SWEEP_WARM, 6, seed=3)
    got = one.similarity_loss(first_slot=4, n_slots=1)
    assert got["loss"].shape == (1, 1) and got["loss"][0, 0] == 0.0 and not np.signbit(got["loss"][0, 0])
    assert (got["chain"], got["slot"], got["min"]) == (0, 4, 0.0)
    for k in STATS:
        if k not in ("mean", "sd"):
            assert np.isnan(got[k]), k
    assert got["mean"] == 0.0
    Z = one.get_chain("Z")
    two = one.similarity_loss(first_slot=3, n_slots=2)
    ref = R.loss([Z], 3, 2)
    _check(two["loss"], ref, 31, 3, "two draws")
    assert ref.max() > 0.0
    assert abs(two["loss"][0, 0] - two["loss"][0, 1]) <= 8.0 * 31 * 31 * R.delta(2, 3)
    one.close()


def test_label_invariance():
    """a second batch whose chain states are the first's with the components permuted; the slots hold what was set"""
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=70, M=2, sigma_sq=0.01, seed=36, ragged=True)
    NCH, T = 3, 2
    states = _states(sim, NCH)
    perms = ([2, 0, 1], [1, 0, 2], [1, 2, 0])
    cvals = [8.0, 10.0, 12.0]
    a = make_sampler_batch(sim, T, NCH, c=cvals)
    b = make_sampler_batch(sim, T, NCH, c=cvals)
    for q in range(NCH):
        perm = perms[q]
        pst = dict(states[q])
        for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
            pst[nm] = np.asarray(states[q][nm])[perm]
        pst["Z"] = np.asarray(states[q]["Z"])[:, perm]
        a.select_chain(q)
        a.set_state(**states[q])
        b.select_chain(q)
        b.set_state(**pst)
    for smp in (a, b):
        smp.select_chain(0)
        smp.run(S.U_LOGLIK, T, seed=1)
    for q in range(NCH):
        a.select_chain(q)
        b.select_chain(q)
        np.testing.assert_array_equal(b.get_chain("Z"), a.get_chain("Z")[:, perms[q]])
        assert not np.array_equal(b.get_chain("Z"), a.get_chain("Z"))
    la, lb = a.similarity_loss()["loss"], b.similarity_loss()["loss"]
    ref = R.loss(_chains(a), 0, T)
    _check(la, ref, 70, 3, "labels as set")
    _check(lb, ref, 70, 3, "labels permuted")
    bd = R.bound(la, 70, NCH * T, 3)
    print(f"label permutation: worst |a - b| / bound {float(np.max(np.abs(la - lb) / bd)):.3e}")
    assert np.all(np.abs(la - lb) <= bd) and la.max() > 0.0
    a.close()
    b.close()


def test_determinism_and_budget(func):
    from bayesfmmm_amd import _lib
    smp, first, S, got = func["smp"], func["first"], func["S"], func["got"]
    again = smp.similarity_loss(first_slot=first, n_slots=S)
    assert again["loss"].tobytes() == got["loss"].tobytes()
    for k in STATS:
        assert np.float64(again[k]).tobytes() == np.float64(got[k]).tobytes(), k
    N = 4 * S
    with pytest.raises(_lib.BfmmmError, match=r"'max_workspace_bytes' below the (\d+) bytes one block needs") as ei:
        smp.similarity_loss(first_slot=first, n_slots=S, diagnostics=False, max_workspace_bytes=16 * N - 1)
    assert re.search(r"below the (\d+) bytes", str(ei.value)).group(1) == str(16 * N)
    exact = smp.similarity_loss(first_slot=first, n_slots=S, diagnostics=False, max_workspace_bytes=16 * N)
    assert exact["loss"].tobytes() == got["loss"].tobytes()


def test_diagnostics_equal_api_diagnostics_bitwise(func):
    from bayesfmmm_amd import api
    smp, first, S, got = func["smp"], func["first"], func["S"], func["got"]
    ref = api.diagnostics(got["loss"].T[:, :, None])      # (C, S) -> (S, C, 1)
    for k in STATS:
        assert isinstance(got[k], float)
        assert np.float64(got[k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes(), k
    assert np.isfinite(got["rhat"]) and got["ess_bulk"] > 0.0
    none = smp.similarity_loss(first_slot=first, n_slots=S, diagnostics=False)
    assert set(none) == {"loss", "chain", "slot", "min"}
    assert none["loss"].tobytes() == got["loss"].tobytes()


def test_get_slot_equals_the_get_chain_slice():
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    S = bf.sampler
    sim = simulate_functional(n=40, M=2, sigma_sq=0.01, seed=34)
    X = np.random.default_rng(2).standard_normal((sim["n"], 2))
    T, NCH = 9, 3
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    smp.set_covariates(X, covariance_adj=True)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(S.SWEEP_WARM | S.COV_MEAN | S.COV_XI, T, seed=3)
    names = STATE + ["eta", "xi", "tau_eta", "gamma_xi", "delta_xi", "A_xi"]
    full = []
    for q in range(NCH):
        smp.select_chain(q)
        full.append({nm: smp.get_chain(nm) for nm in names})
    for q in range(NCH):
        sel = (q + 1) % NCH
        smp.select_chain(sel)
        for slot in (0, 4, T - 1):
            for nm in names:
                want = full[q][nm][slot] if nm == "tau" else full[q][nm][..., slot]
                got = smp.get_slot(nm, slot, chain=q)
                assert got.shape == np.shape(want), (nm, got.shape)
                assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (q, slot, nm)
                # the selection is restored: without `chain` the chain selected before answers
                assert smp.get_slot("pi", slot).tobytes() == np.ascontiguousarray(full[sel]["pi"][..., slot]).tobytes(), (q, slot, nm)
    for bad in (-1, T):
        with pytest.raises(_lib.BfmmmError, match="bfmmm_get_slot: 'slot' out of range"):
            smp.get_slot("Z", bad)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_get_slot: unknown name 'nope'"):
        smp.get_slot("nope", 0)
    out = np.zeros(8)
    dp = _lib.c_double_p
    assert smp.lib.bfmmm_get_slot(smp.h, b"Z", 0, out.ctypes.data_as(dp), 8) != 0
    assert f"'capacity' below {40 * 3} entries" in smp.lib.bfmmm_last_error().decode()
    assert smp.lib.bfmmm_get_slot(None, b"Z", 0, out.ctypes.data_as(dp), 8) != 0 and "'h'" in smp.lib.bfmmm_last_error().decode()
    assert smp.lib.bfmmm_get_slot(smp.h, None, 0, out.ctypes.data_as(dp), 8) != 0 and "'name'" in smp.lib.bfmmm_last_error().decode()
    assert smp.lib.bfmmm_get_slot(smp.h, b"Z", 0, None, 8) != 0 and "'out'" in smp.lib.bfmmm_last_error().decode()
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
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    ref = R.loss(_chains(smp), first, T - first)
    got = smp.similarity_loss(first_slot=first)
    _check(got["loss"], ref, n, K, "multivariate")
    apart, ratio = R.two_smallest_are_apart(ref, n, K)
    print(f"two smallest losses of the restatement: gap / sum of their bounds {ratio:.3e}")
    assert apart
    c, s = R.argmin(ref)
    assert (got["chain"], got["slot"]) == (c, first + s)
    smp.close()


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
    a.similarity_loss(first_slot=1, n_slots=6)
    a.representative_draw(("Z", "nu", "Phi", "chi"), first_slot=0, n_slots=7)
    a.get_slot("tau", 3, chain=1)
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
    lib, T, NCH = smp.lib, smp.T, smp.n_chains
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    loss, stats = np.zeros(NCH * T), np.zeros(7)
    pl, ps = loss.ctypes.data_as(dp), stats.ctypes.data_as(dp)
    bc, bs = C.c_int32(), C.c_int32()

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    call = lib.bfmmm_chain_similarity_loss
    msg = err(call(None, 0, 8, 0, pl, NCH * 8, None, None, None))
    assert "bfmmm_chain_similarity_loss" in msg and "'h'" in msg
    assert "'loss'" in err(call(smp.h, 0, 8, 0, None, NCH * 8, None, None, None))
    assert "'first_slot'" in err(call(smp.h, T, 1, 0, pl, NCH * T, None, None, None))
    assert "'first_slot'" in err(call(smp.h, -1, 4, 0, pl, NCH * T, None, None, None))
    assert "'n_slots'" in err(call(smp.h, 2, T - 1, 0, pl, NCH * T, None, None, None))
    assert "'n_slots'" in err(call(smp.h, 0, 0, 0, pl, NCH * T, None, None, None))
    assert "'max_workspace_bytes' must not be negative" in err(call(smp.h, 0, 8, -1, pl, NCH * 8, None, None, None))
    assert f"'capacity' below {NCH * 8} entries" in err(call(smp.h, 0, 8, 0, pl, NCH * 8 - 1, None, None, None))
    assert f"'max_workspace_bytes' below the {16 * NCH * 8} bytes one block needs" in err(call(smp.h, 0, 8, 16 * NCH * 8 - 1, pl, NCH * 8, None, None, None))
    # the optional results are optional
    assert call(smp.h, 0, 8, 0, pl, NCH * 8, None, None, None) == 0
    assert call(smp.h, 0, 8, 0, pl, NCH * 8, C.byref(bc), C.byref(bs), ps) == 0
    assert 0 <= bc.value < NCH and 0 <= bs.value < 8 and loss[bc.value * 8 + bs.value] == loss[:NCH * 8].min()
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        smp.similarity_loss(first_slot=3, n_slots=T)


def test_draw_count_bound():
    """2^22 draws: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.similarity_loss()
    smp.close()


def test_timing_is_reported(func):
    smp = func["smp"]
    smp.similarity_loss(first_slot=func["first"], n_slots=func["S"])
    for nm in ("similarity_loss", "similarity_loss_reduce"):
        ms, launches = smp.timing(nm)
        assert ms > 0.0 and launches == 1, nm
