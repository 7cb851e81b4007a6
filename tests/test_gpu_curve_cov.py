"""Pooled per-curve covariance surfaces from chain slots on the device (kernels_curve_cov.hip): Sampler.curve_cov
against the numpy restatement (tests/curve_cov_ref.py) fed the get_chain copies, entry by entry within the derived bounds
|mean - ref| <= 2 (N + c_d) 2^-52 mean_t(A) (chain_mean: S for N) and |sd - ref| <= 4 N 2^-52 sd_ref + 2 c_d 2^-52 sqrt(N / (N - 1))
max_t A, c_d = 2 (P + K (1 + D)) + M + 3; edge tiles in both directions, one to four chained MFMAs with k of one and several
slices, covariates, the multivariate and tensor-product models, symmetry, transposition, the diagonal, row selection, chunking,
repeatability, one and two draws, untouched state, argument checks, timing."""
import ctypes as C
import re

import numpy as np
import pytest

import curve_cov_ref as R
from test_gpu_chain_batch import _states, make_sampler_batch
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

STATE = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "tau", "gamma", "Phi", "loglik"]
KEYS = ("mean", "sd", "chain_mean")


def _chains(smp, cov=False):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in ["Z", "Phi"] + (["xi"] if cov else [])})
    return out


def _rows_of_basis(smp, G):
    """G rows in the sampler's basis: the first observation rows of the curves' own bases"""
    return np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:G])


def _check(got, ref, N, label):
    """every entry of the device result within the bounds of the restatement; prints the worst ratio to the bound"""
    for k in KEYS:
        assert got[k].shape == ref[k].shape, (label, k, got[k].shape, ref[k].shape)
    assert np.all(np.isfinite(ref["mean"])) and np.abs(ref["mean"]).max() > 0, label
    worst = {}
    for key in ("mean", "chain_mean"):
        b = ref["bound_" + key]
        err = np.abs(got[key] - ref[key])
        assert np.all(b > 0), (label, key)
        worst[key] = float(np.max(err / b))
        print(f"{label} {key}: worst |device - numpy| / bound = {worst[key]:.3e}")
        assert np.all(err <= b), (label, key, worst[key])
    if N < 2:
        assert np.all(np.isnan(got["sd"])), label
    else:
        b = ref["bound_sd"]
        err = np.abs(got["sd"] - ref["sd"])
        worst["sd"] = float(np.max(err / b))
        print(f"{label} sd: worst |device - numpy| / bound = {worst['sd']:.3e}")
        assert np.all(err <= b), (label, "sd", worst["sd"])


def _same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def func():
    """n = 61 ragged, K = 3, M = 2, 4 chains, T = 30; slots 7 .. 29 are 92 draws.  The 17 x 17 surface of every curve, once."""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=33, ragged=True)
    T, NCH = 30, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(bf.SWEEP_WARM, T, seed=3)
    first, S = 7, T - 7
    E = _rows_of_basis(smp, 65)
    d = dict(smp=smp, chains=_chains(smp), first=first, S=S, E=E,
             full=smp.curve_cov(E[:17], per_chain=True, first_slot=first, n_slots=S))
    yield d
    smp.close()


@pytest.mark.parametrize("G1,G2", [(1, 1), (7, 33), (16, 16), (17, 65)])
def test_functional_matches_restatement(func, G1, G2):
    smp, E = func["smp"], func["E"]
    assert (smp.K, smp.M, smp.n_chains) == (3, 2, 4)
    E1 = E[:G1]
    E2 = None if G1 == G2 else np.ascontiguousarray(E[::-1][:G2])      # square: E2 = E1; otherwise another matrix
    got = smp.curve_cov(E1, E2, per_chain=True, first_slot=func["first"], n_slots=func["S"])
    assert got["mean"].shape == (61, G1, G2) and got["sd"].shape == (61, G1, G2) and got["chain_mean"].shape == (61, 4, G1, G2)
    ref = R.surfaces(func["chains"], E1, E2, func["first"], func["S"])
    _check(got, ref, 4 * func["S"], f"functional {G1} x {G2}")
    if E2 is None:
        assert np.all(np.einsum("igg->ig", got["mean"]) >= 0.0)      # variances


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("M", [1, 4, 5, 8, 9, 16])
def test_number_of_mfmas(K, M):
    """M of one to four chained MFMAs, padded and full, K of one and several k-slices"""
    import bayesfmmm_amd as bf
    from test_gpu_shapes import simulate
    n, degree, n_internal = 32, 3, 10          # P = 14: the largest at which K = 8 with M = 16 fits the sweep kernel's LDS
    sim = simulate(n, K, M, degree, n_internal, seed=300 + K * 20 + M)
    T, NCH, first = 12, 2, 2
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=degree, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 40 + K, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    assert smp.P == 14
    E = _rows_of_basis(smp, 17)
    got = smp.curve_cov(E, per_chain=True, first_slot=first)
    _check(got, R.surfaces(_chains(smp), E, None, first, T - first), NCH * (T - first), f"K={K} M={M}")
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(np.swapaxes(got[k], -1, -2)).tobytes(), k
    dg = smp.curve_cov(E, per_chain=True, diagonal=True, first_slot=first)
    assert dg["mean"].tobytes() == np.ascontiguousarray(np.einsum("igg->ig", got["mean"])).tobytes()
    smp.close()


@pytest.mark.parametrize("covariance_adj", [True, False])
def test_functional_with_covariates(covariance_adj):
    """covariance-adjusted: xi enters V; otherwise X does not enter (the restatement with D = 0)"""
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=60, M=2, sigma_sq=0.01, seed=34)
    X = np.random.default_rng(2).standard_normal((sim["n"], 2))
    T, NCH, first = 24, 3, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    smp.set_covariates(X, covariance_adj=covariance_adj)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(S.SWEEP_WARM | S.COV_MEAN | (S.COV_XI if covariance_adj else 0), T, seed=3)
    chains = _chains(smp, cov=True)
    E = _rows_of_basis(smp, 20)
    got = smp.curve_cov(E[:7], E[7:], per_chain=True, first_slot=first)
    ref = R.surfaces(chains, E[:7], E[7:], first, T - first, X=X, covariance_adj=covariance_adj)
    _check(got, ref, NCH * (T - first), f"functional D=2 cov_adj={covariance_adj}")
    if covariance_adj:      # xi is not negligible: without it the bound is missed
        no_xi = R.surfaces(chains, E[:7], E[7:], first, T - first)
        assert np.any(np.abs(got["mean"] - no_xi["mean"]) > no_xi["bound_mean"])
    smp.close()


@pytest.mark.parametrize("P,NCH", [(10, 4), (10, 1), (33, 2)])
def test_multivariate_identity_basis(P, NCH):
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, K, M, T = 70, 3, 2, 24
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    first = 6 if NCH > 1 else 0
    E = np.eye(P)
    got = smp.curve_cov(E, per_chain=True, first_slot=first)
    _check(got, R.surfaces(_chains(smp), E, None, first, T - first), NCH * (T - first), f"multivariate P={P}, {NCH} chains")
    smp.close()


def test_tensor_product_basis():
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    K, M, degs, n_int, n = 3, 2, [3, 3], [3, 3], 40          # 49 basis functions
    T, NCH, first = 12, 2, 2
    sim = simulate_tensor(n, K, M, degs, n_int, seed=311)
    assert sim["P"] == 49
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=max(degs), tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 5, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    E = np.ascontiguousarray(sim["B"][0][:20])                # rows of the first curve's own basis
    got = smp.curve_cov(E, per_chain=True, first_slot=first)
    _check(got, R.surfaces(_chains(smp), E, None, first, T - first), NCH * (T - first), "tensor basis P=49")
    smp.close()


def test_surface_is_symmetric_bit_for_bit(func):
    full = func["full"]
    assert full["mean"].shape == (61, 17, 17) and full["chain_mean"].shape == (61, 4, 17, 17)
    for k in KEYS:
        assert full[k].tobytes() == np.ascontiguousarray(np.swapaxes(full[k], -1, -2)).tobytes(), k
    # and over several column groups of tiles
    big = func["smp"].curve_cov(func["E"], curves=[0, 60, 31], per_chain=True, first_slot=func["first"], n_slots=func["S"])
    for k in KEYS:
        assert big[k].tobytes() == np.ascontiguousarray(np.swapaxes(big[k], -1, -2)).tobytes(), k
        assert np.ascontiguousarray(big[k][..., :17, :17]).tobytes() == np.ascontiguousarray(func["full"][k][[0, 60, 31]]).tobytes(), k


def test_transposition(func):
    smp, E, first, S = func["smp"], func["E"], func["first"], func["S"]
    E1, E2 = E[:17], np.ascontiguousarray(E[::-1][:33])
    a = smp.curve_cov(E1, E2, per_chain=True, first_slot=first, n_slots=S)
    b = smp.curve_cov(E2, E1, per_chain=True, first_slot=first, n_slots=S)
    ref = R.surfaces(func["chains"], E1, E2, first, S)
    bt = {k: np.ascontiguousarray(np.swapaxes(b[k], -1, -2)) for k in KEYS}
    _check(bt, ref, 4 * S, "transposed (E2, E1)")
    _check(a, ref, 4 * S, "(E1, E2)")


@pytest.mark.parametrize("curves", [None, [60, 3, 3, 17]])
def test_diagonal_equals_the_diagonal_of_the_surface(func, curves):
    smp, full = func["smp"], func["full"]
    got = smp.curve_cov(func["E"][:17], curves=curves, per_chain=True, diagonal=True, first_slot=func["first"], n_slots=func["S"])
    m = 61 if curves is None else len(curves)
    assert got["mean"].shape == (m, 17) and got["sd"].shape == (m, 17) and got["chain_mean"].shape == (m, 4, 17)
    rows = slice(None) if curves is None else curves
    for k, sub in (("mean", "igg->ig"), ("sd", "igg->ig"), ("chain_mean", "icgg->icg")):
        assert got[k].tobytes() == np.ascontiguousarray(np.einsum(sub, full[k][rows])).tobytes(), k
    assert np.all(got["mean"] > 0.0)


def test_row_selection_equals_rows_of_the_full_result(func):
    smp, full = func["smp"], func["full"]
    sel = [60, 3, 3, 17]
    got = smp.curve_cov(func["E"][:17], curves=sel, per_chain=True, first_slot=func["first"], n_slots=func["S"])
    assert got["mean"].shape == (4, 17, 17) and got["chain_mean"].shape == (4, 4, 17, 17)
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(full[k][sel]).tobytes(), k
    # the keys that were not asked for are absent
    a = smp.curve_cov(func["E"][:17], curves=sel, sd=False, first_slot=func["first"], n_slots=func["S"])
    assert set(a) == {"mean"}
    assert a["mean"].tobytes() == got["mean"].tobytes()
    b = smp.curve_cov(func["E"][:17], curves=sel, first_slot=func["first"], n_slots=func["S"])
    assert set(b) == {"mean", "sd"}
    _same(b, got, ("mean", "sd"))


def test_empty_selection(func):
    smp = func["smp"]
    got = smp.curve_cov(func["E"][:17], curves=[], per_chain=True, first_slot=func["first"], n_slots=func["S"])
    assert got["mean"].shape == (0, 17, 17) and got["sd"].shape == (0, 17, 17) and got["chain_mean"].shape == (0, 4, 17, 17)
    got = smp.curve_cov(func["E"][:17], curves=[], diagonal=True)
    assert got["mean"].shape == (0, 17)


def _budget_figures(smp, E, **kw):
    """(shared, per curve) bytes from the refusal of a budget of one byte"""
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'") as ei:
        smp.curve_cov(E, max_workspace_bytes=1, **kw)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    assert re.search(r"below the (\d+) bytes", str(ei.value)).group(1) == str(shared + per_curve)
    return shared, per_curve


def test_chunks_and_repeatability(func):
    smp, E, first, S, full = func["smp"], func["E"][:17], func["first"], func["S"], func["full"]
    kw = dict(per_chain=True, first_slot=first, n_slots=S)
    shared, per_curve = _budget_figures(smp, E, **kw)
    assert per_curve == 8 * 17 * 17 * (2 + 4)
    for chunks, rows in ((1, 61), (2, 31), (5, 13)):
        got = smp.curve_cov(E, max_workspace_bytes=shared + per_curve * rows, **kw)
        _same(got, full)
        assert smp.timing("curve_cov")[1] == chunks
    _same(smp.curve_cov(E, **kw), full)
    # selected rows in chunks
    sel = [60, 3, 3, 17, 0, 44, 9]
    sh2, pc2 = _budget_figures(smp, E, curves=sel, **kw)
    got = smp.curve_cov(E, curves=sel, max_workspace_bytes=sh2 + pc2 * 3, **kw)
    assert smp.timing("curve_cov")[1] == 3
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(full[k][sel]).tobytes(), k
    # the diagonal in chunks
    one = smp.curve_cov(E, diagonal=True, **kw)
    sh3, pc3 = _budget_figures(smp, E, diagonal=True, **kw)
    _same(smp.curve_cov(E, diagonal=True, max_workspace_bytes=sh3 + pc3 * 13, **kw), one)
    assert smp.timing("curve_cov")[1] == 5


def test_budget_below_one_curve_is_refused(func):
    from bayesfmmm_amd import _lib
    smp, E = func["smp"], func["E"][:17]
    kw = dict(per_chain=True, first_slot=func["first"], n_slots=func["S"])
    shared, per_curve = _budget_figures(smp, E, **kw)
    with pytest.raises(_lib.BfmmmError, match=rf"below the {shared + per_curve} bytes one curve needs") as ei:
        smp.curve_cov(E, max_workspace_bytes=shared + per_curve - 1, **kw)
    assert "bfmmm_chain_curve_cov" in str(ei.value)
    got = smp.curve_cov(E, max_workspace_bytes=shared + per_curve, **kw)      # one curve per chunk
    assert smp.timing("curve_cov")[1] == 61
    _same(got, func["full"])


def test_few_draws(func):
    import bayesfmmm_amd as bf
    smp, chains, E = func["smp"], func["chains"], func["E"][:17]
    # two slots of four chains, one slot of four chains
    for first, S in ((11, 2), (5, 1)):
        _check(smp.curve_cov(E, per_chain=True, first_slot=first, n_slots=S), R.surfaces(chains, E, None, first, S), 4 * S, f"slots {first}+{S}")
    # one draw and two draws in all: a single chain
    sim = simulate_functional(n=31, M=2, sigma_sq=0.01, seed=37, ragged=True)
    one = make_sampler_batch(sim, 6, 1)
    one.set_state(**_states(sim, 1)[0])
    one.run(bf.SWEEP_WARM, 6, seed=3)
    ch = _chains(one)
    E = _rows_of_basis(one, 17)
    got = one.curve_cov(E, per_chain=True, first_slot=4, n_slots=1)
    assert np.all(np.isnan(got["sd"])) and np.all(np.isfinite(got["mean"])) and np.all(np.isfinite(got["chain_mean"]))
    _check(got, R.surfaces(ch, E, None, 4, 1), 1, "one draw")
    assert got["chain_mean"][:, 0].tobytes() == got["mean"].tobytes()
    _check(one.curve_cov(E, per_chain=True, first_slot=3, n_slots=2), R.surfaces(ch, E, None, 3, 2), 2, "two draws")
    one.close()


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
    E = _rows_of_basis(a, 20)
    a.curve_cov(E, per_chain=True, first_slot=1, n_slots=6)
    a.curve_cov(E[:5], E[5:], curves=[3, 1], first_slot=0, n_slots=7)
    a.curve_cov(E, diagonal=True, first_slot=2, n_slots=3)
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
    lib, n, T, NC = smp.lib, smp.n, smp.T, smp.n_chains
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    G = 3
    E = np.ascontiguousarray(func["E"][:G])
    pe = E.ctypes.data_as(dp)
    cap = n * G * G
    mean, sd, cm = np.zeros(cap), np.zeros(cap), np.zeros(cap * NC)
    pm, ps, pc = (v.ctypes.data_as(dp) for v in (mean, sd, cm))

    def err(rc):
        assert rc != 0
        msg = lib.bfmmm_last_error().decode()
        assert msg.startswith("bfmmm_chain_curve_cov"), msg
        return msg

    def idx(v):
        a = np.array(v, dtype=np.int32)
        return a, a.ctypes.data_as(ip)

    call = lib.bfmmm_chain_curve_cov
    # (h, E1, G1, E2, G2, diagonal, curves, n_curves, first_slot, n_slots, max_workspace_bytes, mean, sd, chain_mean, capacity)
    assert "'h' is null" in err(call(None, pe, G, None, 0, 0, None, 0, 0, 8, 0, pm, ps, pc, cap))
    assert "'E1' is null" in err(call(smp.h, None, G, None, 0, 0, None, 0, 0, 8, 0, pm, ps, pc, cap))
    assert "'mean' is null" in err(call(smp.h, pe, G, None, 0, 0, None, 0, 0, 8, 0, None, ps, pc, cap))
    assert "'G1' must be at least 1" in err(call(smp.h, pe, 0, None, 0, 0, None, 0, 0, 8, 0, pm, ps, pc, cap))
    assert "'G2' must be at least 1" in err(call(smp.h, pe, G, pe, 0, 0, None, 0, 0, 8, 0, pm, ps, pc, cap))
    assert "'diagonal' requires 'E2' to be null" in err(call(smp.h, pe, G, pe, G, 1, None, 0, 0, 8, 0, pm, ps, pc, cap))
    keep, p = idx([0, n])
    assert re.search(rf"'curves'\[1\] = {n} outside 0 \.\. {n - 1}", err(call(smp.h, pe, G, None, 0, 0, p, 2, 0, 8, 0, pm, ps, pc, cap)))
    keep, p = idx([-1])
    assert "'curves'[0] = -1" in err(call(smp.h, pe, G, None, 0, 0, p, 1, 0, 8, 0, pm, ps, pc, cap))
    assert "'n_curves' must not be negative" in err(call(smp.h, pe, G, None, 0, 0, p, -1, 0, 8, 0, pm, ps, pc, cap))
    assert "'first_slot' out of range" in err(call(smp.h, pe, G, None, 0, 0, None, 0, T, 1, 0, pm, ps, pc, cap))
    assert "'first_slot' out of range" in err(call(smp.h, pe, G, None, 0, 0, None, 0, -1, 4, 0, pm, ps, pc, cap))
    assert "'n_slots' out of range" in err(call(smp.h, pe, G, None, 0, 0, None, 0, 2, T - 1, 0, pm, ps, pc, cap))
    assert "'n_slots' out of range" in err(call(smp.h, pe, G, None, 0, 0, None, 0, 0, 0, 0, pm, ps, pc, cap))
    assert "'max_workspace_bytes' must not be negative" in err(call(smp.h, pe, G, None, 0, 0, None, 0, 0, 8, -1, pm, ps, pc, cap))
    assert f"'capacity' below {cap} entries" in err(call(smp.h, pe, G, None, 0, 0, None, 0, 0, 8, 0, pm, ps, pc, cap - 1))
    assert f"'capacity' below {n * G} entries" in err(call(smp.h, pe, G, None, 0, 1, None, 0, 0, 8, 0, pm, ps, pc, n * G - 1))
    keep, p = idx([5, 6, 7])
    assert f"'capacity' below {3 * G * 2} entries" in err(call(smp.h, pe, G, pe, 2, 0, p, 3, 0, 8, 0, pm, ps, pc, 3 * G * 2 - 1))
    assert "bytes one curve needs" in err(call(smp.h, pe, G, None, 0, 0, None, 0, 0, 8, 64, pm, None, None, cap))
    # the optional results are optional; G2 is ignored where E2 is null; an empty selection is an empty result
    assert call(smp.h, pe, G, None, -5, 0, None, 0, 0, 8, 0, pm, None, None, cap) == 0
    assert call(smp.h, pe, G, None, 0, 1, None, 0, 0, 8, 0, pm, None, None, n * G) == 0
    assert call(smp.h, pe, G, None, 0, 0, p, 0, 0, 8, 0, pm, None, None, 0) == 0
    for bad in ([0, n], [-1]):
        with pytest.raises(_lib.BfmmmError, match="'curves'"):
            smp.curve_cov(E, curves=bad)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        smp.curve_cov(E, first_slot=3, n_slots=T)
    with pytest.raises(_lib.BfmmmError, match="'diagonal'"):
        smp.curve_cov(E, E, diagonal=True)
    with pytest.raises(_lib.BfmmmError, match="'G1'"):
        smp.curve_cov(E[:0])
    # the shape of E is checked before the library sees it
    with pytest.raises(ValueError):
        smp.curve_cov(np.zeros((3, smp.P + 1)))
    with pytest.raises(ValueError):
        smp.curve_cov(E, np.zeros((3, smp.P + 1)))


def test_draw_count_bound():
    """2^22 draws: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.curve_cov(np.eye(2))
    smp.close()


def test_timing_is_reported(func):
    smp = func["smp"]
    smp.curve_cov(func["E"][:17], first_slot=func["first"], n_slots=func["S"])
    ms, launches = smp.timing("curve_cov")
    assert ms > 0.0 and launches == 1
    ms, launches = smp.timing("curve_cov_project")
    assert ms > 0.0 and launches == 1
    smp.curve_cov(func["E"][:17], func["E"][17:40], curves=[1], first_slot=func["first"], n_slots=func["S"])
    assert smp.timing("curve_cov_project")[1] == 2 and smp.timing("curve_cov")[1] == 1
