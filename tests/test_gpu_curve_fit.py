"""Pooled per-curve fitted functions of chain slots and their credible bands on the device (kernels_curve_fit.hip; DESIGN.md
7e): Sampler.curve_fit against the numpy restatement (tests/curve_fit_ref.py) fed the get_chain copies, elementwise within the
restatement's derived forward error bound 2 N_t 2^-52 A; Sampler.curve_bands against numpy on the curve_fit values -- the
quantiles bit for bit, the mean within N 2^-52 mean|v|, the sd within relative 4 N 2^-52 of numpy's two-pass sd; both tiers
and their boundary, rows of one and two draws, curve selection, chunking, repeatability, untouched state, argument checks."""
import re

import numpy as np
import pytest

import curve_fit_ref as R
from test_gpu_chain_batch import _states, make_sampler_batch
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)
STATE = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "tau", "gamma", "Phi", "loglik"]


def _chains(smp, cov=False):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in ["nu", "Phi", "Z", "chi"] + (["eta", "xi"] if cov else [])})
    return out


def _check_values(smp, chains, E, which, first, S, X=None, covariance_adj=False, curves=None, label=""):
    got = smp.curve_fit(E, which=which, curves=curves, first_slot=first, n_slots=S)
    m = smp.n if curves is None else len(curves)
    assert got.shape == (m, E.shape[0], smp.n_chains, S)
    ref = R.values(chains, E, which, first, S, X, covariance_adj, curves)
    b = R.bound(chains, E, which, first, S, X, covariance_adj, curves)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() > 0, label
    err = np.abs(got - ref)
    ratio = np.max(err / np.where(b > 0, b, 1.0))
    print(f"{label} {which} G={E.shape[0]}: worst |device - numpy| / bound = {ratio:.3e}, |v| up to {np.abs(ref).max():.3e}")
    assert np.all(err <= b), (label, which, float(ratio), np.unravel_index(np.argmax(err - b), err.shape))
    return got


def _check_bands(smp, vals, E, which, first, S, probs=PROBS, curves=None, label="", **kw):
    """curve_bands against numpy on the curve_fit values `vals` (m, G, C, S)"""
    got = smp.curve_bands(E, which=which, probs=probs, curves=curves, first_slot=first, n_slots=S, **kw)
    m, G = vals.shape[:2]
    rows = vals.reshape(m, G, -1)
    N = rows.shape[-1]
    assert got["mean"].shape == (m, G) and got["sd"].shape == (m, G) and got["quantiles"].shape == (m, G, len(probs))
    assert np.array_equal(got["probs"], np.asarray(probs, dtype=np.float64))
    q = R.quantiles(rows, probs)
    assert got["quantiles"].tobytes() == q.tobytes(), (label, which, float(np.max(np.abs(got["quantiles"] - q))))
    mean, sd = R.moments(rows)
    tol = N * 2.0 ** -52 * np.mean(np.abs(rows), axis=-1)
    em = np.abs(got["mean"] - mean)
    print(f"{label} {which} N={N}: worst |mean - numpy| / (N 2^-52 mean|v|) = {np.max(em / tol):.3e}")
    assert np.all(em <= tol), (label, which)
    if N < 2:
        assert np.all(np.isnan(got["sd"])), (label, which)
    else:
        es = np.abs(got["sd"] - sd) / sd
        print(f"{label} {which} N={N}: worst relative |sd - numpy| / (4 N 2^-52) = {np.max(es) / (4 * N * 2.0 ** -52):.3e}")
        assert np.all(es <= 4 * N * 2.0 ** -52), (label, which)
    return got


def _rows_of_basis(smp, G):
    """G rows in the sampler's basis: the first observation rows of the curves' own bases"""
    return np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:G])


@pytest.fixture(scope="module")
def func():
    """n = 61 ragged, 4 chains, T = 30; rows from slot 7 on have 92 draws"""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=33, ragged=True)
    T, NCH = 30, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(bf.SWEEP_WARM, T, seed=3)
    d = dict(smp=smp, chains=_chains(smp), first=7, S=T - 7, E=_rows_of_basis(smp, 65), vals={})
    yield d
    smp.close()


def _func_vals(func, which):
    if which not in func["vals"]:
        func["vals"][which] = func["smp"].curve_fit(func["E"], which=which, first_slot=func["first"], n_slots=func["S"])
    return func["vals"][which]


@pytest.mark.parametrize("which", ["mean", "fit"])
@pytest.mark.parametrize("G", [1, 7, 65])
def test_functional_matches_restatement_and_bands_match_numpy(func, G, which):
    smp, E = func["smp"], func["E"][:G]
    vals = _check_values(smp, func["chains"], E, which, func["first"], func["S"], label="functional D=0")
    _check_bands(smp, vals, E, which, func["first"], func["S"], label="functional D=0")


@pytest.mark.parametrize("covariance_adj", [True, False])
def test_functional_with_covariates(covariance_adj):
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
    E = _rows_of_basis(smp, 7)
    for which in ("mean", "fit"):
        label = f"functional D=2 cov_adj={covariance_adj}"
        vals = _check_values(smp, chains, E, which, first, T - first, X=X, covariance_adj=covariance_adj, label=label)
        _check_bands(smp, vals, E, which, first, T - first, label=label)
    smp.close()


@pytest.mark.parametrize("P,NCH", [(10, 4), (10, 1), (33, 2)])
def test_multivariate_identity_basis(P, NCH):
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, K, M, T = 70, 3, 2, 24
    Y = rng.standard_normal((n, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    chains = _chains(smp)
    first = 6 if NCH > 1 else 0
    E = np.eye(P)
    for which in ("mean", "fit"):
        label = f"multivariate P={P}, {NCH} chains"
        vals = _check_values(smp, chains, E, which, first, T - first, label=label)
        _check_bands(smp, vals, E, which, first, T - first, label=label)
    if NCH == 1:
        # rows of one draw and of two draws
        for S in (1, 2):
            vals = _check_values(smp, chains, E, "fit", 5, S, label=f"rows of {S}")
            got = _check_bands(smp, vals, E, "fit", 5, S, probs=(0.0, 0.2, 0.5, 0.8, 1.0), label=f"rows of {S}")
            lo, hi = vals.reshape(n, P, S).min(axis=-1), vals.reshape(n, P, S).max(axis=-1)
            assert np.array_equal(got["quantiles"][..., 0], lo) and np.array_equal(got["quantiles"][..., 4], hi)
            if S == 1:
                assert np.all(np.isnan(got["sd"])) and np.array_equal(got["mean"], lo)
            else:
                assert np.all(np.isfinite(got["sd"]))
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
    chains = _chains(smp)
    E = np.ascontiguousarray(sim["B"][0])                    # the first curve's own basis rows
    for which in ("mean", "fit"):
        vals = _check_values(smp, chains, E, which, first, T - first, label="tensor basis P=49")
        _check_bands(smp, vals, E, which, first, T - first, label="tensor basis P=49")
    smp.close()


def _budget_for_chunks(smp, E, first, S, m, nchunks):
    """a max_workspace_bytes under which m curves take at least `nchunks` chunks, from the refusal's own figures"""
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'") as ei:
        smp.curve_bands(E, first_slot=first, n_slots=S, max_workspace_bytes=1)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    assert re.search(r"below the (\d+) bytes", str(ei.value)).group(1) == str(shared + per_curve)
    return shared + per_curve * (m // nchunks)


@pytest.mark.parametrize("NCH,T", [(4, 2048), (3, 2731)])
def test_tier_boundary(NCH, T):
    """rows of 8192 draws (the last sorted in LDS) and of 8193 (the first through the workspace)"""
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(8)
    n, P, K, M = 12, 6, 2, 2
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 23, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=23)
    assert NCH * T == (8192 if NCH == 4 else 8193)
    chains = _chains(smp)
    E = np.eye(P)[[0, 2, 5]]
    for which in ("mean", "fit"):
        vals = _check_values(smp, chains, E, which, 0, T, label=f"rows of {NCH * T}")
        one = _check_bands(smp, vals, E, which, 0, T, label=f"rows of {NCH * T}")
        few = smp.curve_bands(E, which=which, max_workspace_bytes=_budget_for_chunks(smp, E, 0, T, n, 3))
        for k in ("mean", "sd", "quantiles"):
            assert one[k].tobytes() == few[k].tobytes(), k
    smp.close()


def test_curve_selection(func):
    smp, E, first, S = func["smp"], func["E"][:7], func["first"], func["S"]
    sel = [5, 0, 60]
    for which in ("mean", "fit"):
        full = _func_vals(func, which)[:, :7]
        got = smp.curve_fit(E, which=which, curves=sel, first_slot=first, n_slots=S)
        assert got.tobytes() == np.ascontiguousarray(full[sel]).tobytes()
        fb = smp.curve_bands(E, which=which, first_slot=first, n_slots=S)
        sb = smp.curve_bands(E, which=which, curves=sel, first_slot=first, n_slots=S)
        for k in ("mean", "sd", "quantiles"):
            assert sb[k].tobytes() == np.ascontiguousarray(fb[k][sel]).tobytes(), k
    # the grid rows of a call do not depend on the other rows of E
    assert np.ascontiguousarray(_func_vals(func, "fit")[:, :7]).tobytes() == smp.curve_fit(E, first_slot=first, n_slots=S).tobytes()


def test_chunks_and_repeatability(func):
    smp, E, first, S = func["smp"], func["E"], func["first"], func["S"]
    budget = _budget_for_chunks(smp, E, first, S, smp.n, 3)
    for which in ("mean", "fit"):
        one = smp.curve_bands(E, which=which, first_slot=first, n_slots=S)
        few = smp.curve_bands(E, which=which, first_slot=first, n_slots=S, max_workspace_bytes=budget)
        again = smp.curve_bands(E, which=which, first_slot=first, n_slots=S)
        for k in ("mean", "sd", "quantiles"):
            assert one[k].tobytes() == few[k].tobytes(), k
            assert one[k].tobytes() == again[k].tobytes(), k
        assert _func_vals(func, which).tobytes() == smp.curve_fit(E, which=which, first_slot=first, n_slots=S).tobytes()
    # the same (curve, grid point, chain, slot) from another slot range
    part = smp.curve_fit(E, first_slot=first + 3, n_slots=10)
    assert part.tobytes() == np.ascontiguousarray(_func_vals(func, "fit")[..., 3:13]).tobytes()


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
    E = _rows_of_basis(a, 5)
    a.curve_fit(E, first_slot=1, n_slots=6)
    a.curve_bands(E, first_slot=1, n_slots=6)
    a.curve_bands(E, which="mean", first_slot=0, n_slots=7, curves=[3, 1])
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
    smp, E = func["smp"], func["E"][:3]
    T = smp.T
    for call in (smp.curve_fit, smp.curve_bands):
        with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
            call(E, first_slot=T)
        with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
            call(E, first_slot=-1, n_slots=4)
        with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
            call(E, first_slot=2, n_slots=T - 1)
        with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
            call(E, n_slots=0)
        with pytest.raises(_lib.BfmmmError, match="'which'"):
            call(E, which=2)
        with pytest.raises(_lib.BfmmmError, match="'G'"):
            call(E[:0])
        with pytest.raises(_lib.BfmmmError, match="'curves'"):
            call(E, curves=[0, smp.n])
        with pytest.raises(_lib.BfmmmError, match="'curves'"):
            call(E, curves=[-1])
        with pytest.raises(_lib.BfmmmError, match="'n_curves'"):
            call(E, curves=[])
    with pytest.raises(_lib.BfmmmError, match="'nq'"):
        smp.curve_bands(E, probs=())
    with pytest.raises(_lib.BfmmmError, match="'nq'"):
        smp.curve_bands(E, probs=np.linspace(0.0, 1.0, 17))
    with pytest.raises(_lib.BfmmmError, match="'probs'"):
        smp.curve_bands(E, probs=(0.5, 1.0000001))
    with pytest.raises(_lib.BfmmmError, match="'probs'"):
        smp.curve_bands(E, probs=(-1e-9,))
    with pytest.raises(_lib.BfmmmError, match="'probs'"):
        smp.curve_bands(E, probs=(np.nan,))
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'"):
        smp.curve_bands(E, max_workspace_bytes=-1)
    with pytest.raises(_lib.BfmmmError, match=r"'max_workspace_bytes' below the \d+ bytes"):
        smp.curve_bands(E, max_workspace_bytes=64)
    lib, n, C, G = smp.lib, smp.n, smp.n_chains, 3
    dp = _lib.c_double_p
    Ec = np.ascontiguousarray(E)
    pe = Ec.ctypes.data_as(dp)
    big = np.zeros(n * G * C * 8)
    pb = big.ctypes.data_as(dp)
    pr = np.array(PROBS)
    pp = pr.ctypes.data_as(dp)
    o = [np.zeros(n * G * 3) for _ in range(3)]
    po = [v.ctypes.data_as(dp) for v in o]

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    assert "'capacity'" in err(lib.bfmmm_chain_curve_fit(smp.h, 1, pe, G, None, 0, 0, 8, pb, big.size - 1))
    assert "'out'" in err(lib.bfmmm_chain_curve_fit(smp.h, 1, pe, G, None, 0, 0, 8, None, big.size))
    assert "'E'" in err(lib.bfmmm_chain_curve_fit(smp.h, 1, None, G, None, 0, 0, 8, pb, big.size))
    assert "'h'" in err(lib.bfmmm_chain_curve_fit(None, 1, pe, G, None, 0, 0, 8, pb, big.size))
    assert "'capacity'" in err(lib.bfmmm_chain_curve_bands(smp.h, 1, pe, G, None, 0, 0, 8, pp, 3, 0, *po, n * G - 1))
    assert "'E'" in err(lib.bfmmm_chain_curve_bands(smp.h, 1, None, G, None, 0, 0, 8, pp, 3, 0, *po, n * G))
    assert "'probs'" in err(lib.bfmmm_chain_curve_bands(smp.h, 1, pe, G, None, 0, 0, 8, None, 3, 0, *po, n * G))
    assert "'sd'" in err(lib.bfmmm_chain_curve_bands(smp.h, 1, pe, G, None, 0, 0, 8, pp, 3, 0, po[0], None, po[2], n * G))
    assert "'mean'" in err(lib.bfmmm_chain_curve_bands(smp.h, 1, pe, G, None, 0, 0, 8, pp, 3, 0, None, po[1], po[2], n * G))
    assert "'quantiles'" in err(lib.bfmmm_chain_curve_bands(smp.h, 1, pe, G, None, 0, 0, 8, pp, 3, 0, po[0], po[1], None, n * G))
    assert "'h'" in err(lib.bfmmm_chain_curve_bands(None, 1, pe, G, None, 0, 0, 8, pp, 3, 0, *po, n * G))
    # the shape of E is checked before the library sees it
    with pytest.raises(ValueError):
        smp.curve_fit(np.zeros((3, smp.P + 1)))
    with pytest.raises(ValueError):
        smp.curve_bands(E, which="median")


def test_draws_per_row_bound():
    """2^22 draws per row: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.curve_bands(np.eye(2))
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.curve_fit(np.eye(2), curves=[0])
    smp.close()
