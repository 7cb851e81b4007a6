"""Simultaneous credible bands of the pooled per-curve fits on the device (k_fit_sim in kernels_curve_fit.hip):
Sampler.curve_bands_simultaneous.  mean and sd are Sampler.curve_bands' bit for bit in both tiers; crit, lower and upper are
the numpy restatement's (tests/curve_sim_ref.py) bit for bit when it is fed the device's curve_fit values and the device's mean
and sd -- the values are held to the get_chain restatement and the moments to numpy by tests/test_gpu_curve_fit.py, so this
pins what is new (deviations, maximum, sort, rule, band ends) with no tolerance.  One curve is cross-checked against the
single-table device implementation of the reference's rule (bfmmm_post_table_bands, compiled with contraction on): mid = mean
bit for bit, lower / upper within 4 2^-52 (|mean| + crit sd) (two roundings per side plus a possible fusion).  A planted
zero-variance grid point, curve selection, chunking, repeatability, the tier boundary, rows of one and two draws, the largest
G, untouched state, argument checks."""
import re

import numpy as np
import pytest

import curve_sim_ref as SR
from test_gpu_chain_batch import _states, make_sampler_batch
from test_gpu_curve_fit import STATE, _rows_of_basis
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

KEYS = ("mean", "sd", "crit", "lower", "upper")


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _table_bands(rows, alpha):
    """bfmmm_post_table_bands(simultaneous=1) on one curve's (G, N) rows: a T x ncol table, draw fastest"""
    from bayesfmmm_amd import api, _lib
    G, N = rows.shape
    V = np.ascontiguousarray(rows)
    up, mid, lo = np.zeros(G), np.zeros(G), np.zeros(G)
    dp = _lib.c_double_p
    rc = api._lib_entry().bfmmm_post_table_bands(V.ctypes.data_as(dp), N, G, float(alpha), 1, 0, up.ctypes.data_as(dp),
                                                 mid.ctypes.data_as(dp), lo.ctypes.data_as(dp))
    assert rc == 0
    return lo, mid, up


def _check(smp, E, which, first, S, alpha=0.05, curves=None, label="", cross=True, **kw):
    """checks 1 - 3 of one call; returns (result, values (m, G, N))"""
    got = smp.curve_bands_simultaneous(E, which=which, alpha=alpha, curves=curves, first_slot=first, n_slots=S, **kw)
    pw = smp.curve_bands(E, which=which, probs=(0.5,), curves=curves, first_slot=first, n_slots=S)
    vals = smp.curve_fit(E, which=which, curves=curves, first_slot=first, n_slots=S)
    m, G = vals.shape[:2]
    rows = vals.reshape(m, G, -1)
    N = rows.shape[-1]
    assert got["alpha"] == alpha and got["crit"].shape == (m,)
    for k in ("mean", "sd", "lower", "upper"):
        assert got[k].shape == (m, G), k
    assert _same(got["mean"], pw["mean"]), (label, which)
    ref = SR.sim_bands(rows, alpha, mean=got["mean"], sd=got["sd"])
    if N == 1:
        assert np.all(np.isnan(pw["sd"])) and np.all(np.isnan(got["sd"])), (label, which)
        for k in ("crit", "lower", "upper"):
            assert np.all(np.isnan(got[k])) and np.all(np.isnan(ref[k])), (label, which, k)
        return got, rows
    assert _same(got["sd"], pw["sd"]), (label, which, float(np.max(np.abs(got["sd"] - pw["sd"]) / pw["sd"])))
    for k in ("crit", "lower", "upper"):
        print(f"{label} {which} G={G} N={N} alpha={alpha}: max |device - restatement| of {k} = {np.max(np.abs(got[k] - ref[k])):.3e}")
        assert _same(got[k], ref[k]), (label, which, k)
    assert np.all(got["crit"] >= 0.0)
    if cross and np.all(got["sd"][0] != 0.0):
        lo, mid, up = _table_bands(rows[0], alpha)
        assert _same(mid, got["mean"][0]), (label, which)
        tol = 4 * 2.0 ** -52 * (np.abs(got["mean"][0]) + got["crit"][0] * got["sd"][0])
        el, eu = np.abs(lo - got["lower"][0]), np.abs(up - got["upper"][0])
        print(f"{label} {which} G={G} N={N}: table_bands, worst |difference| / tolerance: lower {np.max(el / tol):.3e}, upper {np.max(eu / tol):.3e}")
        assert np.all(el <= tol) and np.all(eu <= tol), (label, which)
    return got, rows


def _budget_for_chunks(smp, E, first, S, m, nchunks, **kw):
    """a max_workspace_bytes under which m curves take at least `nchunks` chunks, from the refusal's own figures; also checks
    that one byte below shared + one curve is refused with the byte count"""
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'") as ei:
        smp.curve_bands_simultaneous(E, first_slot=first, n_slots=S, max_workspace_bytes=1, **kw)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    assert re.search(r"below the (\d+) bytes", str(ei.value)).group(1) == str(shared + per_curve)
    with pytest.raises(_lib.BfmmmError, match=rf"'max_workspace_bytes' below the {shared + per_curve} bytes"):
        smp.curve_bands_simultaneous(E, first_slot=first, n_slots=S, max_workspace_bytes=shared + per_curve - 1, **kw)
    smp.curve_bands_simultaneous(E, first_slot=first, n_slots=S, max_workspace_bytes=shared + per_curve, **kw)
    return shared, per_curve, shared + per_curve * (m // nchunks)


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
    d = dict(smp=smp, first=7, S=T - 7, E=_rows_of_basis(smp, 65), full={})
    yield d
    smp.close()


def _full(func, which, G=7):
    """the full-budget result of all curves on the first G rows of E, computed once"""
    if (which, G) not in func["full"]:
        func["full"][which, G] = func["smp"].curve_bands_simultaneous(func["E"][:G], which=which, first_slot=func["first"],
                                                                      n_slots=func["S"])
    return func["full"][which, G]


@pytest.mark.parametrize("which", ["mean", "fit"])
@pytest.mark.parametrize("G", [1, 7, 65])
def test_functional(func, G, which):
    """G = 65: nine accumulator tiles, the last of one grid point"""
    alpha = {1: 0.5, 7: 0.05, 65: 0.1}[G]
    got, _ = _check(func["smp"], func["E"][:G], which, func["first"], func["S"], alpha=alpha, label="functional D=0")
    if G == 7:
        assert _same(got["crit"], _full(func, which)["crit"])


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
    E = _rows_of_basis(smp, 7)
    for which in ("mean", "fit"):
        _check(smp, E, which, first, T - first, label=f"functional D=2 cov_adj={covariance_adj}")
    smp.close()


@pytest.mark.parametrize("NCH", [4, 1])
def test_multivariate_identity_basis_and_short_rows(NCH):
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T = 70, 10, 3, 2, 24
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    first = 6 if NCH > 1 else 0
    for which in ("mean", "fit"):
        _check(smp, np.eye(P), which, first, T - first, label=f"multivariate P={P}, {NCH} chains")
    if NCH == 1:
        for S in (1, 2):
            for alpha in (0.05, 0.5, 0.9):
                got, rows = _check(smp, np.eye(P), "fit", 5, S, alpha=alpha, label=f"rows of {S}")
                if S == 1:
                    assert _same(got["mean"], rows[..., 0])
                else:
                    assert np.all(np.isfinite(got["lower"])) and np.all(got["lower"] <= got["upper"])
    smp.close()


@pytest.mark.parametrize("NCH,T", [(4, 2048), (3, 2731)])
def test_tier_boundary(NCH, T):
    """rows of 8192 draws (the last whose C is sorted in LDS) and of 8193 (the first through the workspace), 3 selected curves"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    rng = np.random.default_rng(8)
    n, P, K, M = 12, 6, 2, 2
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 23, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=23)
    N = NCH * T
    assert N == (8192 if NCH == 4 else 8193)
    E = np.eye(P)[[0, 2, 5]]
    sel = [7, 0, 11]
    for which in ("mean", "fit"):
        one, _ = _check(smp, E, which, 0, T, curves=sel, label=f"rows of {N}")
        assert smp.timing("curve_sim")[1] == (1 if N <= 8192 else 2) and smp.timing("curve_sim_reduce")[1] == (0 if N <= 8192 else 1)
        assert smp.timing("curve_sim")[0] > 0.0
        shared, per_curve, budget = _budget_for_chunks(smp, E, 0, T, n, 3, which=which)
        assert per_curve == 8 * (4 * 3 + 1) + (0 if N <= 8192 else 8 * (N + 16384))
        few = smp.curve_bands_simultaneous(E, which=which, max_workspace_bytes=budget)
        assert smp.timing("curve_sim")[1] >= (3 if N <= 8192 else 6)
        again = smp.curve_bands_simultaneous(E, which=which, curves=sel)
        for k in KEYS:
            assert _same(one[k], few[k][sel]), k
            assert _same(one[k], again[k]), k
    if NCH == 4:
        # the largest G: 64 KiB of mean and sd beside the 64 KiB sort row.  Repeated rows of E leave crit as it is.
        G = 4096
        Eb = np.ascontiguousarray(np.tile(E, (G // 3 + 1, 1))[:G])
        big = smp.curve_bands_simultaneous(Eb, which="mean", curves=[0], max_workspace_bytes=1 << 30)
        small = smp.curve_bands_simultaneous(E, which="mean", curves=[0])
        pw = smp.curve_bands(Eb, which="mean", probs=(0.5,), curves=[0], max_workspace_bytes=1 << 30)
        assert _same(big["crit"], small["crit"]) and _same(big["mean"], pw["mean"]) and _same(big["sd"], pw["sd"])
        for k in ("mean", "sd", "lower", "upper"):
            assert _same(big[k][0].reshape(-1)[:4095].reshape(-1, 3), np.tile(small[k][0], (1365, 1))), k
        with pytest.raises(_lib.BfmmmError, match="'G' above 4096"):
            smp.curve_bands_simultaneous(np.zeros((G + 1, P)), which="mean", curves=[0], max_workspace_bytes=1 << 30)
    smp.close()


@pytest.mark.parametrize("which", ["mean", "fit"])
def test_planted_zero_variance_grid_point(func, which):
    smp, first, S = func["smp"], func["first"], func["S"]
    base = _full(func, which)
    for pos in (7, 3):                 # appended, and in the middle of the first accumulator tile
        E = np.insert(func["E"][:7], pos, np.zeros(smp.P), axis=0)
        got = smp.curve_bands_simultaneous(E, which=which, first_slot=first, n_slots=S)
        keep = np.arange(8) != pos
        assert _same(got["crit"], base["crit"])
        for k in ("mean", "sd", "lower", "upper"):
            assert _same(got[k][:, keep], base[k]), k
            assert np.all(got[k][:, pos] == 0.0), k
    # every grid point without variance: crit is 0 and the band is the mean
    got = smp.curve_bands_simultaneous(np.zeros((3, smp.P)), which=which, first_slot=first, n_slots=S)
    assert np.all(got["crit"] == 0.0) and np.all(got["sd"] == 0.0) and np.all(got["lower"] == 0.0) and np.all(got["upper"] == 0.0)


def test_selection_chunks_and_repeatability(func):
    smp, E, first, S = func["smp"], func["E"][:7], func["first"], func["S"]
    sel = [5, 0, 5]
    for which in ("mean", "fit"):
        full = _full(func, which)
        got = smp.curve_bands_simultaneous(E, which=which, curves=sel, first_slot=first, n_slots=S)
        shared, per_curve, budget = _budget_for_chunks(smp, E, first, S, smp.n, 3, which=which)
        assert per_curve == 8 * (4 * 7 + 1)
        few = smp.curve_bands_simultaneous(E, which=which, first_slot=first, n_slots=S, max_workspace_bytes=budget)
        assert smp.timing("curve_sim")[1] >= 3 and smp.timing("curve_sim_reduce") == (0.0, 0)
        again = smp.curve_bands_simultaneous(E, which=which, first_slot=first, n_slots=S)
        for k in KEYS:
            assert _same(got[k], full[k][sel]), k
            assert _same(few[k], full[k]), k
            assert _same(again[k], full[k]), k
    # the grid points of a call do not depend on the other rows of E: a curve's crit does, its mean and sd do not
    wide = _full(func, "fit", 65)
    assert _same(wide["mean"][:, :7], _full(func, "fit")["mean"]) and _same(wide["sd"][:, :7], _full(func, "fit")["sd"])
    assert np.all(wide["crit"] >= _full(func, "fit")["crit"])


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
    a.curve_bands_simultaneous(E, first_slot=1, n_slots=6)
    a.curve_bands_simultaneous(E, which="mean", alpha=0.2, first_slot=0, n_slots=7, curves=[3, 1])
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
    call = smp.curve_bands_simultaneous
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
    for alpha in (0.0, 1.0, -0.1, 1.5, np.nan):
        with pytest.raises(_lib.BfmmmError, match="'alpha'"):
            call(E, alpha=alpha)
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' must not be negative"):
        call(E, max_workspace_bytes=-1)
    with pytest.raises(_lib.BfmmmError, match=r"'max_workspace_bytes' below the \d+ bytes"):
        call(E, max_workspace_bytes=64)
    lib, n, G = smp.lib, smp.n, 3
    dp = _lib.c_double_p
    Ec = np.ascontiguousarray(E)
    pe = Ec.ctypes.data_as(dp)
    o = [np.zeros(n * G) for _ in range(5)]
    po = [v.ctypes.data_as(dp) for v in o]

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    f = lib.bfmmm_chain_curve_bands_sim
    assert "'capacity'" in err(f(smp.h, 1, pe, G, None, 0, 0, 8, 0.05, 0, *po, n * G - 1))
    assert "'E'" in err(f(smp.h, 1, None, G, None, 0, 0, 8, 0.05, 0, *po, n * G))
    assert "'h'" in err(f(None, 1, pe, G, None, 0, 0, 8, 0.05, 0, *po, n * G))
    for j, nm in ((2, "'crit'"), (3, "'lower'"), (4, "'upper'")):
        args = list(po)
        args[j] = None
        assert nm in err(f(smp.h, 1, pe, G, None, 0, 0, 8, 0.05, 0, *args, n * G))
    # mean and sd may be null
    assert f(smp.h, 1, pe, G, None, 0, 0, 8, 0.05, 0, None, None, po[2], po[3], po[4], n * G) == 0
    full = call(E, first_slot=0, n_slots=8)
    assert _same(o[2][:n], full["crit"]) and _same(o[3], full["lower"]) and _same(o[4], full["upper"])
    # the shape of E and the name of `which` are checked before the library sees them
    with pytest.raises(ValueError):
        call(np.zeros((3, smp.P + 1)))
    with pytest.raises(ValueError):
        call(E, which="median")


def test_draws_per_row_bound():
    """2^22 draws per row: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.curve_bands_simultaneous(np.eye(2))
    smp.close()
