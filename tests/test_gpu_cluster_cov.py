"""Cluster covariance surfaces with bands from aligned chain slots on the device (kernels_cluster_cov.hip):
Sampler.cluster_cov_bands against the numpy restatement (tests/cluster_cov_ref.py) fed the get_chain copies.

The values (`trace`) are held entry by entry to the derived bound |device - restatement| <= b = c_v 2^-52 A, c_v = 2 (P + D + 1) +
M + 3.  The reductions are held to the returned trace itself: the quantiles are bfmmm_post_col_quantiles of its rows byte for
byte; mean and sd, for which no public entry runs k_bands_moments on a host table, to tests/test_gpu_align.py's bounds over equal
values (N 2^-52 mean|v|, relative 4 N 2^-52); crit, lower and upper are tests/curve_sim_ref.py's rule per pair on the trace with
the device's own mean and sd, byte for byte.  Then what the layout promises bit for bit (symmetry, transposition, the diagonal,
pair selection, chunking, repeatability), one and two draws, the empty pair list, untouched state, refusals and timers.  A row
above 8192 draws: tests/test_gpu_long_rows.py."""
import ctypes as C
import re

import numpy as np
import pytest

import cluster_cov_ref as R
import curve_fit_ref as FR
from simdata import simulate_functional
from test_gpu_chain_batch import _states, make_sampler_batch
from test_gpu_curve_cov import _chains, _rows_of_basis, func      # noqa: F401 (func: the module fixture, one sampler per module)

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
STATE = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "tau", "gamma", "Phi", "loglik"]
ALL = ("mean", "sd", "quantiles", "crit", "lower", "upper", "trace")
IP = C.POINTER(C.c_int32)


def _random_perm(smp, S, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.permutation(smp.K) for _ in range(S)]) for _ in range(smp.n_chains)]).astype(np.int32)


def _check_trace(got, chains, perm, E1, E2, first, S, label, pairs=None, x=None, diagonal=False):
    """every entry of the device's values within b of the restatement; prints the worst ratio"""
    ref = R.values(chains, perm, E1, E2, first, S, pairs, x, diagonal)
    b = R.bound(chains, perm, E1, E2, first, S, pairs, x, diagonal)
    assert got["trace"].shape == ref.shape, (label, got["trace"].shape, ref.shape)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() > 0 and np.all((b > 0) | (ref == 0.0)), label      # b = 0: a row of zeros in E
    err = np.abs(got["trace"] - ref)
    worst = float(np.max(err[b > 0] / b[b > 0]))
    print(f"{label}: {ref.size} values, worst |device - numpy| / b = {worst:.3e}")
    assert np.all(err <= b), (label, worst)
    return ref, b


def _same(a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _col_quantiles(rows, probs):
    """bfmmm_post_col_quantiles of the table rows (L, N)"""
    from bayesfmmm_amd import api
    V = np.ascontiguousarray(rows, dtype=np.float64)
    L, N = V.shape
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    q = np.zeros((L, pr.size))
    api._check(api._lib_entry().bfmmm_post_col_quantiles(V.ctypes.data_as(api.c_double_p), N, L, pr.ctypes.data_as(api.c_double_p), pr.size, 0,
                                                         q.ctypes.data_as(api.c_double_p)))
    return q


def _check_reductions(got, alpha, label):
    """quantiles, crit, lower and upper byte for byte from the returned trace; mean and sd within the bounds over equal values"""
    tr = got["trace"]
    N = tr.shape[-1]
    cell = tr.shape[:-1]
    q = _col_quantiles(tr.reshape(-1, N), got["probs"])
    assert got["quantiles"].shape == cell + (len(got["probs"]),)
    assert got["quantiles"].tobytes() == q.tobytes(), label
    mean, sd = FR.moments(tr)
    em, tm = np.abs(got["mean"] - mean), N * U * np.mean(np.abs(tr), axis=-1)
    assert np.all(em <= tm), (label, "mean")
    if N > 1:
        es, ts = np.abs(got["sd"] - sd), 4 * N * U * sd
        assert np.all(es <= ts), (label, "sd")
        pos = ts > 0
        print(f"{label}: worst |mean - numpy| / bound {float(np.max(em[tm > 0] / tm[tm > 0])):.3e}, "
              f"|sd - numpy| / bound {float(np.max(es[pos] / ts[pos])):.3e}")
    else:
        assert np.all(np.isnan(got["sd"])), label
    if alpha is not None:
        s = R.sim_bands(tr, alpha, got["mean"], got["sd"])
        assert got["crit"].shape == (tr.shape[0],) and got["lower"].shape == cell and got["upper"].shape == cell
        for k in ("crit", "lower", "upper"):
            assert got[k].tobytes() == np.ascontiguousarray(s[k]).tobytes(), (label, k)


# ---- the values against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("G1,G2", [(1, 1), (7, 33), (16, 16), (17, 65)])
def test_trace_matches_restatement(func, G1, G2, aligned):
    smp, E, first, S = func["smp"], func["E"], func["first"], func["S"]
    assert (smp.K, smp.M, smp.n_chains, S) == (3, 2, 4, 23)
    perm = smp.align(first_slot=first, n_slots=S)["perm"] if aligned else _random_perm(smp, S, 100 + G1)
    E1 = E[:G1]
    E2 = None if G1 == G2 else np.ascontiguousarray(E[::-1][:G2])      # square: E2 = E1; otherwise another matrix
    for pairs in (None, [(2, 0), (1, 1), (2, 0)]):
        got = smp.cluster_cov_bands(E1, perm, E2, pairs=pairs, trace=True, first_slot=first, n_slots=S)
        m = 6 if pairs is None else 3
        assert got["mean"].shape == (m, G1, G2) and got["sd"].shape == (m, G1, G2) and got["quantiles"].shape == (m, G1, G2, 3)
        assert got["trace"].shape == (m, G1, G2, 92) and got["pairs"].shape == (m, 2)
        assert got["pairs"].tolist() == [list(p) for p in (R.all_pairs(3) if pairs is None else pairs)]
        _check_trace(got, func["chains"], perm, E1, E2, first, S, f"{G1} x {G2} aligned={aligned} pairs={pairs}", pairs=pairs)
        _check_reductions(got, None, f"{G1} x {G2}")


# ---- the reductions from the trace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diagonal", [False, True])
def test_reductions_byte_for_byte_from_the_trace(func, diagonal):
    smp, first, S = func["smp"], func["first"], func["S"]
    perm = smp.align(first_slot=first, n_slots=S)["perm"]
    E1 = func["E"][:7].copy()
    E1[3] = 0.0                                  # a row of zeros: values, and so sd, exactly 0 on it
    E2 = None if diagonal else np.ascontiguousarray(func["E"][20:29])
    alpha = 0.1
    got = smp.cluster_cov_bands(E1, perm, E2, diagonal=diagonal, probs=(0.0, 0.05, 0.5, 0.9, 1.0), simultaneous=alpha, trace=True,
                                first_slot=first, n_slots=S)
    assert got["alpha"] == alpha and got["trace"].shape == ((6, 7, 92) if diagonal else (6, 7, 9, 92))
    assert np.all(got["sd"][:, 3] == 0.0) and np.all(got["mean"][:, 3] == 0.0) and np.count_nonzero(got["sd"] == 0.0) == got["sd"][:, 3].size
    assert np.all(got["lower"][:, 3] == 0.0) and np.all(got["upper"][:, 3] == 0.0)
    assert np.all(np.isfinite(got["crit"])) and np.all(got["crit"] > 0.0)
    _check_trace(got, func["chains"], perm, E1, E2, first, S, f"zero row, diagonal={diagonal}", diagonal=diagonal)
    _check_reductions(got, alpha, f"reductions, diagonal={diagonal}")
    # the band holds whole surfaces: the share of draws inside it everywhere is at least 1 - alpha
    inside = np.all((got["trace"] >= got["lower"][..., None]) & (got["trace"] <= got["upper"][..., None]), axis=tuple(range(1, got["trace"].ndim - 1)))
    assert np.all(inside.mean(axis=-1) >= 1.0 - alpha - 1.0 / 92)


# ---- one to four chained MFMAs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("M", [1, 4, 5, 16])
def test_number_of_mfmas(K, M):
    """M of one to four chained MFMAs, padded and full; pairs in any order and a random permutation row per draw"""
    import bayesfmmm_amd as bf
    from test_gpu_shapes import simulate
    n, degree, n_internal = 32, 3, 10          # P = 14
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
    S = T - first
    perm = _random_perm(smp, S, K * 100 + M)
    pairs = [(K - 1, 0), (0, K - 1), (K - 1, K - 1), (0, 0), (K // 2, 1)]
    chains = _chains(smp)
    got = smp.cluster_cov_bands(E, perm, pairs=pairs, simultaneous=0.05, trace=True, first_slot=first)
    _check_trace(got, chains, perm, E, None, first, S, f"K={K} M={M}", pairs=pairs)
    _check_reductions(got, 0.05, f"K={K} M={M}")
    for k in ("mean", "sd", "quantiles", "trace"):
        assert got[k][0].tobytes() == np.ascontiguousarray(np.swapaxes(got[k][1], 0, 1)).tobytes(), k      # (l, k) is (k, l) transposed
        assert got[k][2].tobytes() == np.ascontiguousarray(np.swapaxes(got[k][2], 0, 1)).tobytes(), k      # (k, k) is symmetric
    dg = smp.cluster_cov_bands(E, perm, pairs=pairs, diagonal=True, trace=True, first_slot=first)
    assert dg["trace"].tobytes() == np.ascontiguousarray(np.einsum("rggs->rgs", got["trace"])).tobytes()
    if K == 8:          # all 36 pairs
        _check_trace(smp.cluster_cov_bands(E[:3], perm, E[3:8], trace=True, first_slot=first), chains, perm, E[:3], E[3:8], first, S, f"K={K} M={M}, all pairs")
    smp.close()


# ---- covariates -------------------------------------------------------------------------------------------------------------
def _cov_sampler(covariance_adj):
    import bayesfmmm_amd as bf
    Sm = bf.sampler
    sim = simulate_functional(n=60, M=2, sigma_sq=0.01, seed=34)
    X = np.random.default_rng(2).standard_normal((sim["n"], 2))
    T, NCH = 24, 3
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    smp.set_covariates(X, covariance_adj=covariance_adj)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(Sm.SWEEP_WARM | Sm.COV_MEAN | (Sm.COV_XI if covariance_adj else 0), T, seed=3)
    return smp, T


def test_covariate_setting():
    smp, T = _cov_sampler(True)
    first, S = 4, T - 4
    chains = _chains(smp, cov=True)
    E = _rows_of_basis(smp, 20)
    perm = smp.align(first_slot=first)["perm"]
    x = np.array([0.7, -1.3])
    got = smp.cluster_cov_bands(E[:7], perm, E[7:], x=x, simultaneous=0.05, trace=True, first_slot=first)
    _, b = _check_trace(got, chains, perm, E[:7], E[7:], first, S, "covariance-adjusted, x = (0.7, -1.3)", x=x)
    _check_reductions(got, 0.05, "covariance-adjusted")
    # without x: phi alone, and xi is not negligible
    none = smp.cluster_cov_bands(E[:7], perm, E[7:], trace=True, first_slot=first)
    _, b0 = _check_trace(none, chains, perm, E[:7], E[7:], first, S, "covariance-adjusted, no x")
    assert np.any(np.abs(got["trace"] - none["trace"]) > b + b0)
    # x = 0 is phi alone too, to within the bound (the products with xi are exact zeros)
    zero = smp.cluster_cov_bands(E[:7], perm, E[7:], x=np.zeros(2), trace=True, first_slot=first)
    assert zero["trace"].tobytes() == none["trace"].tobytes()
    with pytest.raises(ValueError):
        smp.cluster_cov_bands(E[:7], perm, x=[1.0], first_slot=first)
    smp.close()


def test_covariate_setting_needs_a_covariance_adjusted_sampler():
    from bayesfmmm_amd import _lib
    smp, T = _cov_sampler(False)
    perm = np.tile(np.arange(smp.K, dtype=np.int32), (smp.n_chains, T - 4, 1))
    E = _rows_of_basis(smp, 5)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_cluster_cov_bands: 'x' is given but the sampler is not covariance-adjusted"):
        smp.cluster_cov_bands(E, perm, x=[0.7, -1.3], first_slot=4)
    got = smp.cluster_cov_bands(E, perm, trace=True, first_slot=4)          # without x it is served: phi alone
    _check_trace(got, _chains(smp), perm, E, None, 4, T - 4, "covariates without adjustment, no x")
    smp.close()


# ---- bit properties ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(func):
    """all six pairs on the 17 x 17 grid with every output, once"""
    smp, first, S = func["smp"], func["first"], func["S"]
    perm = smp.align(first_slot=first, n_slots=S)["perm"]
    E = np.ascontiguousarray(func["E"][:17])
    kw = dict(simultaneous=0.05, trace=True, first_slot=first, n_slots=S)
    return dict(perm=perm, E=E, kw=kw, out=smp.cluster_cov_bands(E, perm, **kw))


def test_symmetry_and_transposition(func, full):
    smp, out = func["smp"], full["out"]
    assert out["pairs"].tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]
    for r in (0, 3, 5):          # k = l: a symmetric surface
        for k in ("mean", "sd", "quantiles", "lower", "upper", "trace"):
            assert out[k][r].tobytes() == np.ascontiguousarray(np.swapaxes(out[k][r], 0, 1)).tobytes(), (r, k)
        assert np.all(np.einsum("gg->g", out["mean"][r]) > 0.0)      # variances
    sw = smp.cluster_cov_bands(full["E"], full["perm"], pairs=[(1, 0), (2, 0), (2, 1)], **full["kw"])
    for j, r in enumerate((1, 2, 4)):
        for k in ("mean", "sd", "quantiles", "lower", "upper", "trace"):
            assert sw[k][j].tobytes() == np.ascontiguousarray(np.swapaxes(out[k][r], 0, 1)).tobytes(), (r, k)
        assert sw["crit"][j] == out["crit"][r]
    # two bases: (k, l, E1, E2) -> (l, k, E2, E1)
    Ea, Eb = full["E"], np.ascontiguousarray(func["E"][30:63])
    a = smp.cluster_cov_bands(Ea, full["perm"], Eb, pairs=[(0, 2), (1, 1)], **full["kw"])
    b = smp.cluster_cov_bands(Eb, full["perm"], Ea, pairs=[(2, 0), (1, 1)], **full["kw"])
    for k in ("mean", "sd", "quantiles", "lower", "upper", "trace"):
        assert a[k].tobytes() == np.ascontiguousarray(np.swapaxes(b[k], 1, 2)).tobytes(), k
    assert a["crit"].tobytes() == b["crit"].tobytes()


def test_diagonal_equals_the_diagonal_of_the_surface(func, full):
    smp, out = func["smp"], full["out"]
    for pairs, rows in ((None, slice(None)), ([(1, 2), (0, 0)], [4, 0])):
        dg = smp.cluster_cov_bands(full["E"], full["perm"], pairs=pairs, diagonal=True, **full["kw"])
        m = 6 if pairs is None else 2
        assert dg["mean"].shape == (m, 17) and dg["quantiles"].shape == (m, 17, 3) and dg["trace"].shape == (m, 17, 92)
        assert dg["lower"].shape == (m, 17) and dg["crit"].shape == (m,)
        for k, sub in (("mean", "rgg->rg"), ("sd", "rgg->rg"), ("quantiles", "rggq->rgq"), ("trace", "rggs->rgs")):
            assert dg[k].tobytes() == np.ascontiguousarray(np.einsum(sub, out[k][rows])).tobytes(), k
        _check_reductions(dg, 0.05, "diagonal")      # its band is over the diagonal's entries alone


def test_pair_selection_equals_rows_of_the_full_result(func, full):
    smp, out = func["smp"], full["out"]
    got = smp.cluster_cov_bands(full["E"], full["perm"], pairs=[(1, 2), (0, 0), (1, 2)], **full["kw"])
    for k in ALL:
        assert got[k].tobytes() == np.ascontiguousarray(out[k][[4, 0, 4]]).tobytes(), k
    # the keys that were not asked for are absent; what is there does not depend on them
    a = smp.cluster_cov_bands(full["E"], full["perm"], pairs=[(1, 2)], probs=(), first_slot=func["first"], n_slots=func["S"])
    assert set(a) == {"mean", "sd", "quantiles", "probs", "pairs"} and a["quantiles"].shape == (1, 17, 17, 0)
    _same(a, {k: np.ascontiguousarray(out[k][[4]]) for k in ("mean", "sd")}, ("mean", "sd"))


def _budget_figures(smp, E, perm, **kw):
    """(shared, per row) bytes from the refusal of a budget of one byte"""
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'") as ei:
        smp.cluster_cov_bands(E, perm, max_workspace_bytes=1, **kw)
    msg = str(ei.value)
    shared, per_row = (int(v) for v in re.search(r"\((\d+) shared by all rows \+ (\d+) per row\)", msg).groups())
    assert msg.startswith("bfmmm_chain_cluster_cov_bands") and re.search(r"below the (\d+) bytes one row needs", msg).group(1) == str(shared + per_row)
    return shared, per_row


def test_chunks_and_repeatability(func, full):
    from bayesfmmm_amd import _lib
    smp, perm, kw = func["smp"], full["perm"], full["kw"]
    E = np.ascontiguousarray(func["E"][:5])
    one = smp.cluster_cov_bands(E, perm, **kw)                         # 6 x 5 x 5 = 150 rows in one chunk
    assert smp.timing("cluster_cov")[1] == 1 and smp.timing("cluster_cov_maxdev")[1] == 1
    _same(smp.cluster_cov_bands(E, perm, **kw), one, ALL)
    _same(one, {k: np.ascontiguousarray(full["out"][k][:, :5, :5]) for k in ("mean", "sd", "quantiles", "trace")}, ("mean", "sd", "quantiles", "trace"))
    shared, per_row = _budget_figures(smp, E, perm, **kw)
    assert per_row == 8 * (92 + 2 + 3)
    for rows, chunks in ((75, 2), (50, 3), (49, 4), (7, 22), (1, 150)):
        got = smp.cluster_cov_bands(E, perm, max_workspace_bytes=shared + per_row * rows + 7, **kw)
        _same(got, one, ALL)
        # the band takes a second sweep over the chunks
        assert smp.timing("cluster_cov")[1] == 2 * chunks and smp.timing("cluster_cov_maxdev")[1] == chunks
    with pytest.raises(_lib.BfmmmError, match=rf"below the {shared + per_row} bytes one row needs"):
        smp.cluster_cov_bands(E, perm, max_workspace_bytes=shared + per_row - 1, **kw)
    # without the band: one sweep, a smaller share, the same pointwise results
    kw2 = dict(kw, simultaneous=None)
    sh2, pr2 = _budget_figures(smp, E, perm, **kw2)
    assert pr2 == per_row and shared - sh2 == 8 * (6 * 92 + 6)
    got = smp.cluster_cov_bands(E, perm, max_workspace_bytes=sh2 + pr2 * 50, **kw2)
    _same(got, one, ("mean", "sd", "quantiles", "trace"))
    assert smp.timing("cluster_cov")[1] == 3 and smp.timing("cluster_cov_maxdev") == (0.0, 0)
    # the diagonal and two bases in chunks
    for extra in (dict(diagonal=True), dict(E2=np.ascontiguousarray(func["E"][40:47]), pairs=[(2, 1), (0, 0), (1, 2)])):
        ref = smp.cluster_cov_bands(E, perm, **kw, **extra)
        sh3, pr3 = _budget_figures(smp, E, perm, **kw, **extra)
        _same(smp.cluster_cov_bands(E, perm, max_workspace_bytes=sh3 + pr3 * 4, **kw, **extra), ref, ALL)


def test_multivariate_identity_basis():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T, NCH, first = 70, 10, 3, 2, 24, 4, 6
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    perm = smp.align(first_slot=first)["perm"]
    E = np.eye(P)
    got = smp.cluster_cov_bands(E, perm, simultaneous=0.05, trace=True, first_slot=first)
    _check_trace(got, _chains(smp), perm, E, None, first, T - first, "multivariate P=10")
    _check_reductions(got, 0.05, "multivariate P=10")
    smp.close()


# ---- edges ------------------------------------------------------------------------------------------------------------------
def test_one_and_two_draws(func):
    import bayesfmmm_amd as bf
    smp, chains, E = func["smp"], func["chains"], np.ascontiguousarray(func["E"][:17])
    # two slots and one slot of four chains
    for first, S in ((11, 2), (5, 1)):
        perm = _random_perm(smp, S, first)
        got = smp.cluster_cov_bands(E, perm, simultaneous=0.05, trace=True, first_slot=first, n_slots=S)
        _check_trace(got, chains, perm, E, None, first, S, f"slots {first}+{S}")
        _check_reductions(got, 0.05, f"slots {first}+{S}")
    # one draw and two draws in all: a single chain
    sim = simulate_functional(n=31, M=2, sigma_sq=0.01, seed=37, ragged=True)
    one = make_sampler_batch(sim, 6, 1)
    one.set_state(**_states(sim, 1)[0])
    one.run(bf.SWEEP_WARM, 6, seed=3)
    ch = _chains(one)
    E = _rows_of_basis(one, 17)
    perm = _random_perm(one, 1, 1)
    got = one.cluster_cov_bands(E, perm, simultaneous=0.05, trace=True, first_slot=4, n_slots=1)
    assert np.all(np.isnan(got["sd"])) and np.all(np.isfinite(got["mean"]))
    assert np.all(np.isnan(got["crit"])) and np.all(np.isnan(got["lower"])) and np.all(np.isnan(got["upper"]))
    _check_trace(got, ch, perm, E, None, 4, 1, "one draw")
    assert got["mean"].tobytes() == np.ascontiguousarray(got["trace"][..., 0]).tobytes()
    for q in range(3):
        assert got["quantiles"][..., q].tobytes() == got["mean"].tobytes()
    perm = _random_perm(one, 2, 2)
    got = one.cluster_cov_bands(E, perm, simultaneous=0.05, trace=True, first_slot=3, n_slots=2)
    _check_trace(got, ch, perm, E, None, 3, 2, "two draws")
    _check_reductions(got, 0.05, "two draws")
    one.close()


def test_empty_pair_list(func, full):
    smp = func["smp"]
    got = smp.cluster_cov_bands(full["E"], full["perm"], pairs=[], **full["kw"])
    assert got["mean"].shape == (0, 17, 17) and got["quantiles"].shape == (0, 17, 17, 3) and got["crit"].shape == (0,)
    assert got["trace"].shape == (0, 17, 17, 92) and got["pairs"].shape == (0, 2)
    got = smp.cluster_cov_bands(full["E"], full["perm"], pairs=[], diagonal=True, first_slot=func["first"], n_slots=func["S"])
    assert got["mean"].shape == (0, 17)
    # nothing is written
    m = np.full(4, 7.0)
    p = np.zeros(2, dtype=np.int32)
    dp = m.ctypes.data_as
    from bayesfmmm_amd import _lib
    rc = smp.lib.bfmmm_chain_cluster_cov_bands(smp.h, full["perm"].ctypes.data_as(IP), full["E"].ctypes.data_as(_lib.c_double_p), 17, None, 0, 0,
                                               p.ctypes.data_as(IP), 0, None, func["first"], func["S"], None, 0, 0.0, 0,
                                               dp(_lib.c_double_p), dp(_lib.c_double_p), None, None, None, None, None, 0)
    assert rc == 0 and np.all(m == 7.0)


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
        smp.select_chain(0)
        return out

    before = slots(a)
    E = _rows_of_basis(a, 20)
    r = a.align(first_slot=1, n_slots=6)
    a.cluster_cov_bands(E, r["perm"], simultaneous=0.05, trace=True, first_slot=1, n_slots=6)
    a.cluster_cov_bands(E[:5], r["perm"], E[5:], pairs=[(2, 1)], first_slot=1, n_slots=6, max_workspace_bytes=1 << 16)
    a.cluster_cov_bands(E, r["perm"][:, 1:4], diagonal=True, first_slot=2, n_slots=3)
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


def test_refusals(func, full):
    from bayesfmmm_amd import _lib
    smp = func["smp"]
    lib, T, NC, K = smp.lib, smp.T, smp.n_chains, smp.K
    dp = _lib.c_double_p
    G, S = 3, 8
    E = np.ascontiguousarray(func["E"][:G])
    perm = np.tile(np.arange(K, dtype=np.int32), (NC, S, 1))
    cap = 6 * G * G
    bufs = {k: np.zeros(cap) for k in ("mean", "sd", "crit", "lower", "upper")}
    quant = np.zeros(cap * 16)
    probs = np.array([0.025, 0.5, 0.975])
    keep = []

    def ptr(a, t=dp):
        if a is None:
            return None
        keep.append(a)
        return a.ctypes.data_as(t)

    base = dict(h=smp.h, perm=perm, E1=E, G1=G, E2=None, G2=0, diagonal=0, pairs=None, n_pairs=0, x=None, first_slot=0, n_slots=S,
                probs=probs, nq=3, alpha=0.05, budget=0, mean=bufs["mean"], sd=bufs["sd"], quant=quant, crit=None, lower=None, upper=None,
                trace=None, capacity=cap)

    def call(**over):
        a = dict(base, **over)
        return lib.bfmmm_chain_cluster_cov_bands(
            a["h"], ptr(a["perm"], IP), ptr(a["E1"]), a["G1"], ptr(a["E2"]), a["G2"], a["diagonal"], ptr(a["pairs"], IP), a["n_pairs"], ptr(a["x"]),
            a["first_slot"], a["n_slots"], ptr(a["probs"]), a["nq"], a["alpha"], a["budget"], ptr(a["mean"]), ptr(a["sd"]), ptr(a["quant"]),
            ptr(a["crit"]), ptr(a["lower"]), ptr(a["upper"]), ptr(a["trace"]), a["capacity"])

    def err(rc):
        assert rc != 0
        msg = lib.bfmmm_last_error().decode()
        assert msg.startswith("bfmmm_chain_cluster_cov_bands"), msg
        return msg

    def pl(v):
        return np.array(v, dtype=np.int32).reshape(-1)

    band = dict(crit=bufs["crit"], lower=bufs["lower"], upper=bufs["upper"])
    assert call() == 0 and call(**band) == 0
    for nm in ("h", "perm", "E1", "mean", "sd"):
        assert f"'{nm}' is null" in err(call(**{nm: None}))
    assert "'G1' must be at least 1" in err(call(G1=0))
    assert "'G2' must be at least 1 where 'E2' is given" in err(call(E2=E, G2=0))
    assert "'diagonal' requires 'E2' to be null" in err(call(E2=E, G2=G, diagonal=1))
    assert "'n_pairs' must not be negative" in err(call(pairs=pl([0, 0]), n_pairs=-1))
    assert f"'pairs'[1] = (0, {K}) outside 0 .. {K - 1}" in err(call(pairs=pl([0, 0, 0, K]), n_pairs=2))
    assert "'pairs'[0] = (-1, 0)" in err(call(pairs=pl([-1, 0]), n_pairs=1))
    assert "'x' is given but the sampler is not covariance-adjusted" in err(call(x=np.array([0.5, 0.5])))
    assert "'first_slot' out of range" in err(call(first_slot=T, n_slots=1))
    assert "'first_slot' out of range" in err(call(first_slot=-1))
    assert "'n_slots' out of range" in err(call(first_slot=2, n_slots=T - 1))
    assert "'n_slots' out of range" in err(call(n_slots=0))
    assert "'max_workspace_bytes' must not be negative" in err(call(budget=-1))
    assert f"'capacity' below {cap} entries" in err(call(capacity=cap - 1))
    assert f"'capacity' below {6 * G} entries" in err(call(diagonal=1, capacity=6 * G - 1))
    assert f"'capacity' below {2 * G * 2} entries" in err(call(E2=E, G2=2, pairs=pl([0, 1, 2, 2]), n_pairs=2, capacity=2 * G * 2 - 1))
    assert "'nq' outside 0 .. 16" in err(call(nq=17))
    assert "'nq' outside 0 .. 16" in err(call(nq=-1))
    assert "'probs'[1] outside [0, 1]" in err(call(probs=np.array([0.5, 1.5, 0.2])))
    assert "'probs'[0] outside [0, 1]" in err(call(probs=np.array([np.nan, 0.5, 0.2])))
    assert "'probs' is null" in err(call(probs=None))
    assert "'quant' is null" in err(call(quant=None))
    for bad in (0.0, 1.0, -0.1, np.nan):
        assert "'alpha' must be inside (0, 1)" in err(call(alpha=bad, **band))
    assert call(alpha=7.0) == 0                                         # alpha is checked only where the band is asked for
    for part in ({"crit": None}, {"lower": None}, {"upper": None}, {"lower": None, "upper": None}):
        assert "'crit', 'lower' and 'upper' must be all null or all set" in err(call(**dict(band, **part)))
    p2 = perm.copy()
    p2[2, 5] = [0, 0, 1]
    assert f"'perm' of chain 2, slot 5 is not a permutation of 0 .. {K - 1}" in err(call(perm=p2))
    p2 = perm.copy()
    p2[1, 0, 2] = K
    assert "'perm' of chain 1, slot 3 is not a permutation" in err(call(perm=p2, first_slot=3))
    assert "bytes one row needs" in err(call(budget=64))
    # the optional results are optional; G2 is ignored where E2 is null
    assert call(nq=0, probs=None, quant=None, G2=-5) == 0
    assert call(diagonal=1, capacity=6 * G) == 0
    # through the sampler
    S2 = func["S"]
    with pytest.raises(_lib.BfmmmError, match="'pairs'"):
        smp.cluster_cov_bands(E, full["perm"], pairs=[(0, 3)], first_slot=func["first"], n_slots=S2)
    with pytest.raises(_lib.BfmmmError, match="'alpha'"):
        smp.cluster_cov_bands(E, full["perm"], simultaneous=1.0, first_slot=func["first"], n_slots=S2)
    with pytest.raises(_lib.BfmmmError, match="'diagonal'"):
        smp.cluster_cov_bands(E, full["perm"], E, diagonal=True, first_slot=func["first"], n_slots=S2)
    with pytest.raises(_lib.BfmmmError, match="'G1'"):
        smp.cluster_cov_bands(E[:0], full["perm"], first_slot=func["first"], n_slots=S2)
    # shapes are checked before the library sees them
    with pytest.raises(ValueError):
        smp.cluster_cov_bands(np.zeros((3, smp.P + 1)), full["perm"], first_slot=func["first"], n_slots=S2)
    with pytest.raises(ValueError):
        smp.cluster_cov_bands(E, full["perm"], np.zeros((3, smp.P + 1)), first_slot=func["first"], n_slots=S2)
    with pytest.raises(ValueError):
        smp.cluster_cov_bands(E, full["perm"][:, :5], first_slot=func["first"], n_slots=S2)


def test_refusals_of_the_model():
    """a non-finite x (covariance-adjusted) and more than 2^22 draws: each check precedes any work on the slots.  The refusal of
    n_eigen = 0 cannot be reached: bfmmm_create refuses such a model ("'n_eigen' must be an integer greater than or equal to 1"),
    which is asserted here in its place."""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    smp, T = _cov_sampler(True)
    perm = np.tile(np.arange(smp.K, dtype=np.int32), (smp.n_chains, T, 1))
    E = _rows_of_basis(smp, 3)
    for bad in (np.nan, np.inf):
        with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_cluster_cov_bands: 'x'\[1\] is not finite"):
            smp.cluster_cov_bands(E, perm, x=[0.5, bad])
    smp.close()
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=0, tot_mcmc_iters=4)
    with pytest.raises(_lib.BfmmmError, match="'n_eigen' must be an integer greater than or equal to 1"):
        bf.Sampler(cfg, rng.standard_normal((6, 2)), n_chains=2)
    T = (1 << 21) + 1
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    dummy, one = np.zeros(2, dtype=np.int32), np.zeros(4)
    p1 = one.ctypes.data_as(_lib.c_double_p)
    rc = smp.lib.bfmmm_chain_cluster_cov_bands(smp.h, dummy.ctypes.data_as(IP), p1, 1, None, 0, 0, None, 0, None, 0, T, None, 0, 0.0, 0, p1, p1,
                                               None, None, None, None, None, 3)
    assert rc != 0 and re.search(r"bfmmm_chain_cluster_cov_bands: .*2\^22", smp.lib.bfmmm_last_error().decode())
    smp.close()


def test_timing_is_reported(func, full):
    smp, E, perm = func["smp"], full["E"], full["perm"]
    kw = dict(first_slot=func["first"], n_slots=func["S"])
    smp.cluster_cov_bands(E, perm, **kw)
    for name, launches in (("cluster_cov_project", 1), ("cluster_cov", 1), ("cluster_cov_maxdev", 0)):
        ms, n = smp.timing(name)
        assert n == launches and (ms > 0.0) == (launches > 0), name
    smp.cluster_cov_bands(E, perm, np.ascontiguousarray(func["E"][17:40]), pairs=[(1, 0)], simultaneous=0.05, **kw)
    assert smp.timing("cluster_cov_project")[1] == 2 and smp.timing("cluster_cov")[1] == 1
    ms, n = smp.timing("cluster_cov_maxdev")
    assert ms > 0.0 and n == 1
