"""Contrasts of cluster mean functions and covariate effects from chain slots on the device (kernels_cluster_contrast.hip; DESIGN.md
7t): Sampler.cluster_contrast_bands against the long-double restatement tests/cluster_contrast_ref.py fed the get_chain copies.  Slots
are planted with set_state + run(U_LOGLIK) by the helpers of tests/test_gpu_rescale.py; the row of 260 draws is a run of the sampler.

Values: every entry of `trace` within b = (P + K (D + 2) + 2) u abar of the restatement, u = 2^-52 (derived in the restatement's
docstring for the shipped order: k, then c with its d, then p, each from 0.0, one rounding per product and per sum; no path is longer
than the one counted).  Mean, sd and quantiles carry B = max b over a row by the rule of tests/test_gpu_align.py's docstring
(test_gpu_rescale._check_rows).  The pooled quantiles are bfmmm_post_col_quantiles of the trace's rows, and crit, lower and upper
tests/curve_sim_ref.py's rule on the trace with the device's own mean and sd, byte for byte: the rule tests/test_gpu_cluster_cov.py
uses for its band.  The norm: sqrt(sum_g w_g v^2) is a weighted 2-norm, so it moves by at most sqrt(sum_g w_g b_g^2) where every v_g
moves by at most b_g (the triangle inequality), plus its own roundings: a square, a product and a sum per grid point and the root,
(G + 3) u norm.  Its seven statistics are api.diagnostics of the returned norm_trace bit for bit.

prob_positive and p_sim are counts, not Lipschitz: the test first asserts that the restatement has no value within its bound of
the threshold (|v| > b; and every |dev - t| above what B and the bounds of mean and sd can move dev and t by), then asserts equal
counts.  The draws are continuous random numbers from fixed seeds, for which this holds; the guard says so if a seed ever fails it.

With permutation matrices and a single term (1, k) the sum over p is k_align_project's and the mixing is exact: mean, sd, quantiles
and the values equal cluster_mean_bands(E, perm) bit for bit.  With a rescale dict and (1, k, x) the mixing is rounded in another order
than k_rescale_project's: agreement within 2 B.

The refusal of more than 8 covariates cannot be reached: set_covariates refuses them first."""
import ctypes as C
import re

import numpy as np
import pytest

import cluster_cov_ref as CCR
import cluster_contrast_ref as CR
import test_gpu_rescale as RS
from test_gpu_cluster_cov import _col_quantiles

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
PROBS = (0.025, 0.5, 0.975)
STATS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")
KEYS = ("mean", "sd", "quantiles", "prob_positive")
BAND = ("crit", "lower", "upper", "excludes_zero", "p_sim")


def _planted(K, NCH, T, D, seed, n=12):
    """a sampler of the base shape (M = 2, degree 2, 5 internal knots: P = 8) with every slot planted; returns (smp, the get_chain copies, what was planted)"""
    smp = RS._make(n, K, NCH, T, D=D)
    assert smp.P == 8
    rng = np.random.default_rng(seed)
    draws = []
    for q in range(NCH):
        draws.append([])
        for t in range(T):
            Z = 0.9 * rng.dirichlet(np.full(K, 1.5), size=n) + 0.1 / K
            # K curves with 0.75 or more on their own component: two components cannot share their purest curve (no singular draw)
            Z[rng.choice(n, size=K, replace=False)] = 0.75 * np.eye(K) + 0.25 * rng.dirichlet(np.full(K, 1.5), size=K)
            d = {"Z": Z, "nu": rng.standard_normal((K, smp.P)) + 0.6 * np.arange(K)[:, None]}
            if D:
                d["eta"] = rng.standard_normal((smp.P, D, K))
            draws[q].append(d)
    return smp, RS._plant(smp, draws), draws


def _grid(G, P, seed=5):
    return np.ascontiguousarray(np.random.default_rng(seed).standard_normal((G, P)))


def _same(a, b, keys):
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for k in STATS + ("quantiles",):
        assert a["norm"][k].tobytes() == b["norm"][k].tobytes(), ("norm", k)


def _given(smp, perm, seed):
    """a rescale dict of given transforms: every draw's permutation matrix pulled towards the barycentre, well conditioned"""
    rng = np.random.default_rng(seed)
    K = smp.K
    A = 0.7 * CR.perm_matrix(perm) + 0.3 * rng.dirichlet(np.full(K, 1.5), size=perm.shape[:2] + (K,))
    r = smp.rescale(perm=perm, transform=np.ascontiguousarray(A))
    assert r["n_singular"] == 0
    return r


def _check(smp, chains, E, contrasts, first, S, label, perm=None, rescale=None, weights=None, alpha=0.1, bscale=1.0, ref_mix=None, **kw):
    """the whole result of one call against the restatement (ref_mix: the label maps the restatement takes, where `chains` are in
    another labelling than the slots); returns (got, v, b)"""
    from bayesfmmm_amd import api
    got = smp.cluster_contrast_bands(E, contrasts, perm=perm, rescale=rescale, weights=weights, probs=PROBS, simultaneous=alpha, trace=True,
                                     first_slot=first, n_slots=S, **kw)
    mix = ref_mix if ref_mix is not None else rescale["transform"] if rescale is not None else CR.perm_matrix(perm)
    w_nu, w_eta = got["w_nu"], got["w_eta"]
    R, G, N = w_nu.shape[0], E.shape[0], smp.n_chains * S
    assert (w_eta is None) == (smp.D == 0)
    v, abar = CR.pooled(chains, E, mix, w_nu, w_eta, first, S)
    b = bscale * CR.bound_count(smp.P, smp.K, smp.D) * U * np.asarray(abar, dtype=np.float64)
    v64 = np.asarray(v, dtype=np.float64)
    # ---- the values
    assert got["trace"].shape == (R, G, N) and got["norm_trace"].shape == (R, smp.n_chains, S)
    err = np.abs(got["trace"] - v64)
    print(f"{label}: {v.size} values, worst |device - restatement| / b = {float(np.max(err[b > 0] / b[b > 0])):.3e}")
    assert np.all(err <= b), label
    # ---- mean, sd and quantiles carry B; the quantiles are the host rule on the trace byte for byte
    RS._check_rows(got, v, b, PROBS, label)
    assert got["quantiles"].tobytes() == _col_quantiles(got["trace"].reshape(-1, N), got["probs"]).reshape(R, G, -1).tobytes(), label
    # ---- crit and the band from the trace with the device's own mean and sd, byte for byte
    s = CCR.sim_bands(got["trace"], alpha, got["mean"], got["sd"])
    assert got["crit"].shape == (R,) and got["alpha"] == alpha
    for k in ("crit", "lower", "upper"):
        assert got[k].tobytes() == np.ascontiguousarray(s[k]).tobytes(), (label, k)
    assert np.array_equal(got["excludes_zero"], (got["lower"] > 0) | (got["upper"] < 0))
    # ---- the counts: no value of the restatement within its bound of the threshold, then equal counts
    ref = CR.summary(v64, alpha, weights)
    assert np.all(np.abs(v64) > b), (label, "a value within its bound of zero: choose another seed")
    assert np.array_equal(got["prob_positive"], ref["prob_positive"]), label
    B = b.max(axis=-1)
    tm = B + N * U * np.mean(np.abs(v64), axis=-1)
    ts = np.sqrt(N / (N - 1.0)) * B + 4 * N * U * ref["sd"]
    t = CR.threshold(ref["mean"], ref["sd"])
    # dev_g = |v - mean| / sd moves by at most (B + tm + dev ts) / (sd - ts), |mean| / sd by (tm + t ts) / (sd - ts); twice the larger
    delta = 2.0 * np.max((B + tm + (ref["dev"].max(axis=-1) + t)[:, None] * ts) / (ref["sd"] - ts), axis=-1)
    gap = np.min(np.abs(ref["dev"] - t[:, None]), axis=-1)
    assert np.all(gap > delta), (label, "a deviation within its bound of t: choose another seed", gap, delta)
    assert np.array_equal(got["p_sim"], ref["p_sim"]), (label, got["p_sim"], ref["p_sim"])
    # ---- the size of the contrast per draw
    w = np.full(G, 1.0 / G) if weights is None else np.asarray(weights, dtype=np.float64)
    nref = np.asarray(CR.norm(v, None if weights is None else np.asarray(weights, dtype=CR.LD)), dtype=np.float64)
    nb = np.sqrt(np.einsum("g,rgn->rn", w, b * b)) + (G + 3) * U * nref
    nt = got["norm_trace"].reshape(R, N)
    print(f"{label}: worst |norm - restatement| / bound = {float(np.max(np.abs(nt - nref) / nb)):.3e}")
    assert np.all(np.abs(nt - nref) <= nb), label
    d = api.diagnostics(got["norm_trace"].transpose(2, 1, 0))      # (R, C, S) -> (S, C, R)
    for k in STATS:
        assert got["norm"][k].shape == (R,) and got["norm"][k].tobytes() == np.ascontiguousarray(d[k]).tobytes(), (label, "norm", k)
    assert got["norm"]["quantiles"].tobytes() == _col_quantiles(nt, got["probs"]).tobytes(), label
    return got, v, b


# ---- the base shape: n = 12, K = 3, M = 2, P = 8, 2 chains, G = 5 -----------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 2], ids=["D0", "D2"])
def base(request):
    D = request.param
    smp, chains, draws = _planted(3, 2, 9, D, 100 + D)
    d = dict(smp=smp, chains=chains, draws=draws, D=D, T=9, E=_grid(5, 8), perm=RS._random_perm(2, 9, 3, 7))
    d["rescale"] = smp.rescale(perm=d["perm"])
    assert d["rescale"]["n_singular"] == 0
    yield d
    smp.close()


def _lists(D):
    """contrasts of every kind the issue names: a difference, a single cluster, a difference of differences, and with covariates an
    effect, f_k(x) - f_k(x') and f_k(x) - f_l(x)"""
    out = [[(1, 0), (-1, 2)], [(1, 1)], [(1, 0), (-1, 1), (-1, 1), (1, 2)]]
    if D:
        x, x2 = [0.3, -1.2], [1.0, 0.5]
        out += [[(1, 1, x), (-1, 1, x2)], [(1, 0, x), (-1, 2, x)], [(0.5, 2, x)]]
    return out


@pytest.mark.parametrize("labels", ["perm", "rescale"])
def test_values_bands_counts_and_norm_against_the_restatement(base, labels):
    smp, T = base["smp"], base["T"]
    kw = {labels: base[labels]}
    got, _, _ = _check(smp, base["chains"], base["E"], "pairwise", 0, T, f"pairwise D={base['D']} {labels}", **kw)
    assert got["mean"].shape == (3, 5) and np.array_equal(got["w_nu"], [[1, -1, 0], [1, 0, -1], [0, 1, -1]])
    assert smp.timing("contrast_coef")[1] == 1 and smp.timing("contrast_values")[1] == 1 and smp.timing("contrast_norm")[1] == 1
    assert all(smp.timing(nm)[0] > 0.0 for nm in ("contrast_coef", "contrast_values", "contrast_norm"))
    w = np.array([0.5, 1.0, 0.0, 2.0, 0.25])
    _check(smp, base["chains"], base["E"], _lists(base["D"]), 0, T, f"lists D={base['D']} {labels}", weights=w, alpha=0.25, **kw)
    if base["D"]:
        got, _, _ = _check(smp, base["chains"], base["E"], "effects", 0, T, f"effects {labels}", **kw)
        assert got["mean"].shape == (6, 5)
    # a slot range of its own
    sub = {"perm": base["perm"][:, 2:7]} if labels == "perm" else {"rescale": smp.rescale(perm=base["perm"][:, 2:7], first_slot=2, n_slots=5)}
    _check(smp, base["chains"], base["E"], "pairwise", 2, 5, f"slots 2 .. 6 {labels}", **sub)


def test_invariances(base):
    smp, E, T, r = base["smp"], base["E"], base["T"], base["rescale"]
    lists = _lists(base["D"])
    kw = dict(rescale=r, probs=PROBS)
    full = smp.cluster_contrast_bands(E, lists, simultaneous=0.1, trace=True, **kw)
    _same(full, smp.cluster_contrast_bands(E, lists, simultaneous=0.1, trace=True, **kw), KEYS + BAND + ("trace", "norm_trace"))
    # any budget above the least: three chunks of five rows, and the least itself
    with pytest.raises(Exception) as ei:
        smp.cluster_contrast_bands(E, lists, simultaneous=0.1, trace=True, max_workspace_bytes=1, **kw)
    m = re.search(r"\((\d+) shared by all rows \+ (\d+) per row\)", str(ei.value))
    assert m and "bfmmm_chain_cluster_contrast_bands: 'max_workspace_bytes' below the" in str(ei.value), str(ei.value)
    shared, per = int(m.group(1)), int(m.group(2))
    rows = len(lists) * 5
    for chunk in (-(-rows // 3), 4, 1):
        few = smp.cluster_contrast_bands(E, lists, simultaneous=0.1, trace=True, max_workspace_bytes=shared + chunk * per, **kw)
        nch = -(-rows // chunk)
        assert nch >= 3 and smp.timing("contrast_values")[1] == 2 * nch and smp.timing("contrast_norm")[1] == nch      # two sweeps
        _same(full, few, KEYS + BAND + ("trace", "norm_trace"))
    with pytest.raises(Exception, match="'max_workspace_bytes' below the"):
        smp.cluster_contrast_bands(E, lists, simultaneous=0.1, max_workspace_bytes=shared + per - 1, **kw)
    # without the band one sweep; without trace; without both
    with pytest.raises(Exception) as ei:
        smp.cluster_contrast_bands(E, lists, trace=True, max_workspace_bytes=1, **kw)
    m = re.search(r"\((\d+) shared by all rows \+ (\d+) per row\)", str(ei.value))
    assert int(m.group(1)) < shared and int(m.group(2)) == per                # dev, crit and t are the band's
    nob = smp.cluster_contrast_bands(E, lists, trace=True, max_workspace_bytes=int(m.group(1)) + 4 * per, **kw)
    assert smp.timing("contrast_values")[1] == -(-rows // 4) and not any(k in nob for k in BAND + ("alpha",))
    _same(full, nob, KEYS + ("trace", "norm_trace"))
    notr = smp.cluster_contrast_bands(E, lists, simultaneous=0.1, **kw)
    assert "trace" not in notr and "norm_trace" not in notr
    _same(full, notr, KEYS + BAND)
    _same(full, smp.cluster_contrast_bands(E, lists, **kw), KEYS)
    # a sub-list and the reverse order
    idx = [2, 0] if not base["D"] else [4, 1, 3]
    sub = smp.cluster_contrast_bands(E, [lists[i] for i in idx], simultaneous=0.1, trace=True, **kw)
    rev = smp.cluster_contrast_bands(E, lists[::-1], simultaneous=0.1, trace=True, **kw)
    for k in KEYS + BAND + ("trace", "norm_trace"):
        assert sub[k].tobytes() == np.ascontiguousarray(full[k][idx]).tobytes(), ("sub-list", k)
        assert rev[k].tobytes() == np.ascontiguousarray(full[k][::-1]).tobytes(), ("reverse", k)
    for k in STATS + ("quantiles",):
        assert sub["norm"][k].tobytes() == np.ascontiguousarray(full["norm"][k][idx]).tobytes(), ("sub-list norm", k)
        assert rev["norm"][k].tobytes() == np.ascontiguousarray(full["norm"][k][::-1]).tobytes(), ("reverse norm", k)
    # another level leaves everything but the band
    _same(full, smp.cluster_contrast_bands(E, lists, simultaneous=0.3, trace=True, **kw), KEYS + ("p_sim", "trace", "norm_trace"))


def test_permutation_matrices_equal_cluster_mean_bands(base):
    smp, E, T, perm = base["smp"], base["E"], base["T"], base["perm"]
    want = smp.cluster_mean_bands(E, perm, probs=PROBS)                       # (K, G)
    got = smp.cluster_contrast_bands(E, [[(1, k)] for k in range(3)], perm=perm, probs=PROBS, trace=True)
    for k in ("mean", "sd", "quantiles"):
        assert got[k].tobytes() == want[k].tobytes(), k
    # the per-draw values too: the same sum over p from 0.0 of the same products (nu planted without a signed zero)
    for k in range(3):
        for q in range(2):
            for s in range(T):
                nu = base["chains"][q]["nu"][perm[q, s, k], :, s]
                v = np.zeros(E.shape[0])
                for p in range(smp.P):
                    v = v + E[:, p] * nu[p]
                assert got["trace"][k, :, q * T + s].tobytes() == v.tobytes(), (k, q, s)


def test_rescale_dict_agrees_with_cluster_mean_bands_at_x(base):
    """(1, k, x) under a rescale dict (without covariates: (1, k)) against cluster_mean_bands(rescale=, x=): two orders of the same
    sums, each within B of the exact rows"""
    smp, E, T, r = base["smp"], base["E"], base["T"], base["rescale"]
    x = [0.3, -1.2] if base["D"] else None
    want = smp.cluster_mean_bands(E, rescale=r, x=x, probs=PROBS)
    got = smp.cluster_contrast_bands(E, [[(1, k, x) if x else (1, k)] for k in range(3)], rescale=r, probs=PROBS)
    v, abar = CR.pooled(base["chains"], E, r["transform"], got["w_nu"], got["w_eta"], 0, T)
    b = CR.bound_count(smp.P, smp.K, smp.D) * U * np.asarray(abar, dtype=np.float64)
    B = b.max(axis=-1)
    N = v.shape[-1]
    sd = got["sd"]
    worst = {}
    for k, tol in (("mean", 2 * B + 2 * N * U * np.mean(np.abs(np.asarray(v, dtype=np.float64)), axis=-1)),
                   ("sd", 2 * np.sqrt(N / (N - 1.0)) * B + 8 * N * U * sd),
                   ("quantiles", (2 * B)[..., None] + 4 * U * np.abs(got["quantiles"]))):
        e = np.abs(got[k] - want[k])
        worst[k] = float(np.max(e / tol))
        assert np.all(e <= tol), (k, worst[k])
    print("rescale dict, (1, k, x) against cluster_mean_bands(rescale=, x=): worst difference / (2 B rule) " +
          ", ".join(f"{k} {val:.3e}" for k, val in worst.items()))


def test_relabelling_one_chain_moves_nothing_by_more_than_2b(base):
    """chain 1's components renamed in every draw, perm adjusted to match: the same posterior.  The planted slots are restored afterwards."""
    smp, E, T, perm, draws = base["smp"], base["E"], base["T"], base["perm"], base["draws"]
    lists = _lists(base["D"])
    rng = np.random.default_rng(31)
    moved, perm2 = [list(draws[0]), []], perm.copy()
    for t in range(T):
        sg = rng.permutation(3)                       # new label j holds what was component sg[j]
        d = {"Z": np.ascontiguousarray(draws[1][t]["Z"][:, sg]), "nu": np.ascontiguousarray(draws[1][t]["nu"][sg])}
        if base["D"]:
            d["eta"] = np.ascontiguousarray(draws[1][t]["eta"][:, :, sg])
        moved[1].append(d)
        perm2[1, t] = np.argsort(sg)[perm[1, t]]
    try:
        RS._plant(smp, moved)
        # against the restatement of the original labelling, with twice its bound
        _check(smp, base["chains"], E, lists, 0, T, "relabelled, perm", perm=perm2, bscale=2.0, ref_mix=CR.perm_matrix(perm))
        r2 = smp.rescale(perm=perm2)
        assert np.array_equal(r2["curve"], base["rescale"]["curve"])          # the same pure curves under either labelling
        got = smp.cluster_contrast_bands(E, lists, rescale=r2, probs=PROBS, simultaneous=0.1, trace=True)
    finally:
        RS._plant(smp, draws)
    # the transform's columns are summed in another order: within 2 b of the restatement of the original labelling
    was = smp.cluster_contrast_bands(E, lists, rescale=base["rescale"], probs=PROBS, simultaneous=0.1, trace=True)
    v, abar = CR.pooled(base["chains"], E, base["rescale"]["transform"], was["w_nu"], was["w_eta"], 0, T)
    b = CR.bound_count(smp.P, smp.K, smp.D) * U * np.asarray(abar, dtype=np.float64)
    assert np.all(np.abs(got["trace"] - np.asarray(v, dtype=np.float64)) <= 2 * b)
    RS._check_rows(got, v, 2 * b, PROBS, "relabelled, rescale")
    # (the counts of these contrasts are decidable: test_values_bands_counts_and_norm_against_the_restatement's guard, whose margin is
    # many orders above b)
    assert np.array_equal(got["prob_positive"], was["prob_positive"]) and np.array_equal(got["p_sim"], was["p_sim"])


def test_two_clusters_with_the_same_nu_differ_by_exactly_zero():
    """raw components 0 and 2 hold the same nu in every draw, and every draw's perm is the identity or swaps the two"""
    smp, chains, draws = _planted(3, 2, 6, 0, 55)
    RS._plant(smp, [[dict(d, nu=np.ascontiguousarray(d["nu"][[0, 1, 0]])) for d in row] for row in draws])
    swap = np.random.default_rng(9).integers(0, 2, size=(2, 6)).astype(bool)
    perm = np.where(swap[..., None], np.array([2, 1, 0], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32)).astype(np.int32)
    assert swap.any() and not swap.all()
    got = smp.cluster_contrast_bands(_grid(5, 8), [[(1, 0), (-1, 2)], [(1, 0), (-1, 1)]], perm=perm, simultaneous=0.1, trace=True)
    assert not got["trace"][0].any() and not got["mean"][0].any() and not got["sd"][0].any() and not got["prob_positive"][0].any()
    assert got["crit"][0] == 0.0 and got["p_sim"][0] == 1.0 and not got["excludes_zero"][0].any()
    assert not got["lower"][0].any() and not got["upper"][0].any() and not got["norm_trace"][0].any() and got["norm"]["mean"][0] == 0.0
    assert got["trace"][1].all() and got["crit"][1] > 0.0
    smp.close()


# ---- other shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5])
def test_other_K(K):
    """K = 5 crosses the KP boundary of k_rescale_transform"""
    smp, chains, _ = _planted(K, 2, 7, 2, 200 + K)
    perm = RS._random_perm(2, 7, K, K)
    r = _given(smp, perm, 10 + K)
    E = _grid(5, 8)
    got, _, _ = _check(smp, chains, E, "pairwise", 0, 7, f"K={K} pairwise, given transforms", rescale=r)
    assert got["mean"].shape == (K * (K - 1) // 2, 5)
    _check(smp, chains, E, "effects", 0, 7, f"K={K} effects, perm", perm=perm)
    smp.close()


def test_three_chains_of_seven_slots_and_a_partial_grid_tile():
    """N = 21; G = 17"""
    smp, chains, _ = _planted(3, 3, 7, 0, 77)
    perm = RS._random_perm(3, 7, 3, 2)
    got, _, _ = _check(smp, chains, _grid(17, 8), "pairwise", 0, 7, "N=21 G=17", perm=perm)
    assert got["trace"].shape == (3, 17, 21)
    smp.close()


def test_a_second_partial_block_of_draws():
    """N = 260 = 2 x 130: a second, partial block of 256 draws in k_contrast_values and k_contrast_norm, a fifth, partial wave of
    k_contrast_coef; the slots are a run of the sampler"""
    import bayesfmmm_amd as bf
    T = 130
    smp = RS._make(40, 3, 2, T)
    smp.run(bf.SWEEP_WARM, T, seed=3)
    chains = RS._copies(smp, ["nu", "Z"])
    perm = smp.align()["perm"]
    _check(smp, chains, _grid(5, 8), "pairwise", 0, T, "N=260 perm", perm=perm)
    _check(smp, chains, _grid(5, 8), [[(1, 0), (-1, 1)], [(1, 2)]], 0, T, "N=260 given transforms", rescale=_given(smp, perm, 8))
    smp.close()


def test_multivariate_with_the_identity():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, T, NCH = 20, 6, 3, 8, 2
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)) + np.repeat(np.arange(2.0), n // 2)[:, None], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    chains = RS._copies(smp, ["nu", "Z"])
    got, _, _ = _check(smp, chains, np.eye(P), "pairwise", 0, T, "multivariate, E = I", perm=smp.align()["perm"])
    assert got["mean"].shape == (3, P)
    smp.close()


# ---- refusals, each by its message -----------------------------------------------------------------------------------------------
def _raw(smp, S, **over):
    """a valid call of the entry point itself with some arguments replaced; returns (rc, message)"""
    from bayesfmmm_amd.sampler import _dp, _ip
    K, D, N, G, R = smp.K, smp.D, smp.n_chains * S, 5, 2
    a = dict(mix=np.ascontiguousarray(np.tile(np.eye(K), (N, 1, 1))), E=_grid(G, smp.P), G=G, w_nu=np.ascontiguousarray(np.eye(K)[:R]),
             w_eta=np.zeros((R, K, D)) if D else None, R=R, weights=None, first_slot=0, n_slots=S, probs=np.array(PROBS), nq=3, alpha=0.1, budget=0,
             mean=np.zeros(R * G), sd=np.zeros(R * G), quant=np.zeros(R * G * 3), n_positive=np.zeros(R * G, dtype=np.int32), crit=np.zeros(R),
             lower=np.zeros(R * G), upper=np.zeros(R * G), n_exceed=np.zeros(R, dtype=np.int32), norm_stats=np.zeros(7 * R),
             norm_quant=np.zeros(3 * R), trace=None, norm_trace=None, capacity=R * G)
    a.update(over)
    p = lambda k: None if a[k] is None else (_ip(a[k]) if a[k].dtype == np.int32 else _dp(a[k]))
    rc = smp.lib.bfmmm_chain_cluster_contrast_bands(
        smp.h, p("mix"), p("E"), a["G"], p("w_nu"), p("w_eta"), a["R"], p("weights"), a["first_slot"], a["n_slots"], p("probs"), a["nq"],
        C.c_double(a["alpha"]), a["budget"], p("mean"), p("sd"), p("quant"), p("n_positive"), p("crit"), p("lower"), p("upper"), p("n_exceed"),
        p("norm_stats"), p("norm_quant"), p("trace"), p("norm_trace"), a["capacity"])
    return rc, smp.lib.bfmmm_last_error().decode()


def test_refusals(base):
    from bayesfmmm_amd._lib import BfmmmError
    smp, T, K, D = base["smp"], base["T"], 3, base["D"]
    fn = "bfmmm_chain_cluster_contrast_bands: "
    assert _raw(smp, T)[0] == 0                                    # the helper's call is valid as it stands
    nan_nu, zero_nu = np.eye(K)[:2].copy(), np.eye(K)[:2].copy()
    nan_nu[1, 2], zero_nu[1] = np.inf, 0.0
    cases = [(dict(mix=None), "'mix' is null"), (dict(E=None), "'E' is null"), (dict(w_nu=None), "'w_nu' is null"), (dict(mean=None), "'mean' is null"),
             (dict(sd=None), "'sd' is null"), (dict(n_positive=None), "'n_positive' is null"), (dict(norm_stats=None), "'norm_stats' is null"),
             (dict(quant=None), "'quant' is null"), (dict(norm_quant=None), "'norm_quant' is null"), (dict(probs=None), "'probs' is null"),
             (dict(G=0), "'G' must be at least 1"), (dict(R=0), "'R' = 0 outside 1 .. 64"), (dict(R=65), "'R' = 65 outside 1 .. 64"),
             (dict(w_nu=zero_nu), "contrast 1 has no weight other than zero"), (dict(w_nu=nan_nu), r"'w_nu'[1, 2] is not finite"),
             (dict(weights=np.array([1.0, 1.0, -0.5, 1.0, 1.0])), "'weights'[2] is negative or not finite"),
             (dict(weights=np.array([1.0, np.inf, 1.0, 1.0, 1.0])), "'weights'[1] is negative or not finite"),
             (dict(weights=np.array([1.0, 1.0, 1.0, np.nan, 1.0])), "'weights'[3] is negative or not finite"),
             (dict(alpha=0.0), "'alpha' must be inside (0, 1)"), (dict(alpha=1.0), "'alpha' must be inside (0, 1)"),
             (dict(crit=None), "'crit', 'lower', 'upper' and 'n_exceed' must be all null or all set"),
             (dict(capacity=9), "'capacity' below 10 rows"), (dict(first_slot=T), "'first_slot' out of range"),
             (dict(n_slots=T + 1), "'n_slots' out of range"), (dict(budget=-1), "'max_workspace_bytes' must not be negative"),
             (dict(nq=17), "'nq' outside 0 .. 16")]
    if D:
        bad = np.zeros((2, K, D))
        bad[0, 1, 1] = np.nan
        cases.append((dict(w_eta=bad), "'w_eta'[0, 1, 1] is not finite"))
        cases.append((dict(w_nu=zero_nu, w_eta=np.zeros((2, K, D))), "contrast 1 has no weight other than zero"))
        only_eta = np.zeros((2, K, D))
        only_eta[1, 0, 1] = 2.0
        assert _raw(smp, T, w_nu=zero_nu, w_eta=only_eta)[0] == 0          # a weight on eta alone is a contrast
    else:
        cases.append((dict(w_eta=np.ones((2, K, 1))), "'w_eta' is given but the sampler has no covariates"))
    for over, msg in cases:
        rc, text = _raw(smp, T, **over)
        assert rc != 0 and text.startswith(fn + msg), (over, text)
    # the band's level is not read without the band
    assert _raw(smp, T, alpha=7.0, crit=None, lower=None, upper=None, n_exceed=None)[0] == 0
    # through the method
    E = base["E"]
    with pytest.raises(BfmmmError, match="contrast 0 has no weight other than zero"):
        smp.cluster_contrast_bands(E, [[(1, 0), (-1, 0)]], perm=base["perm"])
    with pytest.raises(BfmmmError, match="'R' = 65 outside 1 .. 64"):
        smp.cluster_contrast_bands(E, [[(1, 0)]] * 65, perm=base["perm"])
    with pytest.raises(BfmmmError, match=r"'alpha' must be inside \(0, 1\)"):
        smp.cluster_contrast_bands(E, perm=base["perm"], simultaneous=1.5)
    with pytest.raises(BfmmmError, match=r"'weights'\[0\] is negative or not finite"):
        smp.cluster_contrast_bands(E, perm=base["perm"], weights=[-1.0, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="weights must have 5 entries"):
        smp.cluster_contrast_bands(E, perm=base["perm"], weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="exactly one of 'perm' and 'rescale'"):
        smp.cluster_contrast_bands(E)
    with pytest.raises(ValueError, match="exactly one of 'perm' and 'rescale'"):
        smp.cluster_contrast_bands(E, perm=base["perm"], rescale=base["rescale"])
    with pytest.raises(ValueError, match="every row of perm must be a permutation of 0 .. 2"):
        smp.cluster_contrast_bands(E, perm=np.zeros_like(base["perm"]))
    with pytest.raises(ValueError, match=r"rescale is of slots \[0, 9\), not of \[2, 9\)"):
        smp.cluster_contrast_bands(E, rescale=base["rescale"], first_slot=2)
    if not D:
        with pytest.raises(ValueError, match="requires covariates"):
            smp.cluster_contrast_bands(E, "effects", perm=base["perm"])


def test_row_limit_is_refused_before_any_work():
    """more than 2^22 draws a row: a model of two curves with 2^21 + 1 slots in each of two chains, as tests/test_gpu_cluster_cov.py builds it"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd.sampler import _dp, _ip
    T = (1 << 21) + 1
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, np.random.default_rng(1).standard_normal((2, 2)), n_chains=2)
    one, w, cnt = np.zeros(8), np.array([1.0, -1.0]), np.zeros(2, dtype=np.int32)
    rc = smp.lib.bfmmm_chain_cluster_contrast_bands(smp.h, _dp(one), _dp(one), 1, _dp(w), None, 1, None, 0, T, None, 0, 0.0, 0, _dp(one), _dp(one),
                                                    None, _ip(cnt), None, None, None, None, _dp(one), None, None, None, 1)
    assert rc != 0 and re.search(r"bfmmm_chain_cluster_contrast_bands: .*2\^22", smp.lib.bfmmm_last_error().decode())
    smp.close()
