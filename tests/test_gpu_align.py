"""Label alignment against a pivot and the pooled cluster summaries on the device (kernels_align.hip).

Sampler.align against the numpy restatement (tests/align_ref.py) fed the get_chain("Z") copies: perm equal on every decidable
draw, score within bound = (n + K + 2) 2^-52 score on every draw; planted labels and exact ties; Sampler.aligned_summary
against Sampler.diagnostics (identity), against api.diagnostics and bfmmm_post_col_quantiles of the host-aligned get_chain
copies (byte for byte), Sampler.cluster_mean_bands against numpy on the aligned get_chain("nu").

Bounds of cluster_mean_bands, derived, with u = 2^-52 and N = C S draws a row.  A value is a sum of P products: device and numpy
each within P u / 2 sum_p |E_gp nu_kp| of the exact one, so they differ by at most b = P u sum_p |E_gp nu_kp|; B = max b over
the row.  Order statistics and the mean are 1-Lipschitz in the sup norm, the quantile rule is a convex combination of two order
statistics rounded three times: |quantile - numpy's| <= B + 2 u |q|.  Mean: B plus the N u mean|v| that
tests/test_gpu_curve_fit.py allows curve_bands' mean over equal values.  sd = |v - mean|_2 / sqrt(N - 1) moves by at most
sqrt(N / (N - 1)) B when every value moves by at most B, plus the relative 4 N u allowed there over equal values."""
import ctypes as C

import numpy as np
import pytest

import align_ref as R
import curve_fit_ref as FR
from simdata import simulate_functional, truth_chain
from test_gpu_chain_batch import _states, make_sampler_batch

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
PROBS = (0.025, 0.5, 0.975)
STATE = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "tau", "gamma", "Phi", "loglik"]
COMPONENT = ["nu", "Phi", "gamma", "Z", "pi", "tau", "delta", "A"]
COV_NAMES = ["eta", "xi", "tau_eta", "gamma_xi", "delta_xi", "A_xi"]
STATS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")
IP = C.POINTER(C.c_int32)


def _chain_copies(smp, names):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in names})
    smp.select_chain(0)
    return out


def _identity(smp, S):
    return np.tile(np.arange(smp.K, dtype=np.int32), (smp.n_chains, S, 1))


def _check_align(a, zchains, Zref, first, S, label, max_undecidable=0.0):
    """perm equal on every decidable draw and score within the bound on every draw; prints the undecidable count"""
    n, K = Zref.shape
    perm, score, dec = R.align(zchains, Zref, first, S)
    und = int((~dec).sum())
    b = R.bound(score, n, K)
    err = np.abs(a["score"] - score)
    print(f"{label} n={n} K={K} draws={dec.size}: {und} undecidable, worst |score - restatement| / bound "
          f"{float(np.max(err / b)):.3e}")
    assert a["perm"].shape == perm.shape and a["perm"].dtype == np.int32 and a["score"].shape == score.shape, label
    assert und <= max_undecidable * dec.size, (label, und)
    assert np.array_equal(a["perm"][dec], perm[dec]), label
    assert np.all(np.sort(a["perm"], axis=-1) == np.arange(K)), label
    assert np.all(err <= b), label
    return perm, dec


def _rows(chains, name, perm, first, S):
    """the rows aligned_summary gathers, from the get_chain copies: (len, C, S), element index in the reference's (column-major)
    order, each slot's components relabelled by perm[q, s]"""
    out = []
    for q, ch in enumerate(chains):
        x = np.asarray(ch[name])
        full = np.zeros((x.shape[0] if name == "tau" else x.shape[-1], perm.shape[2]), dtype=np.int64)
        full[first:first + S] = perm[q]
        y = R.relabel(x, name, full, perm.shape[2])
        y = y.T if name == "tau" else y.reshape(-1, y.shape[-1], order="F")
        out.append(y[:, first:first + S])
    return np.ascontiguousarray(np.stack(out, axis=1))


def _host_summary(rows, probs):
    """api.diagnostics and bfmmm_post_col_quantiles of the table rows (len, C, S)"""
    from bayesfmmm_amd import api
    L, Cn, S = rows.shape
    stats = api.diagnostics(np.ascontiguousarray(rows.transpose(2, 1, 0)))
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    q = np.zeros((L, pr.size))
    V = np.ascontiguousarray(rows.reshape(L, Cn * S))
    api._check(api._lib_entry().bfmmm_post_col_quantiles(V.ctypes.data_as(api.c_double_p), Cn * S, L, pr.ctypes.data_as(api.c_double_p),
                                                         pr.size, 0, q.ctypes.data_as(api.c_double_p)))
    return stats, q


def _check_summary_against_host(smp, chains, name, perm, first, S, probs=PROBS, **kw):
    got = smp.aligned_summary(name, perm, probs=probs, first_slot=first, n_slots=S, **kw)
    stats, q = _host_summary(_rows(chains, name, perm, first, S), probs)
    for k in STATS:
        assert np.ravel(got[k], order="F").tobytes() == np.ascontiguousarray(stats[k]).tobytes(), (name, k)
    L = q.shape[0]
    gq = got["quantiles"].reshape((L, len(probs)), order="F") if got["quantiles"].ndim > 1 else got["quantiles"].reshape(1, -1)
    assert np.ascontiguousarray(gq).tobytes() == q.tobytes(), name
    return got


def _check_cluster_bands(smp, chains, E, perm, first, S, probs=PROBS, label="", **kw):
    got = smp.cluster_mean_bands(E, perm, probs=probs, first_slot=first, n_slots=S, **kw)
    K, G, P = smp.K, E.shape[0], smp.P
    nu = _rows(chains, "nu", perm, first, S).reshape(P, K, smp.n_chains * S).transpose(1, 0, 2)      # element k + K p, draw q S + s
    v = np.einsum("gp,kpt->kgt", E, nu)
    b = P * U * np.einsum("gp,kpt->kgt", np.abs(E), np.abs(nu))
    B = b.max(axis=-1)
    N = v.shape[-1]
    assert got["mean"].shape == (K, G) and got["sd"].shape == (K, G) and got["quantiles"].shape == (K, G, len(probs))
    q = FR.quantiles(v, probs)
    eq = np.abs(got["quantiles"] - q)
    tq = B[..., None] + 2 * U * np.abs(q)
    mean, sd = FR.moments(v)
    em, tm = np.abs(got["mean"] - mean), B + N * U * np.mean(np.abs(v), axis=-1)
    print(f"{label} K={K} G={G} N={N}: worst |quantile - numpy| / bound {float(np.max(eq / tq)):.3e}, "
          f"|mean - numpy| / bound {float(np.max(em / tm)):.3e}")
    assert np.all(eq <= tq), label
    assert np.all(em <= tm), label
    if N > 1:
        es, ts = np.abs(got["sd"] - sd), np.sqrt(N / (N - 1.0)) * B + 4 * N * U * sd
        print(f"{label}: worst |sd - numpy| / bound {float(np.max(es / ts)):.3e}")
        assert np.all(es <= ts), label
    return got, v, B


def _basis_rows(smp, G):
    return np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:G])


@pytest.fixture(scope="module")
def func():
    """n = 61 ragged, K = 3, 4 chains, T = 30; slots 7 .. 29 are 92 draws: fewer curves than threads.  Aligned once against the
    representative draw."""
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
    first, S = 7, T - 7
    d = dict(smp=smp, chains=_chain_copies(smp, STATE), first=first, S=S, a=smp.align(first_slot=first, n_slots=S))
    yield d
    smp.close()


def _k_sampler(K, n, T, NCH, M=2, degree=2, n_internal=5):
    from test_gpu_similarity_loss import _k_sampler as make
    return make(K, M, degree, n_internal, n, T, NCH)


@pytest.fixture(scope="module")
def small():
    """n = 130, K = 3, P = 8, C = 2, slots 2 .. 13: the sampler of the budget, determinism, refusal and timing tests"""
    smp = _k_sampler(3, 130, 14, 2)
    first, S = 2, 12
    d = dict(smp=smp, chains=_chain_copies(smp, STATE), first=first, S=S, a=smp.align(first_slot=first, n_slots=S))
    yield d
    smp.close()


def test_fewer_curves_than_threads_matches_restatement(func):
    smp, a, first, S = func["smp"], func["a"], func["first"], func["S"]
    assert set(a) == {"perm", "score", "pivot", "chain_perm", "modal_share"}
    piv = a["pivot"]
    rep = smp.representative_draw(("Z",), first_slot=first, n_slots=S)
    assert (piv["chain"], piv["slot"]) == (rep["chain"], rep["slot"]) and piv["Z"].tobytes() == rep["Z"].tobytes()
    z = [ch["Z"] for ch in func["chains"]]
    perm, dec = _check_align(a, z, piv["Z"], first, S, "functional, pivot = representative draw", max_undecidable=0.05)
    # the pivot aligns to itself
    assert np.array_equal(a["perm"][piv["chain"], piv["slot"] - first], [0, 1, 2])
    # chain_perm and modal_share are the host's count of perm
    for q in range(4):
        rows, counts = np.unique(a["perm"][q], axis=0, return_counts=True)
        assert np.array_equal(a["chain_perm"][q], rows[np.argmax(counts)]) and a["modal_share"][q] == counts.max() / S
    # the same pivot given as (chain, slot) and as an array
    for pivot in ((piv["chain"], piv["slot"]), piv["Z"]):
        again = smp.align(pivot=pivot, first_slot=first, n_slots=S)
        assert again["perm"].tobytes() == a["perm"].tobytes() and again["score"].tobytes() == a["score"].tobytes()
    assert again["pivot"] is None


@pytest.mark.parametrize("K,M,degree,n_internal", [
    (3, 2, 2, 5),      # the K <= 4 instantiation with a padded component
    (5, 2, 3, 4),      # the K <= 8 instantiation, three padded components
    (8, 2, 2, 5),      # no padding, 256 masks
])
def test_one_stride_with_a_short_tail(K, M, degree, n_internal):
    """n = 130: every thread has at most one curve, the first 130 one; C = 2, S = 12, pivot = chain 1's last draw"""
    smp = _k_sampler(K, 130, 14, 2, M, degree, n_internal)
    a = smp.align(pivot=(1, 13), first_slot=2)
    z = [ch["Z"] for ch in _chain_copies(smp, ["Z"])]
    assert a["pivot"]["Z"].tobytes() == np.ascontiguousarray(z[1][:, :, 13]).tobytes()
    _check_align(a, z, a["pivot"]["Z"], 2, 12, "n = 130", max_undecidable=0.05)
    assert np.array_equal(a["perm"][1, 11], np.arange(K))
    smp.close()


def test_two_full_strides_and_a_tail_of_three():
    smp = _k_sampler(4, 515, 6, 2)
    a = smp.align(first_slot=1)
    z = [ch["Z"] for ch in _chain_copies(smp, ["Z"])]
    _check_align(a, z, a["pivot"]["Z"], 1, 5, "n = 515", max_undecidable=0.05)
    smp.close()


def _planted_pair(D):
    """two batches (n = 70, K = 3, 3 chains) whose chain states are the same up to the components' labels, the second's permuted
    per chain; U_LOGLIK runs, so that the slots hold what was set.  D > 0: with covariates."""
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=70, M=2, sigma_sq=0.01, seed=36, ragged=True)
    NCH, T = 3, 4
    states = _states(sim, NCH)
    perms = ([2, 0, 1], [1, 0, 2], [1, 2, 0])
    cvals = [8.0, 10.0, 12.0]
    rng = np.random.default_rng(8)
    X = rng.standard_normal((sim["n"], D)) if D else None
    a = make_sampler_batch(sim, T, NCH, c=cvals)
    b = make_sampler_batch(sim, T, NCH, c=cvals)
    if D:
        for smp in (a, b):
            smp.set_covariates(X, covariance_adj=True)
    for q in range(NCH):
        perm = perms[q]
        st = dict(states[q])
        if D:
            for nm in COV_NAMES:
                shp = a._draw_shape(nm)
                st[nm] = rng.gamma(2.0, 1.0, size=shp) if nm in ("tau_eta", "gamma_xi", "delta_xi", "A_xi") else rng.standard_normal(shp)
        pst = dict(st)
        for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau") + (("tau_eta", "delta_xi", "A_xi") if D else ()):
            pst[nm] = np.asarray(st[nm])[perm]
        pst["Z"] = np.asarray(st["Z"])[:, perm]
        if D:
            pst["eta"] = st["eta"][:, :, perm]
            pst["xi"] = st["xi"][..., perm]
            pst["gamma_xi"] = st["gamma_xi"][..., perm]
        a.select_chain(q)
        a.set_state(**st)
        b.select_chain(q)
        b.set_state(**pst)
    for smp in (a, b):
        smp.select_chain(0)
        smp.run(S.U_LOGLIK, T, seed=1)
    names = COMPONENT + (COV_NAMES if D else [])
    ca, cb = _chain_copies(a, names), _chain_copies(b, names)
    for q in range(NCH):
        full = np.tile(np.asarray(perms[q]), (T, 1))
        for nm in names:      # the plant took: b's slots are a's relabelled, and not a's
            assert np.array_equal(cb[q][nm], R.relabel(ca[q][nm], nm, full, 3)), (q, nm)
            assert not np.array_equal(cb[q][nm], ca[q][nm]), (q, nm)
    return a, b, ca, cb, perms, names, T


@pytest.mark.parametrize("D", [0, 2])
def test_planted_labels(D):
    a, b, ca, cb, perms, names, T = _planted_pair(D)
    Zref = np.ascontiguousarray(ca[2]["Z"][:, :, 0])
    ra, rb = a.align(pivot=Zref), b.align(pivot=Zref)
    for smp, chains, r in ((a, ca, ra), (b, cb, rb)):
        perm, dec = _check_align(r, [ch["Z"] for ch in chains], Zref, 0, T, f"planted, D = {D}")
        assert dec.all()
    for q in range(3):
        # column j of b's draw is column perms[q][j] of a's: b's row c of A is a's row perms[q][c], the same sums in the same
        # order, so the maximisers correspond exactly: perm_a = perms[q][perm_b]
        assert np.array_equal(np.asarray(perms[q])[rb["perm"][q]], ra["perm"][q]), q
        assert rb["score"][q].tobytes() == ra["score"][q].tobytes(), q
    assert np.array_equal(ra["perm"][2], np.tile(np.arange(3, dtype=np.int32), (T, 1)))
    assert np.all(ra["modal_share"] == 1.0) and np.all(rb["modal_share"] == 1.0)
    for nm in names:
        sa = a.aligned_summary(nm, ra["perm"], probs=PROBS)
        sb = b.aligned_summary(nm, rb["perm"], probs=PROBS)
        for k in STATS + ("quantiles",):
            assert sa[k].tobytes() == sb[k].tobytes(), (nm, k)
        assert sa["mean"].shape == a._draw_shape(nm) and sa["quantiles"].shape == a._draw_shape(nm) + (3,), nm
        assert np.all(np.isfinite(sa["mean"])) and np.all(np.isfinite(sa["quantiles"])), nm
        # and they are the host's
        _check_summary_against_host(a, ca, nm, ra["perm"], 0, T)
    if D:      # the covariate arrays under the identity: diagnostics' bytes (the other names: test_identity_equals_diagnostics_bitwise)
        for nm in COV_NAMES:
            got, ref = a.aligned_summary(nm, _identity(a, T), probs=()), a.diagnostics(nm)
            for k in STATS:
                assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (nm, k)
    E = _basis_rows(a, 9)
    ma, mb = a.cluster_mean_bands(E, ra["perm"]), b.cluster_mean_bands(E, rb["perm"])
    for k in ("mean", "sd", "quantiles"):
        assert ma[k].tobytes() == mb[k].tobytes(), k
    a.close()
    b.close()


def test_ties_on_the_device():
    """planted memberships with entries in {0, 1/2, 1}: every sum is exact, ties go to the lexicographically smallest
    permutation"""
    import bayesfmmm_amd as bf
    from test_align_ref import tied_cases
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=36, ragged=True)
    cases = [c for c in tied_cases() if c[0].shape == (61, 3)]
    assert len(cases) == 3
    states = _states(sim, 3)
    smp = make_sampler_batch(sim, 2, 3)
    for q, (Z, _, _) in enumerate(cases):
        smp.select_chain(q)
        smp.set_state(**dict(states[q], Z=Z))
    smp.select_chain(0)
    smp.run(bf.sampler.U_LOGLIK, 2, seed=1)
    z = [ch["Z"] for ch in _chain_copies(smp, ["Z"])]
    for q, (Z, Zref, label) in enumerate(cases):
        assert np.array_equal(z[q][:, :, 1], Z), label
        want, score, second = R.assign(R.gram(Z, Zref, np.float64))
        assert score == second, label      # a tie
        got = smp.align(pivot=Zref)
        assert np.array_equal(got["perm"][q], np.tile(want, (2, 1))), (label, got["perm"][q], want)
        assert np.all(got["score"][q] == float(score)), label
    smp.close()


def test_identity_equals_diagnostics_bitwise(func):
    smp, first, S = func["smp"], func["first"], func["S"]
    ident = _identity(smp, S)
    for nm in STATE:
        got = smp.aligned_summary(nm, ident, probs=(), first_slot=first, n_slots=S)
        ref = smp.diagnostics(nm, first_slot=first, n_slots=S)
        for k in STATS:
            assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (nm, k)
        assert got["quantiles"].shape[-1] == 0


def test_summary_equals_the_host_on_aligned_copies(func):
    smp, a, first, S = func["smp"], func["a"], func["first"], func["S"]
    assert len(np.unique(a["perm"].reshape(-1, 3), axis=0)) > 1      # the chains do label differently
    for nm in COMPONENT + ["chi", "sigma_sq"]:
        got = _check_summary_against_host(smp, func["chains"], nm, a["perm"], first, S)
        assert got["mean"].shape == smp._draw_shape(nm)
    z = smp.aligned_summary("Z", a["perm"], first_slot=first, n_slots=S)
    assert z["quantiles"].shape == (61, 3, 3) and np.all(z["quantiles"][..., 0] <= z["quantiles"][..., 2])
    assert np.all(z["quantiles"] >= 0.0) and np.all(z["quantiles"] <= 1.0)
    before = float(np.nanmax(smp.diagnostics("Z", first_slot=first, n_slots=S)["rhat"]))
    print(f"largest R-hat of Z: {before:.3f} as labelled, {float(np.nanmax(z['rhat'])):.3f} aligned; modal_share {a['modal_share']}")


def test_cluster_mean_bands_against_numpy(func):
    smp, a, first, S = func["smp"], func["a"], func["first"], func["S"]
    E = _basis_rows(smp, 21)
    got, v, B = _check_cluster_bands(smp, func["chains"], E, a["perm"], first, S, label="functional")
    assert np.array_equal(got["probs"], np.asarray(PROBS))
    # a single chain with the identity: bfmmm_post_bands on the same coefficient table
    from bayesfmmm_amd import api
    one = _k_sampler(3, 40, 12, 1)
    ch = _chain_copies(one, ["nu"])
    E1 = _basis_rows(one, 7)
    ident = _identity(one, 10)
    g1, v1, B1 = _check_cluster_bands(one, ch, E1, ident, 2, 10, label="one chain, identity")
    lib = api._lib_entry()
    dp = api.c_double_p
    for k in range(3):
        coef = np.ascontiguousarray(ch[0]["nu"][k, :, 2:12].T)      # (T, P)
        up, mid, lo = np.zeros(7), np.zeros(7), np.zeros(7)
        api._check(lib.bfmmm_post_bands(coef.ctypes.data_as(dp), 10, one.P, E1.ctypes.data_as(dp), 7, 0.05, 0, 0, up.ctypes.data_as(dp),
                                        mid.ctypes.data_as(dp), lo.ctypes.data_as(dp), None))
        ref = np.stack([lo, mid, up], axis=-1)
        assert np.all(np.abs(g1["quantiles"][k] - ref) <= B1[k][:, None] + 2 * U * np.abs(ref)), k
    one.close()


def test_determinism_and_budgets(small):
    from bayesfmmm_amd import _lib
    smp, a, first, S = small["smp"], small["a"], small["first"], small["S"]
    again = smp.align(first_slot=first, n_slots=S)
    assert again["perm"].tobytes() == a["perm"].tobytes() and again["score"].tobytes() == a["score"].tobytes()
    N, K, P = 2 * S, 3, smp.P
    E = _basis_rows(smp, 4)
    full = smp.aligned_summary("nu", a["perm"], first_slot=first, n_slots=S)
    assert smp.timing("align_gather")[1] == 1
    bands = smp.cluster_mean_bands(E, a["perm"], first_slot=first, n_slots=S)
    assert smp.timing("align_project")[1] == 1
    row_s, row_b = 8 * (N + 7 + 3), 8 * (N + 2 + 3)      # a gathered row with its seven statistics and three quantiles; a row of values
    for per_chunk in (1, 2, 4):
        s = smp.aligned_summary("nu", a["perm"], first_slot=first, n_slots=S, max_workspace_bytes=per_chunk * row_s + 7)
        for k in STATS + ("quantiles",):
            assert s[k].tobytes() == full[k].tobytes(), (per_chunk, k)
        assert smp.timing("align_gather")[1] == -(-K * P // per_chunk) and smp.timing("align_gather")[0] > 0.0
        m = smp.cluster_mean_bands(E, a["perm"], first_slot=first, n_slots=S, max_workspace_bytes=per_chunk * row_b + 7)
        for k in ("mean", "sd", "quantiles"):
            assert m[k].tobytes() == bands[k].tobytes(), (per_chunk, k)
        assert smp.timing("align_project")[1] == -(-K * 4 // per_chunk) and smp.timing("align_project")[0] > 0.0
    with pytest.raises(_lib.BfmmmError, match=f"'max_workspace_bytes' below the {row_s} bytes of one row"):
        smp.aligned_summary("nu", a["perm"], first_slot=first, n_slots=S, max_workspace_bytes=row_s - 1)
    with pytest.raises(_lib.BfmmmError, match=f"'max_workspace_bytes' below the {row_b} bytes of one row"):
        smp.cluster_mean_bands(E, a["perm"], first_slot=first, n_slots=S, max_workspace_bytes=row_b - 1)


def test_rows_longer_than_8192_draws():
    """2 chains x 4100 slots of a small multivariate model: the global tier of the diagnostics and the global sort"""
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(6)
    n, P, K, T = 12, 3, 2, 4100
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=2)
    for q in range(2):
        smp.select_chain(q)
        smp.init_state(1, 21, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=21)
    chains = _chain_copies(smp, ["Z", "nu", "pi"])
    a = smp.align(pivot=(0, T - 1))
    _check_align(a, [ch["Z"] for ch in chains], a["pivot"]["Z"], 0, T, "8200 draws", max_undecidable=0.05)
    _check_summary_against_host(smp, chains, "pi", a["perm"], 0, T)
    _check_cluster_bands(smp, chains, np.eye(P), a["perm"], 0, T, label="8200 draws")
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
    chains = _chain_copies(smp, ["Z", "nu"])
    a = smp.align(first_slot=first)
    _check_align(a, [ch["Z"] for ch in chains], a["pivot"]["Z"], first, T - first, "multivariate", max_undecidable=0.05)
    _check_summary_against_host(smp, chains, "Z", a["perm"], first, T - first)
    _check_cluster_bands(smp, chains, np.eye(P), a["perm"], first, T - first, label="multivariate")
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
    before = _chain_copies(a, STATE)
    r = a.align(first_slot=1, n_slots=6)
    a.aligned_summary("Z", r["perm"], first_slot=1, n_slots=6)
    a.aligned_summary("tau", r["perm"], first_slot=1, n_slots=6)
    a.cluster_mean_bands(_basis_rows(a, 5), r["perm"], first_slot=1, n_slots=6)
    after = _chain_copies(a, STATE)
    for q in range(NCH):
        for nm in STATE:
            assert before[q][nm].tobytes() == after[q][nm].tobytes(), (q, nm)
    for smp in pair:
        smp.select_chain(0)
        smp.run(bf.SWEEP_WARM, 3, first_iter=7, seed=3)
    sa, sb = _chain_copies(a, STATE), _chain_copies(b, STATE)
    for q in range(NCH):
        for nm in STATE:
            assert sa[q][nm].tobytes() == sb[q][nm].tobytes(), (q, nm)
    a.close()
    b.close()


def test_refusals(small):
    from bayesfmmm_amd import _lib
    smp, a = small["smp"], small["a"]
    lib, T, NCH, K, n = smp.lib, smp.T, smp.n_chains, smp.K, smp.n
    dp = _lib.c_double_p
    S = 8
    N = NCH * S
    Zref = np.asfortranarray(a["pivot"]["Z"])
    perm = np.ascontiguousarray(_identity(smp, S))
    score, probs = np.zeros(NCH * T), np.array([0.1, 0.9])
    out = [np.zeros(n * K) for _ in range(7)]
    quant = np.zeros(n * K * 2)
    E = _basis_rows(smp, 4)
    pz, pp, ps, pq, pr, pe = Zref.ctypes.data_as(dp), perm.ctypes.data_as(IP), score.ctypes.data_as(dp), quant.ctypes.data_as(dp), \
        probs.ctypes.data_as(dp), E.ctypes.data_as(dp)
    po = [o.ctypes.data_as(dp) for o in out]
    big = np.zeros(NCH * T * K, dtype=np.int32)
    pb = big.ctypes.data_as(IP)

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    # ---- bfmmm_chain_align ----
    al = lib.bfmmm_chain_align
    msg = err(al(None, pz, 0, S, pb, ps, N * K))
    assert "bfmmm_chain_align" in msg and "'h' is null" in msg
    assert "'Zref' is null" in err(al(smp.h, None, 0, S, pb, ps, N * K))
    assert "'perm' is null" in err(al(smp.h, pz, 0, S, None, ps, N * K))
    assert "'first_slot' out of range" in err(al(smp.h, pz, T, 1, pb, ps, N * K))
    assert "'first_slot' out of range" in err(al(smp.h, pz, -1, 1, pb, ps, N * K))
    assert "'n_slots' out of range" in err(al(smp.h, pz, 2, T - 1, pb, ps, NCH * T * K))
    assert "'n_slots' out of range" in err(al(smp.h, pz, 0, 0, pb, ps, N * K))
    assert f"'capacity' below {N * K} entries" in err(al(smp.h, pz, 0, S, pb, ps, N * K - 1))
    bad = Zref.copy(order="F")
    bad[5, 1] = np.nan
    assert "'Zref'[5, 1] is not finite" in err(al(smp.h, bad.ctypes.data_as(dp), 0, S, pb, ps, N * K))
    bad[5, 1] = np.inf
    assert "is not finite" in err(al(smp.h, bad.ctypes.data_as(dp), 0, S, pb, ps, N * K))
    assert al(smp.h, pz, 0, S, pb, None, N * K) == 0      # the score is optional
    with pytest.raises(ValueError, match="pivot"):
        smp.align(pivot=np.zeros((n, K + 1)))

    # ---- bfmmm_chain_aligned_summary ----
    def summ(h=smp.h, name=b"Z", p=pp, first=0, slots=S, pr_=pr, nq=2, budget=0, o=None, q=pq, cap=n * K):
        o = po if o is None else o
        return lib.bfmmm_chain_aligned_summary(h, name, p, first, slots, pr_, nq, budget, *o, q, cap)

    msg = err(summ(h=None))
    assert "bfmmm_chain_aligned_summary" in msg and "'h' is null" in msg
    assert "'name' is null" in err(summ(name=None))
    assert "'perm' is null" in err(summ(p=None))
    for j, k in enumerate(STATS):
        assert f"'{k}' is null" in err(summ(o=po[:j] + [None] + po[j + 1:]))
    assert "'probs' is null" in err(summ(pr_=None))
    assert "'quant' is null" in err(summ(q=None))
    assert summ(pr_=None, nq=0, q=None) == 0
    assert "'first_slot' out of range" in err(summ(first=T))
    assert "'n_slots' out of range" in err(summ(first=T - 2, slots=3))
    assert "'max_workspace_bytes' must not be negative" in err(summ(budget=-1))
    row = 8 * (N + 7 + 2)
    assert f"'max_workspace_bytes' below the {row} bytes of one row" in err(summ(budget=row - 1))
    assert f"bfmmm_chain_aligned_summary(Z): 'capacity' below {n * K} entries" in err(summ(cap=n * K - 1))
    assert "unknown name 'nope'" in err(summ(name=b"nope"))
    assert "unknown name 'eta'" in err(summ(name=b"eta"))      # no covariates were set
    assert "'nq' outside 0 .. 16" in err(summ(nq=17))
    for v in (-0.1, 1.5, np.nan):
        pbad = np.array([0.5, v])
        assert "'probs'[1] outside [0, 1]" in err(summ(pr_=pbad.ctypes.data_as(dp)))
    for row_, vals in (((1, 3), [0, 0, 1]), ((0, 5), [0, 1, 3]), ((1, 0), [-1, 1, 2])):
        p2 = perm.copy()
        p2[row_] = vals
        assert f"'perm' of chain {row_[0]}, slot {row_[1]} is not a permutation of 0 .. {K - 1}" in err(summ(p=p2.ctypes.data_as(IP)))
    p2 = perm.copy()
    p2[1, 2] = [0, 1, 1]
    assert "'perm' of chain 1, slot 6 is not a permutation" in err(summ(p=p2.ctypes.data_as(IP), first=4, slots=S))
    with pytest.raises(ValueError, match="perm must have shape"):
        smp.aligned_summary("Z", perm[:, :3])

    # ---- bfmmm_chain_cluster_mean_bands ----
    mean, sd, q3 = np.zeros(K * 4), np.zeros(K * 4), np.zeros(K * 4 * 2)
    pm, psd, pq3 = mean.ctypes.data_as(dp), sd.ctypes.data_as(dp), q3.ctypes.data_as(dp)

    def bands(h=smp.h, p=pp, e=pe, G=4, first=0, slots=S, pr_=pr, nq=2, budget=0, m=pm, s=psd, q=pq3, cap=K * 4):
        return lib.bfmmm_chain_cluster_mean_bands(h, p, e, G, first, slots, pr_, nq, budget, m, s, q, cap)

    msg = err(bands(h=None))
    assert "bfmmm_chain_cluster_mean_bands" in msg and "'h' is null" in msg
    assert "'perm' is null" in err(bands(p=None))
    assert "'E' is null" in err(bands(e=None))
    assert "'mean' is null" in err(bands(m=None))
    assert "'sd' is null" in err(bands(s=None))
    assert "'probs' is null" in err(bands(pr_=None))
    assert "'quant' is null" in err(bands(q=None))
    assert "'G' must be at least 1" in err(bands(G=0))
    assert "'first_slot' out of range" in err(bands(first=-1))
    assert "'n_slots' out of range" in err(bands(slots=T + 1))
    assert "'max_workspace_bytes' must not be negative" in err(bands(budget=-5))
    assert f"'max_workspace_bytes' below the {8 * (N + 2 + 2)} bytes of one row" in err(bands(budget=8 * (N + 2 + 2) - 1))
    assert f"'capacity' below {K * 4} rows" in err(bands(cap=K * 4 - 1))
    pbad = np.array([2.0, 0.5])
    assert "'probs'[0] outside [0, 1]" in err(bands(pr_=pbad.ctypes.data_as(dp)))
    p2 = perm.copy()
    p2[0, 7] = [2, 2, 0]
    assert "'perm' of chain 0, slot 7 is not a permutation of 0 .. 2" in err(bands(p=p2.ctypes.data_as(IP)))
    assert bands() == 0 and np.all(np.isfinite(mean)) and np.all(sd > 0)
    with pytest.raises(ValueError, match="E must be a G x"):
        smp.cluster_mean_bands(np.zeros((3, smp.P + 1)), perm, n_slots=S)


def test_draw_count_bound():
    """2^22 draws a row at most: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    dp = _lib.c_double_p
    Zref, one = np.full((2, 2), 0.5, order="F"), np.zeros(8)
    p1 = one.ctypes.data_as(dp)
    dummy = np.zeros(4, dtype=np.int32)      # never read: the row limit is checked before perm
    for rc in (smp.lib.bfmmm_chain_align(smp.h, Zref.ctypes.data_as(dp), 0, T, dummy.ctypes.data_as(IP), None, 1 << 40),
               smp.lib.bfmmm_chain_aligned_summary(smp.h, b"pi", dummy.ctypes.data_as(IP), 0, T, None, 0, 0, *([p1] * 7), None, 2),
               smp.lib.bfmmm_chain_cluster_mean_bands(smp.h, dummy.ctypes.data_as(IP), p1, 1, 0, T, None, 0, 0, p1, p1, None, 2)):
        assert rc != 0 and "2^22" in smp.lib.bfmmm_last_error().decode()
    smp.close()


def test_timers(small):
    smp, a, first, S = small["smp"], small["a"], small["first"], small["S"]
    smp.align(first_slot=first, n_slots=S)
    smp.aligned_summary("Z", a["perm"], first_slot=first, n_slots=S)
    smp.cluster_mean_bands(_basis_rows(smp, 3), a["perm"], first_slot=first, n_slots=S)
    for nm in ("align_gram", "align_gather", "align_project"):
        ms, launches = smp.timing(nm)
        assert ms > 0.0 and launches == 1, nm


def test_sampled_labels():
    """chains started from the truth with permuted labels (sigma^2 = 0.01), SWEEP_WARM, T = 30: the device's perm is the
    restatement's; modal_share and the largest R-hat of Z before and after alignment are printed, not asserted"""
    import bayesfmmm_amd as bf
    from gpu_parity import STATE_NAMES, oracle_slot
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=41, ragged=True)
    T, NCH = 30, 3
    perms = ([0, 1, 2], [2, 0, 1], [1, 0, 2])
    model, ch = truth_chain(sim, 2)
    truth = {nm: oracle_slot(ch, nm, 0) for nm in STATE_NAMES}
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        st = dict(truth)
        for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
            st[nm] = np.asarray(truth[nm])[perms[q]]
        st["Z"] = np.asarray(truth["Z"])[:, perms[q]]
        smp.select_chain(q)
        smp.set_state(**st)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=7)
    z = [c["Z"] for c in _chain_copies(smp, ["Z"])]
    a = smp.align(pivot=np.asfortranarray(sim["Z"]))
    _check_align(a, z, sim["Z"], 0, T, "sampled from permuted truth", max_undecidable=0.05)
    before = smp.diagnostics("Z")["rhat"]
    after = smp.aligned_summary("Z", a["perm"])["rhat"]
    print(f"chain_perm {a['chain_perm'].tolist()} (planted {list(perms)}), modal_share {a['modal_share']}; "
          f"largest R-hat of Z {float(np.nanmax(before)):.3f} as labelled, {float(np.nanmax(after)):.3f} aligned")
    smp.close()
