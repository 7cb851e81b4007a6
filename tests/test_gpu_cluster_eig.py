"""Cluster eigenvalues and eigenfunctions from aligned chain slots on the device (kernels_cluster_eig.hip):
Sampler.cluster_eigen against the numpy restatement (tests/cluster_eig_ref.py) fed the get_chain copies.

Every draw's eigenvalues (`values_trace`) are held entry by entry to |device - long double| <= ||bound_S||_F + C_J 2^-53 ||S||_F,
the eigenfunctions (`functions_trace`) to the residual, orthonormality, sign and exact-zero conditions of the restatement's module
docstring, with the constants fixed there from its own float64 run.  The call does not return the total and the share of variance
draw by draw: they are held through the sum of the eigenvalue trace (within the eigenvalue and total bounds), through their mean
(within the mean of the per-draw bounds plus the summation's rounding) and through their smallest and largest values (quantiles 0
and 1, within the largest per-draw bound: order statistics move no further than the entries do), and entry by entry where a call
has two draws.  The sum of the eigenvalues is also held to sum_g w_g of cluster_cov_bands' variance function, an independent
kernel.  The reductions are held to the returned traces: quantiles byte for byte bfmmm_post_col_quantiles, the seven statistics of
the eigenvalues byte for byte api.diagnostics, mean and sd within tests/test_gpu_align.py's bounds over equal values.  Then what
the layout promises bit for bit, the refusals, untouched state, the sweep counts and the timers.  The samplers are tiny and run
a handful of sweeps; nothing here depends on convergence.  The non-convergence error is not provoked on the device."""
import re

import numpy as np
import pytest

import cluster_cov_ref as CR
import cluster_eig_ref as R
import curve_fit_ref as FR
from simdata import simulate_functional
from test_gpu_chain_batch import make_sampler_batch
from test_gpu_cluster_cov import STATE, _col_quantiles, _random_perm
from test_gpu_curve_cov import _chains, _rows_of_basis, func      # noqa: F401 (func: the module fixture, one sampler per module)
from tiny_sampler import make_tiny

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
LD = np.longdouble
VAL_KEYS = ("mean", "sd", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "quantiles")


def _weights(G, kind, seed=1):
    if kind is None:
        return None
    w = np.random.default_rng(seed).uniform(0.1, 2.0, G)
    if kind == "zero" and G > 1:
        w[G // 2] = 0.0
    return w


def _check(smp, chains, E, perm, first, S, label, w=None, J=None, ref=None, x=None, **kw):
    """one call with trace=True against the restatement, component by component; returns the result and the worst ratios"""
    got = smp.cluster_eigen(E, perm, weights=w, n_functions=J, x=x, ref=ref, probs=(0.0, 0.5, 1.0), trace=True, first_slot=first,
                            n_slots=S, **kw)
    K, M, G = smp.K, smp.M, E.shape[0]
    Jn = M if J is None else J
    N = smp.n_chains * S
    assert got["values_trace"].shape == (K, M, N) and got["functions_trace"].shape == (K, Jn, G, N)
    assert got["functions"]["mean"].shape == (K, Jn, G) and got["functions"]["quantiles"].shape == (K, Jn, G, 3)
    assert got["values"]["mean"].shape == (K, M) and got["pve"]["quantiles"].shape == (K, M, 3) and got["total"]["quantiles"].shape == (K, 3)
    Th = R.thetas(chains, perm, first, S, x)                         # (K, N, P, M)
    D = 0 if x is None else len(x)
    refs = got["ref"]
    assert (refs is None) == (ref is None or Jn == 0) or isinstance(ref, str)
    worst, sweeps64 = {}, 0
    vt = got["values_trace"]
    assert np.all(vt >= 0) and np.all(np.diff(vt, axis=1) <= 0), label                 # descending, clamped
    for k in range(K):
        lam = np.ascontiguousarray(vt[k].T)
        dev = dict(lam=lam, total=np.sum(lam.astype(LD), axis=1), pve=lam, psi=np.transpose(got["functions_trace"][k], (2, 0, 1)))
        rk = None if refs is None else refs[k]
        out, exact_zero, ld = R.check(dev, Th[k], E, w, rk, D, ref_rule="largest" if rk is None else None)
        del out["total"], out["pve"]                                 # not returned draw by draw: below
        assert exact_zero, (label, k)
        for name, v in out.items():
            worst[name] = max(worst.get(name, 0.0), v)
        sweeps64 = max(sweeps64, int(R.solve(Th[k], E, w, rk, 0, np.float64)["sweeps"].max()))
        # total and pve through their mean, smallest and largest values
        bS, A = R.bound_S(Th[k], E, w, D)
        nS = np.sqrt(np.sum(ld["S"] ** 2, axis=(1, 2)))
        b_lam = np.sqrt(np.sum(bS * bS, axis=(1, 2))) + LD(R.C_J * R.U) * nS
        b_tot = np.einsum("bii->b", bS) + LD(M * U52) * np.einsum("bii->b", A)
        den = ld["total"] - b_tot
        assert np.all(den > 0), label
        b_pve = (b_lam[:, None] + ld["pve"] * b_tot[:, None]) / den[:, None] + LD(U52) * ld["pve"]
        for key, val, bnd in (("total", ld["total"][None, :], b_tot[None, :]), ("pve", ld["pve"].T, b_pve.T)):
            g = got[key]
            gm = g["mean"][k].reshape(-1)
            gq = g["quantiles"][k].reshape(-1, 3)
            em = np.abs(gm - np.mean(val, axis=1))
            tm = np.mean(bnd, axis=1) + N * U52 * np.mean(np.abs(val), axis=1)
            elo, ehi = np.abs(gq[:, 0] - val.min(axis=1)), np.abs(gq[:, 2] - val.max(axis=1))
            tq = bnd.max(axis=1) + U52 * np.abs(val).max(axis=1)
            r = float(max(np.max(em / tm), np.max(elo / tq), np.max(ehi / tq)))
            worst[key] = max(worst.get(key, 0.0), r)
            if N == 2:                                               # two draws: the two order statistics are the entries
                so = np.sort(val, axis=1)
                assert np.all(np.abs(gq[:, 0] - so[:, 0]) <= tq) and np.all(np.abs(gq[:, 2] - so[:, 1]) <= tq), (label, key)
    print(f"{label}: K={K} M={M} J={Jn} G={G} N={N}: worst ratios " + ", ".join(f"{a} {b:.3g}" for a, b in sorted(worst.items())) +
          f"; sweeps device {got['max_sweeps']}, float64 restatement {sweeps64}")
    bad = {a: b for a, b in worst.items() if not a.endswith("_units") and not b <= 1.0}
    assert not bad, (label, bad)
    assert got["max_sweeps"] <= sweeps64 + 2 and got["max_sweeps"] < R.CAP, label
    return got


def _check_reductions(got, smp, S, label):
    """quantiles byte for byte from the returned traces, the seven statistics of lambda byte for byte api.diagnostics of its rows,
    mean and sd of the functions within the bounds over equal values"""
    from bayesfmmm_amd import api
    vt, ft = got["values_trace"], got["functions_trace"]
    K, M, N = vt.shape
    pr = got["probs"]
    assert got["values"]["quantiles"].tobytes() == _col_quantiles(vt.reshape(-1, N), pr).tobytes(), label
    if S >= 4:                                                       # shorter chains: only the layout of the NaNs could be compared
        stats = api.diagnostics(np.ascontiguousarray(vt.reshape(K * M, smp.n_chains, S).transpose(2, 1, 0)))
        for name in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd"):
            assert np.ascontiguousarray(got["values"][name]).reshape(-1).tobytes() == np.ascontiguousarray(stats[name]).reshape(-1).tobytes(), (label, name)
    else:
        mean, sd = FR.moments(vt)
        assert np.all(np.abs(got["values"]["mean"] - mean) <= N * U52 * np.mean(np.abs(vt), axis=-1)), (label, "values mean")
        assert np.all(np.isnan(got["values"]["sd"])) if N == 1 else np.all(np.abs(got["values"]["sd"] - sd) <= 4 * N * U52 * sd), label
    if ft.size:
        assert got["functions"]["quantiles"].tobytes() == _col_quantiles(ft.reshape(-1, N), pr).tobytes(), label
        mean, sd = FR.moments(ft)
        em, tm = np.abs(got["functions"]["mean"] - mean), N * U52 * np.mean(np.abs(ft), axis=-1)
        assert np.all(em <= tm), (label, "mean")
        if N > 1:
            assert np.all(np.abs(got["functions"]["sd"] - sd) <= 4 * N * U52 * sd), (label, "sd")
        else:
            assert np.all(np.isnan(got["functions"]["sd"])), label
    if N == 1:
        assert np.all(np.isnan(got["pve"]["sd"])) and np.all(np.isnan(got["total"]["sd"])), label


def _same(a, b, groups=("values", "pve", "total", "functions"), traces=True):
    for grp in groups:
        for k in a[grp]:
            assert np.ascontiguousarray(a[grp][k]).tobytes() == np.ascontiguousarray(b[grp][k]).tobytes(), (grp, k)
    if traces:
        for k in ("values_trace", "functions_trace"):
            if k in a and k in b and ("functions" in groups or k == "values_trace"):
                assert a[k].tobytes() == b[k].tobytes(), k
    assert a["max_sweeps"] == b["max_sweeps"]


# ---- (a) K = 3, M = 2, 4 chains x 23 slots ------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("G,J,wkind,refkind", [(1, 2, None, "array"), (7, 1, "random", None), (16, 2, "zero", "mean"), (17, 0, None, "mean"),
                                               (65, 2, "random", "array"), (17, 2, None, None)])
def test_func_against_restatement(func, G, J, wkind, refkind, aligned):
    smp, first, S = func["smp"], func["first"], func["S"]
    assert (smp.K, smp.M, smp.n_chains, S) == (3, 2, 4, 23)          # 276 problems: no multiple of a workgroup's 2 or 4
    perm = smp.align(first_slot=first, n_slots=S)["perm"] if aligned else _random_perm(smp, S, 200 + G)
    E = np.ascontiguousarray(func["E"][:G])
    w = _weights(G, wkind)
    ref = {"array": np.random.default_rng(G).standard_normal((3, J, G)), None: None, "mean": "mean"}[refkind]
    label = f"(a) G={G} J={J} w={wkind} ref={refkind} aligned={aligned}"
    got = _check(smp, func["chains"], E, perm, first, S, label, w=w, J=J, ref=ref)
    _check_reductions(got, smp, S, label)
    if refkind == "mean" and J > 0:
        # the default reference: w-orthonormal eigenfunctions of the mean surface, largest entry positive
        r = got["ref"]
        ww = np.ones(G) if w is None else w
        gram = np.einsum("g,kig,kjg->kij", ww, r, r)
        assert np.all(np.abs(gram - np.eye(J)) <= 1e-12)
        gi = np.argmax(np.sqrt(ww) * np.abs(r), axis=-1)
        assert np.all(np.take_along_axis(r, gi[..., None], axis=-1) > 0)


def test_sum_of_eigenvalues_is_the_weighted_variance_function(func):
    """through k_ccov_values: sum_j lambda_kj = sum_g w_g C^(k,k)(g, g), within the sum of both bounds"""
    smp, first, S = func["smp"], func["first"], func["S"]
    perm = smp.align(first_slot=first, n_slots=S)["perm"]
    E = np.ascontiguousarray(func["E"][:17])
    w = _weights(17, "zero")
    pairs = [(k, k) for k in range(3)]
    cov = smp.cluster_cov_bands(E, perm, pairs=pairs, diagonal=True, trace=True, first_slot=first, n_slots=S)["trace"]      # (3, 17, N)
    b_cov = CR.bound(func["chains"], perm, E, None, first, S, pairs, None, True)
    got = smp.cluster_eigen(E, perm, weights=w, n_functions=0, trace=True, first_slot=first, n_slots=S)
    Th = R.thetas(func["chains"], perm, first, S)
    for k in range(3):
        lhs = np.sum(got["values_trace"][k].astype(LD), axis=0)
        rhs = np.einsum("g,gn->n", w.astype(LD), cov[k].astype(LD))
        bS, A = R.bound_S(Th[k], E, w, 0)
        S_ld = R.form_S(R.gram(E, w, LD), Th[k].astype(LD))
        nS = np.sqrt(np.sum(S_ld ** 2, axis=(1, 2)))
        b_lam = np.sqrt(np.sum(bS * bS, axis=(1, 2))) + LD(R.C_J * R.U) * nS
        bound = smp.M * b_lam + np.einsum("g,gn->n", w, b_cov[k])
        ratio = float(np.max(np.abs(lhs - rhs) / bound))
        print(f"component {k}: worst |sum lambda - sum w C(g, g)| / bound = {ratio:.3e}")
        assert ratio <= 1.0


# ---- (b) odd M, M = 1, P not a multiple of 4 ----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[5, 1], ids=["M5", "M1"])
def small(request):
    """functional, n = 24, K = 2, P = 5 (one internal knot), 2 chains, T = 8; slots 2 .. 7 are 12 draws"""
    import bayesfmmm_amd as bf
    M = request.param
    sim = simulate_functional(n=24, M=M, sigma_sq=0.01, seed=41, K=2)
    sim["internal_knots"] = np.array([495.0])
    T, NCH = 8, 2
    smp = make_sampler_batch(sim, T, NCH)
    assert (smp.K, smp.M, smp.P) == (2, M, 5)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 11, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=3)
    yield dict(smp=smp, chains=_chains(smp), first=2, S=T - 2, E=_rows_of_basis(smp, 17))
    smp.close()


@pytest.mark.parametrize("G,Jkind,wkind,refkind", [(7, "M", "random", "array"), (17, "M", "zero", None), (16, "1", None, "mean"), (1, "M", None, None)])
def test_small_against_restatement(small, G, Jkind, wkind, refkind):
    smp, first, S = small["smp"], small["first"], small["S"]
    J = smp.M if Jkind == "M" else 1
    E = np.ascontiguousarray(small["E"][:G])
    ref = {"array": np.random.default_rng(G).standard_normal((2, J, G)), None: None, "mean": "mean"}[refkind]
    for aligned in (True, False):
        perm = smp.align(first_slot=first, n_slots=S)["perm"] if aligned else _random_perm(smp, S, 300 + G)
        label = f"(b) M={smp.M} G={G} J={J} w={wkind} ref={refkind} aligned={aligned}"
        got = _check(smp, small["chains"], E, perm, first, S, label, w=_weights(G, wkind), J=J, ref=ref)
        _check_reductions(got, smp, S, label)
        if smp.M == 1:
            assert got["max_sweeps"] == 1 and np.all(got["pve"]["mean"] == 1.0)           # no rotation at all


@pytest.mark.parametrize("form", [1, 2], ids=["fma", "mfma"])
def test_small_both_forms_of_S(small, form):
    """the plain and the MFMA form of S_k, each set explicitly, at P = 5 (padded to one 16-row tile, two steps of four) and odd M"""
    smp, first, S = small["smp"], small["first"], small["S"]
    E = np.ascontiguousarray(small["E"][:17])
    perm = _random_perm(smp, S, 77)
    smp.lib.bfmmm_set_cluster_eig_form(form)
    try:
        got = _check(smp, small["chains"], E, perm, first, S, f"(b) M={smp.M} form={form}", w=_weights(17, "zero"), ref=None)
        again = smp.cluster_eigen(E, perm, weights=_weights(17, "zero"), ref=None, probs=(0.0, 0.5, 1.0), trace=True, first_slot=first, n_slots=S)
        _same(got, again)
    finally:
        smp.lib.bfmmm_set_cluster_eig_form(0)


# ---- (c) the limits: P = 64, M = 16, multivariate -----------------------------------------------------------------------------
def test_limits_multivariate_identity():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T, NCH, first = 30, 64, 2, 16, 7, 2, 2
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((n, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    S = T - first
    chains = _chains(smp)
    E = np.eye(P)
    for aligned, J, ref in ((True, M, "mean"), (False, 1, None), (True, M, np.random.default_rng(9).standard_normal((K, M, P)))):
        perm = smp.align(first_slot=first)["perm"] if aligned else _random_perm(smp, S, 400)
        label = f"(c) P=64 M=16 J={J} aligned={aligned}"
        got = _check(smp, chains, E, perm, first, S, label, J=J, ref=ref)
        _check_reductions(got, smp, S, label)
    # the full MFMA tile and the plain form, each set explicitly
    for form in (1, 2):
        smp.lib.bfmmm_set_cluster_eig_form(form)
        try:
            _check(smp, chains, E, perm, first, S, f"(c) P=64 M=16 form={form}", J=M, ref=ref)
        finally:
            smp.lib.bfmmm_set_cluster_eig_form(0)
    # 65 rows: more than one tile of k_ceig_values' 16 rows at the widest P, weights with a zero
    E65 = np.ascontiguousarray(np.vstack([np.eye(P), rng.standard_normal((1, P))]))
    _check(smp, chains, E65, perm, first, S, "(c) G=65", w=_weights(65, "zero"), J=2, ref=None)
    smp.close()


# ---- (d) covariates -----------------------------------------------------------------------------------------------------------
def test_covariate_setting():
    from bayesfmmm_amd import _lib
    smp = make_tiny(D=2, covariance_adj=True, run=True)
    first, S = 1, smp.T - 1
    chains = _chains(smp, cov=True)
    E = _rows_of_basis(smp, 7)
    x = np.array([0.7, -1.3])
    w = _weights(7, "random")
    for aligned in (True, False):
        perm = smp.align(first_slot=first)["perm"] if aligned else _random_perm(smp, S, 500)
        got = _check(smp, chains, E, perm, first, S, f"(d) x = (0.7, -1.3) aligned={aligned}", w=w, x=x, ref="mean")
        _check_reductions(got, smp, S, "(d)")
        none = _check(smp, chains, E, perm, first, S, "(d) no x", w=w, ref="mean")
        assert np.any(got["values_trace"] != none["values_trace"])
        zero = smp.cluster_eigen(E, perm, weights=w, x=np.zeros(2), ref=none["ref"], trace=True, first_slot=first)
        assert zero["values_trace"].tobytes() == none["values_trace"].tobytes()
    # one slot of two chains: two draws, where the two order statistics are the entries; then one chain's worth is N = 2 still
    p1 = smp.align(first_slot=2, n_slots=1)["perm"]
    _check(smp, chains, E, p1, 2, 1, "(d) two draws", w=w, x=x, ref=None)
    smp.close()
    plain = make_tiny(D=2, covariance_adj=False, run=True)
    perm = np.tile(np.arange(plain.K, dtype=np.int32), (plain.n_chains, plain.T - 1, 1))
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_cluster_eigen: 'x' is given but the sampler is not covariance-adjusted"):
        plain.cluster_eigen(_rows_of_basis(plain, 5), perm, x=[0.7, -1.3], ref=None, first_slot=1)
    plain.close()


def test_one_draw_gives_nan_sd():
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=24, M=2, sigma_sq=0.01, seed=41, K=2)
    sim["internal_knots"] = np.array([495.0])
    smp = make_sampler_batch(sim, 3, 1)
    smp.init_state(1, 11, chain=0)
    smp.run(bf.SWEEP_WARM, 3, seed=3)
    E = _rows_of_basis(smp, 7)
    perm = np.tile(np.arange(2, dtype=np.int32), (1, 1, 1))
    got = _check(smp, _chains(smp), E, perm, 2, 1, "one draw", ref=None)
    _check_reductions(got, smp, 1, "one draw")
    assert np.all(np.isnan(got["values"]["sd"])) and np.all(np.isnan(got["functions"]["sd"]))
    assert got["values"]["mean"].tobytes() == np.ascontiguousarray(got["values_trace"][..., 0]).tobytes()
    smp.close()


# ---- bit properties -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(func):
    smp, first, S = func["smp"], func["first"], func["S"]
    perm = smp.align(first_slot=first, n_slots=S)["perm"]
    E = np.ascontiguousarray(func["E"][:17])
    w = _weights(17, "random")
    ref = np.random.default_rng(3).standard_normal((3, 2, 17))
    kw = dict(weights=w, ref=ref, trace=True, first_slot=first, n_slots=S)
    return dict(perm=perm, E=E, kw=kw, out=smp.cluster_eigen(E, perm, **kw))


def _budget_figures(smp, E, perm, **kw):
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'") as ei:
        smp.cluster_eigen(E, perm, max_workspace_bytes=1, **kw)
    msg = str(ei.value)
    shared, per_row = (int(v) for v in re.search(r"\((\d+) shared by all rows \+ (\d+) per row\)", msg).groups())
    assert msg.startswith("bfmmm_chain_cluster_eigen") and re.search(r"below the (\d+) bytes one row needs", msg).group(1) == str(shared + per_row)
    return shared, per_row


def test_chunks_repeatability_and_timers(func, full):
    from bayesfmmm_amd import _lib
    smp, perm, E, kw, one = func["smp"], full["perm"], full["E"], full["kw"], full["out"]
    _same(smp.cluster_eigen(E, perm, **kw), one)
    for t, n in (("cluster_eig_gram", 1), ("cluster_eig", 1), ("cluster_eig_values", 1)):
        ms, cnt = smp.timing(t)
        assert ms > 0 and cnt == n, t
    shared, per_row = _budget_figures(smp, E, perm, **kw)
    assert per_row == 8 * (92 + 2 + 3)
    for rows, chunks in ((51, 2), (34, 3), (7, 15), (1, 102)):                        # 3 x 2 x 17 = 102 rows
        got = smp.cluster_eigen(E, perm, max_workspace_bytes=shared + per_row * rows + 7, **kw)
        _same(got, one)
        assert smp.timing("cluster_eig_values")[1] == chunks and smp.timing("cluster_eig")[1] == 1 and smp.timing("cluster_eig_gram")[1] == 1
    with pytest.raises(_lib.BfmmmError, match=rf"below the {shared + per_row} bytes one row needs"):
        smp.cluster_eigen(E, perm, max_workspace_bytes=shared + per_row - 1, **kw)


def test_values_do_not_depend_on_the_functions(func, full):
    smp, perm, E, kw, one = func["smp"], full["perm"], full["E"], full["kw"], full["out"]
    small = ("values", "pve", "total")
    # n_functions, ref, trace, the grid's chunking
    j0 = smp.cluster_eigen(E, perm, **dict(kw, n_functions=0, ref=None))
    _same(j0, one, small)
    assert smp.timing("cluster_eig_values") == (0.0, 0) and smp.timing("cluster_eig")[1] == 1
    assert j0["functions"]["mean"].shape == (3, 0, 17) and j0["functions_trace"].shape == (3, 0, 17, 92)
    _same(smp.cluster_eigen(E, perm, **dict(kw, ref=None)), one, small)
    _same(smp.cluster_eigen(E, perm, **dict(kw, ref="mean")), one, small)
    nt = smp.cluster_eigen(E, perm, **dict(kw, trace=False))
    assert "values_trace" not in nt and "functions_trace" not in nt
    _same(nt, one, traces=False)
    # J < M: the first J functions of J = M
    j1 = smp.cluster_eigen(E, perm, **dict(kw, n_functions=1, ref=np.ascontiguousarray(kw["ref"][:, :1])))
    _same(j1, one, small)
    for k in ("mean", "sd", "quantiles"):
        assert j1["functions"][k].tobytes() == np.ascontiguousarray(one["functions"][k][:, :1]).tobytes(), k
    assert j1["functions_trace"].tobytes() == np.ascontiguousarray(one["functions_trace"][:, :1]).tobytes()
    # a constant permutation applied to every draw permutes the components of the result
    sigma = np.array([2, 0, 1])
    ps = smp.cluster_eigen(E, np.ascontiguousarray(perm[:, :, sigma]), **dict(kw, ref=np.ascontiguousarray(kw["ref"][sigma])))
    for grp in ("values", "pve", "total", "functions"):
        for k in one[grp]:
            assert np.ascontiguousarray(ps[grp][k]).tobytes() == np.ascontiguousarray(one[grp][k][sigma]).tobytes(), (grp, k)
    assert ps["values_trace"].tobytes() == np.ascontiguousarray(one["values_trace"][sigma]).tobytes()
    assert ps["functions_trace"].tobytes() == np.ascontiguousarray(one["functions_trace"][sigma]).tobytes()


def test_state_and_slots_untouched(func, full):
    smp, perm, E, kw = func["smp"], full["perm"], full["E"], full["kw"]

    def snap():
        out = []
        for q in range(smp.n_chains):
            smp.select_chain(q)
            out.append({nm: smp.get_chain(nm).tobytes() for nm in STATE})
            out.append({nm: smp.get_state(nm).tobytes() for nm in ("nu", "Phi", "Z", "pi", "sigma_sq")})
        smp.select_chain(0)
        return out
    before = snap()
    smp.cluster_eigen(E, perm, **dict(kw, ref="mean"))
    smp.cluster_eigen(E, perm, max_workspace_bytes=_budget_figures(smp, E, perm, **kw)[0] + 8 * 97 * 5, **kw)      # chunks of 5 rows
    assert snap() == before


def test_refusals(func, full):
    from bayesfmmm_amd import _lib
    smp, perm, E, kw = func["smp"], full["perm"], full["E"], full["kw"]
    fn = "bfmmm_chain_cluster_eigen: "
    bad = perm.copy()
    bad[1, 4] = (0, 0, 2)
    with pytest.raises(_lib.BfmmmError, match=re.escape(fn + "'perm' of chain 1, slot 11 is not a permutation of 0 .. 2")):
        smp.cluster_eigen(E, bad, **kw)
    w = kw["weights"].copy()
    w[3] = -1e-300
    with pytest.raises(_lib.BfmmmError, match=re.escape(fn + "'w'[3] is negative or not finite")):
        smp.cluster_eigen(E, perm, **dict(kw, weights=w))
    w[3] = np.nan
    with pytest.raises(_lib.BfmmmError, match=re.escape(fn + "'w'[3] is negative or not finite")):
        smp.cluster_eigen(E, perm, **dict(kw, weights=w, ref=None))
    with pytest.raises(_lib.BfmmmError, match=re.escape(fn + "'n_functions' = 3 outside 0 .. 2")):
        smp.cluster_eigen(E, perm, **dict(kw, n_functions=3, ref=None))
    with pytest.raises(_lib.BfmmmError, match=re.escape(fn + "'x' is given but the sampler is not covariance-adjusted")):
        smp.cluster_eigen(E, perm, **dict(kw, x=[1.0]))
    shared, per_row = _budget_figures(smp, E, perm, **kw)
    with pytest.raises(_lib.BfmmmError, match=rf"'max_workspace_bytes' below the {shared + per_row} bytes one row needs \({shared} shared"):
        smp.cluster_eigen(E, perm, max_workspace_bytes=shared, **kw)
