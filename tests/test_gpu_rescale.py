"""The reference's rescale step per draw on the device (kernels_rescale.hip, k_ccov_mix) against the long-double
restatement tests/rescale_ref.py fed the get_chain copies.  Slots are planted with set_state + run(U_LOGLIK), one run per slot.

curve and transform: byte for byte on every draw -- A is copied, and the smallest maximiser is decidable whatever the values.

Bound of the inverse, derived for the elimination used (Gauss-Jordan with partial pivoting on [A | I]; rescale_ref's docstring),
u = 2^-52: every entry of the device's X within b = 8 K^2 rho u kappa_1(A) |A^-1|_1 of the long-double inverse, rho the growth factor
of the restatement's own elimination of that A.  rcond =
1 / (|A|_1 |X|_1): |X|_1 is a sum of K entries, so it moves by at most K b; with the K roundings of either column sum, the product and
the division, |rcond - ref| <= rcond (K b / |A^-1|_1 + (2 K + 3) u).  z_min: Z~[i, k] = sum_c Z[i, c] X[c][k] moves by at most S1 b
where X does (S1 = max_i sum_c |Z[i, c]|) and by K u S1 max|X| through its own roundings; a minimum is 1-Lipschitz.

Mixed rows: an element is a sum of K products, device and long double within K u / 2 sum_c |w_c x_c| each way, b = K u sum_c |w_c x_c|;
mean bands: D + K + P products and as many sums, b = (P + K + D + 2) u a with a the same sum over absolute values (2: section 7g's
allowance); covariance values: tests/test_gpu_cluster_cov.py's constant with the K of the mixing pass in either table, b = (2 (P + D + K
+ 1) + M + 3) u a.  B = max b over a row's draws is carried through the order statistics (1-Lipschitz in the sup norm) as
tests/test_gpu_align.py's docstring derives for cluster_mean_bands: |quantile - numpy's| <= B + 2 u |q|, mean B + N u mean|v|, sd
sqrt(N / (N - 1)) B + 4 N u sd.  R-hat and the effective sample sizes rank the draws and are not Lipschitz: they are compared where the
rows are equal (permutation matrices), byte for byte.

K = 1 is not among the argmax cases: no sampler of one component can be built (bfmmm_create refuses K < 2); K = 2 .. 4 run the
instantiation it would share."""
import os
import re
import sys

import numpy as np
import pytest

import rescale_ref as R
import curve_fit_ref as FR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import post_ci as O      # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
PROBS = (0.025, 0.5, 0.975)
STATS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")
NAMES = ("nu", "Phi", "Z", "eta", "xi")


def _make(n, K, NCH, T, D=0, M=2, degree=2, n_internal=5):
    import bayesfmmm_amd as bf
    from test_gpu_shapes import simulate
    sim = simulate(n, K, M, degree, n_internal, seed=300 + 10 * K + n % 9)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=degree, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"], n_chains=NCH)
    if D:
        smp.set_covariates(np.random.default_rng(n + D).standard_normal((n, D)), covariance_adj=True)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 40 + K, chain=q)
    smp.select_chain(0)
    return smp


def _plant(smp, draws):
    """draws[q][t]: the arrays of chain q's slot t; one U_LOGLIK run per slot, so that the slots hold what was set"""
    import bayesfmmm_amd as bf
    T = len(draws[0])
    for t in range(T):
        for q in range(smp.n_chains):
            smp.select_chain(q)
            smp.set_state(**draws[q][t])
        smp.select_chain(0)
        smp.run(bf.sampler.U_LOGLIK, 1, first_iter=t, seed=1)
    chains = _copies(smp, list(draws[0][0]))
    for q in range(smp.n_chains):
        for t in range(T):
            for nm, v in draws[q][t].items():
                assert np.array_equal(chains[q][nm][..., t], v, equal_nan=True), (q, t, nm)
    return chains


def _copies(smp, names):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in names})
    smp.select_chain(0)
    return out


def _random_perm(C, S, K, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.permutation(K) for _ in range(S)]) for _ in range(C)]).astype(np.int32)


def _perm_matrices(perm):
    K = perm.shape[-1]
    return np.ascontiguousarray((perm[..., None] == np.arange(K)).astype(np.float64))      # [q, s, k, c] = 1 where c = perm[k]


def _check_rescale(r, chains, first, S, label, perm=None, given=None):
    """curve and transform byte for byte, inverse, rcond and z_min within their bounds, singular draws flagged; returns the restatement"""
    Cn, K = len(chains), chains[0]["Z"].shape[1]
    assert r["transform"].shape == (Cn, S, K, K) and r["inverse"].shape == (Cn, S, K, K)
    assert r["rcond"].shape == (Cn, S) and r["z_min"].shape == (Cn, S)
    assert (r["curve"] is None) if given is not None else (r["curve"].shape == (Cn, S, K) and r["curve"].dtype == np.int32)
    worst = {"inverse": 0.0, "rcond": 0.0, "z_min": 0.0}
    refs, n_sing = [], 0
    for q in range(Cn):
        refs.append([])
        for s in range(S):
            Z = chains[q]["Z"][:, :, first + s]
            d = R.draw(Z, None if perm is None else perm[q, s], None if given is None else given[q, s])
            refs[q].append(d)
            if given is None:
                assert np.array_equal(r["curve"][q, s], d["curve"]), (label, q, s, r["curve"][q, s], d["curve"])
            assert r["transform"][q, s].tobytes() == d["A"].tobytes(), (label, q, s)
            if d["singular"]:
                n_sing += 1
                assert np.all(np.isnan(r["inverse"][q, s])) and r["rcond"][q, s] == 0.0 and np.isnan(r["z_min"][q, s]), (label, q, s)
                continue
            Ai = np.asarray(d["Ainv"], dtype=np.float64)
            b = R.inverse_bound(d["A"], d["Ainv"])
            ni = float(R.norm1(d["Ainv"]))
            S1 = float(np.max(np.sum(np.abs(Z), axis=1)))
            bounds = {"inverse": b, "rcond": d["rcond"] * (K * b / ni + (2 * K + 3) * U),
                      "z_min": S1 * (b + K * U * (float(np.max(np.abs(Ai))) + b))}
            errs = {"inverse": float(np.max(np.abs(r["inverse"][q, s] - Ai))), "rcond": abs(r["rcond"][q, s] - d["rcond"]),
                    "z_min": abs(r["z_min"][q, s] - d["z_min"])}
            if np.isnan(d["z_min"]):          # a NaN membership outside the pure curves: kept, and the draw is not singular
                assert np.isnan(r["z_min"][q, s]), (label, q, s)
                errs["z_min"] = 0.0
            for k in worst:
                assert np.isfinite(errs[k]), (label, k, q, s)
                worst[k] = max(worst[k], errs[k] / bounds[k])
    rc = [d["rcond"] for row in refs for d in row if not d["singular"]]
    print(f"{label} K={K} draws={Cn * S}: {n_sing} singular, rcond {min(rc, default=0):.2e} .. {max(rc, default=0):.2e}, worst error / bound: "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert r["n_singular"] == n_sing, (label, r["n_singular"], n_sing)
    for k, v in worst.items():
        assert v <= 1.0, (label, k, v)
    return refs


def _check_rows(got, v, b, probs, label):
    """mean, sd and quantiles of rows v (..., N) whose device values are within b (..., N) of v"""
    N = v.shape[-1]
    v64, B = np.asarray(v, dtype=np.float64), np.asarray(b, dtype=np.float64).max(axis=-1)
    assert got["mean"].shape == v.shape[:-1] and got["quantiles"].shape == v.shape[:-1] + (len(probs),), (label, got["mean"].shape, v.shape)
    q = FR.quantiles(v64, probs)
    eq, tq = np.abs(got["quantiles"] - q), B[..., None] + 2 * U * np.abs(q)
    mean, sd = FR.moments(v64)
    em, tm = np.abs(got["mean"] - mean), B + N * U * np.mean(np.abs(v64), axis=-1)
    es, ts = np.abs(got["sd"] - sd), np.sqrt(N / (N - 1.0)) * B + 4 * N * U * sd
    pos = lambda e, t: float(np.max(e[t > 0] / t[t > 0])) if np.any(t > 0) else 0.0
    print(f"{label} N={N}: worst |quantile - numpy| / bound {pos(eq, tq):.3e}, mean {pos(em, tm):.3e}, sd {pos(es, ts):.3e}")
    assert np.all(eq <= tq) and np.all(em <= tm) and np.all(es <= ts), label


def _tied_Z(rng, n, K, q, t):
    """memberships below 0.96875 with that value planted twice or three times in one column: in the same thread's stride (curves 0
    and 256), in two lanes of a wave, in three waves"""
    Z = 0.9 * rng.dirichlet(np.full(K, 1.5), size=n) + 0.1 / K
    if K == 1:
        return Z                      # every curve ties
    top = 0.96875
    plan = {(0, 0): ((256, 0), 0), (0, 1): ((17, 3), min(1, K - 1)), (1, 0): ((5 + 128, 5 + 64, 5), K - 1), (1, 1): ((256 + 70, 70 + 64), 0)}
    if (q, t) in plan:
        rows, c = plan[(q, t)]
        for i in rows:
            if i < n:
                Z[i, :] = (1 - top) / (K - 1)
                Z[i, c] = top
    return Z


# ---- the transform of every draw ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(1, 3), (255, 3), (256, 3), (257, 3), (300, 3), (300, 2), (300, 4), (300, 5), (300, 8)])
def test_argmax_whatever_the_grid(n, K):
    NCH, T = 2, 3
    smp = _make(n, K, NCH, T)
    rng = np.random.default_rng(1000 * K + n)
    chains = _plant(smp, [[{"Z": _tied_Z(rng, n, K, q, t)} for t in range(T)] for q in range(NCH)])
    if n >= 257 and K > 1:
        z = chains[0]["Z"][:, 0, 0]
        assert z[0] == z[256] == z.max()      # the plant took
    r = smp.rescale()
    assert set(r) == {"transform", "inverse", "curve", "rcond", "z_min", "n_singular", "perm", "first_slot", "n_slots"} and r["perm"] is None
    _check_rescale(r, chains, 0, T, f"n={n} identity")
    assert smp.timing("rescale_transform")[1] == 1 and smp.timing("rescale_transform")[0] > 0.0
    perm = _random_perm(NCH, T - 1, K, n + K)
    r2 = smp.rescale(perm=perm, first_slot=1)
    _check_rescale(r2, chains, 1, T - 1, f"n={n} random perm, slots 1 ..", perm=perm)
    again = smp.rescale(perm=perm, first_slot=1)
    for k in ("transform", "inverse", "curve", "rcond", "z_min"):
        assert again[k].tobytes() == r2[k].tobytes(), k
    smp.close()


@pytest.mark.parametrize("K", [3, 5])
def test_inverse_from_near_pure_curves_to_the_barycentre(K):
    n, NCH, T = 70, 2, 3
    smp = _make(n, K, NCH, T)
    rng = np.random.default_rng(K)
    pure = [{"Z": rng.dirichlet(np.full(K, 0.05), size=n)} for _ in range(T)]
    bary = [{"Z": 1.0 / K + 4e-3 * (rng.dirichlet(np.full(K, 1.5), size=n) - 1.0 / K)} for _ in range(T)]
    chains = _plant(smp, [pure, bary])
    r = smp.rescale()
    refs = _check_rescale(r, chains, 0, T, "near-pure | barycentre")
    assert all(d["rcond"] > 0.2 for d in refs[0]), [d["rcond"] for d in refs[0]]
    assert all(1e-5 < d["rcond"] < 1e-2 for d in refs[1]), [d["rcond"] for d in refs[1]]
    given = np.ascontiguousarray(r["transform"][:, ::-1])      # any matrices will do: the other slots' transforms
    g = smp.rescale(transform=given)
    assert g["curve"] is None
    _check_rescale(g, chains, 0, T, "given mode", given=given)
    smp.close()


def test_two_components_on_one_curve_are_singular():
    n, K, NCH, T = 70, 3, 2, 3
    smp = _make(n, K, NCH, T)
    rng = np.random.default_rng(9)
    draws = [[{"Z": 0.4 * rng.dirichlet(np.full(K, 1.5), size=n) + 0.2, "nu": rng.standard_normal((K, smp.P))} for _ in range(T)]
             for _ in range(NCH)]
    draws[1][1]["Z"][7] = [0.65, 0.65, 0.2]        # the largest entry of columns 0 and 1
    draws[0][2]["Z"][11, 1] = np.nan               # never the maximum; z_min keeps it, and the draw is not singular
    chains = _plant(smp, draws)
    r = smp.rescale()
    refs = _check_rescale(r, chains, 0, T, "shared pure curve")
    assert r["n_singular"] == 1 and refs[1][1]["singular"] and r["curve"][1, 1, 0] == r["curve"][1, 1, 1] == 7
    assert np.isnan(r["z_min"][0, 2]) and r["rcond"][0, 2] > 0.0 and np.all(np.isfinite(r["inverse"][0, 2])) and 11 not in r["curve"][0, 2]
    z = smp.aligned_summary("Z", rescale=r, probs=PROBS)              # the pooled rows carry the NaN; no error
    assert np.all(np.isnan(z["mean"]))
    nu = smp.aligned_summary("nu", rescale=r, probs=PROBS)            # A itself is finite
    assert np.all(np.isfinite(nu["mean"])) and np.all(np.isfinite(nu["quantiles"]))
    smp.close()


# ---- permutation matrices: the permutation kernels' bits ------------------------------------------------------------------------
def _same_as_permutation_calls(smp, r, perm, names, first, S, x=None):
    kw = dict(first_slot=first, n_slots=S)
    for nm in names:
        a, b = smp.aligned_summary(nm, rescale=r, probs=PROBS, **kw), smp.aligned_summary(nm, perm, probs=PROBS, **kw)
        for k in STATS + ("quantiles",):
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (nm, k)
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:9])
    a, b = smp.cluster_mean_bands(E, perm, rescale=r, **kw), smp.cluster_mean_bands(E, perm, **kw)
    for k in ("mean", "sd", "quantiles"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for ckw in (dict(simultaneous=0.1, trace=True), dict(diagonal=True, simultaneous=0.2), dict(E2=E[::-1][:5].copy(), pairs=[(2, 0), (1, 1)]),
                dict(x=x, simultaneous=0.1) if x is not None else dict(probs=())):
        a, b = smp.cluster_cov_bands(E, rescale=r, **ckw, **kw), smp.cluster_cov_bands(E, perm, **ckw, **kw)
        for k in ("mean", "sd", "quantiles", "crit", "lower", "upper", "trace"):
            if k in b:
                assert a[k].tobytes() == b[k].tobytes(), (sorted(ckw), k)


@pytest.mark.parametrize("D", [0, 2])
def test_given_permutation_matrices_equal_the_aligned_calls(D):
    from test_gpu_align import _planted_pair
    a, b, ca, cb, perms, names, T = _planted_pair(D)
    b.close()
    perm = a.align(pivot=np.ascontiguousarray(ca[2]["Z"][:, :, 0]))["perm"]
    Pm = _perm_matrices(perm)
    r = a.rescale(perm=perm, transform=Pm)
    assert r["curve"] is None and r["n_singular"] == 0 and np.array_equal(r["perm"], perm)
    assert np.array_equal(r["transform"], Pm) and np.array_equal(r["inverse"], Pm.transpose(0, 1, 3, 2)) and np.all(r["rcond"] == 1.0)
    _same_as_permutation_calls(a, r, perm, [nm for nm in NAMES if D or nm not in ("eta", "xi")], 0, T, x=[0.4, -1.1] if D else None)
    a.close()


@pytest.fixture(scope="module")
def mixed():
    """n = 70, K = 3, M = 2, D = 2, 2 chains, 6 planted slots: slots 0 .. 2 generic memberships, slots 3 .. 5 with K rows exactly e_k"""
    n, K, NCH, T, D = 70, 3, 2, 6, 2
    smp = _make(n, K, NCH, T, D=D)
    rng = np.random.default_rng(77)
    draws = []
    for q in range(NCH):
        draws.append([])
        for t in range(T):
            Z = 0.9 * rng.dirichlet(np.full(K, 1.5), size=n) + 0.1 / K
            if t >= 3:
                Z[rng.choice(n, size=K, replace=False)] = np.eye(K)
            d = {"Z": Z}
            for nm in ("nu", "Phi", "eta", "xi"):
                d[nm] = rng.standard_normal(smp._draw_shape(nm))
            draws[q].append(d)
    d = dict(smp=smp, chains=_plant(smp, draws), K=K, D=D, T=T)
    yield d
    smp.close()


def test_planted_pure_curves_give_the_permutation_matrix(mixed):
    smp, K = mixed["smp"], mixed["K"]
    first, S = 3, 3
    perm = _random_perm(smp.n_chains, S, K, 4)
    r = smp.rescale(perm=perm, first_slot=first, n_slots=S)
    _check_rescale(r, mixed["chains"], first, S, "pure curves", perm=perm)
    Pm = _perm_matrices(perm)
    assert np.array_equal(r["transform"], Pm) and np.array_equal(r["inverse"], Pm.transpose(0, 1, 3, 2))
    assert np.all(r["rcond"] == 1.0) and np.all(r["z_min"] == 0.0) and r["n_singular"] == 0
    _same_as_permutation_calls(smp, r, perm, NAMES, first, S, x=[0.4, -1.1])


# ---- general transforms against numpy on the get_chain copies -------------------------------------------------------------------
def _draws(mixed, S):
    return [(q, s) for q in range(mixed["smp"].n_chains) for s in range(S)]


@pytest.fixture(scope="module")
def mixed_r(mixed):
    smp = mixed["smp"]
    first, S = 0, mixed["T"]
    perm = _random_perm(smp.n_chains, S, mixed["K"], 21)
    r = smp.rescale(perm=perm, first_slot=first, n_slots=S)
    _check_rescale(r, mixed["chains"], first, S, "mixed fixture", perm=perm)
    return dict(r=r, perm=perm, first=first, S=S)


@pytest.mark.parametrize("name", NAMES)
def test_mixed_rows_through_the_statistics(mixed, mixed_r, name):
    smp, K, r = mixed["smp"], mixed["K"], mixed_r["r"]
    first, S = mixed_r["first"], mixed_r["S"]
    got = smp.aligned_summary(name, rescale=r, probs=PROBS, first_slot=first, n_slots=S)
    v, b = [], []
    for q, s in _draws(mixed, S):
        x = mixed["chains"][q][name][..., first + s]
        A, Ai = r["transform"][q, s], r["inverse"][q, s]      # the device's own
        v.append(R.mix(x, name, A, Ai))
        b.append(K * U * R.mix_abs(x, name, A, Ai))
    v, b = np.stack(v, axis=-1), np.stack(b, axis=-1)
    assert v.shape[:-1] == smp._draw_shape(name)
    _check_rows(got, v, b, PROBS, f"aligned_summary({name}, rescale=)")
    assert all(np.all(np.isfinite(got[k])) for k in ("mean", "sd", "quantiles"))
    assert smp.timing("rescale_gather")[1] == 1


@pytest.mark.parametrize("x", [None, (0.3, -1.2)])
def test_mean_bands_against_numpy(mixed, mixed_r, x):
    smp, K, D, r = mixed["smp"], mixed["K"], mixed["D"], mixed_r["r"]
    first, S = mixed_r["first"], mixed_r["S"]
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:9])
    got = smp.cluster_mean_bands(E, rescale=r, x=x, probs=PROBS, first_slot=first, n_slots=S)
    v, a = [], []
    for q, s in _draws(mixed, S):
        ch = mixed["chains"][q]
        vv, aa = R.mean_values(E, ch["nu"][..., first + s], r["transform"][q, s], ch["eta"][..., first + s], x)
        v.append(vv)
        a.append(aa)
    v, a = np.stack(v, axis=-1), np.stack(a, axis=-1)
    _check_rows(got, v, (smp.P + K + D + 2) * U * a, PROBS, f"cluster_mean_bands(rescale=, x={x})")
    assert smp.timing("rescale_project")[1] == 1


@pytest.mark.parametrize("case", ["full", "diagonal", "pairs", "E2", "simultaneous", "x"])
def test_cov_bands_against_numpy(mixed, mixed_r, case):
    from test_gpu_cluster_cov import _check_reductions
    smp, K, D, r = mixed["smp"], mixed["K"], mixed["D"], mixed_r["r"]
    first, S = mixed_r["first"], mixed_r["S"]
    Eall = np.concatenate(smp.get_basis(), axis=0)
    E, E2, pairs, x, alpha, diagonal = np.ascontiguousarray(Eall[:17]), None, None, None, None, False
    if case == "diagonal":
        diagonal, alpha = True, 0.2
    elif case == "pairs":
        pairs = [(2, 0), (1, 1), (2, 0)]
    elif case == "E2":
        E2 = np.ascontiguousarray(Eall[20:25])
    elif case == "simultaneous":
        alpha = 0.1
    elif case == "x":
        x, alpha = (0.3, -1.2), 0.1
    got = smp.cluster_cov_bands(E, rescale=r, E2=E2, pairs=pairs, x=x, diagonal=diagonal, simultaneous=alpha, trace=True, first_slot=first,
                                         n_slots=S)
    pl = [(k, l) for k in range(K) for l in range(k, K)] if pairs is None else pairs
    assert got["pairs"].tolist() == [list(p) for p in pl]
    c, a = [], []
    for q, s in _draws(mixed, S):
        ch = mixed["chains"][q]
        cc, aa = R.cov_values(E, E2, ch["Phi"][..., first + s], r["transform"][q, s], pl, ch["xi"][..., first + s], x)
        if diagonal:
            cc, aa = np.stack([np.diag(m) for m in cc]), np.stack([np.diag(m) for m in aa])
        c.append(cc)
        a.append(aa)
    c, a = np.stack(c, axis=-1), np.stack(a, axis=-1)
    b = (2 * (smp.P + D + K + 1) + smp.M + 3) * U * np.asarray(a, dtype=np.float64)
    assert got["trace"].shape == c.shape, (got["trace"].shape, c.shape)
    err = np.abs(got["trace"] - np.asarray(c, dtype=np.float64))
    print(f"cov bands, {case}: {c.size} values, worst |device - numpy| / b = {float(np.max(err / b)):.3e}")
    assert np.all(err <= b), case
    _check_reductions(got, alpha, f"cov bands, {case}")


def test_results_do_not_depend_on_the_budget(mixed, mixed_r):
    smp, r = mixed["smp"], mixed_r["r"]
    kw = dict(first_slot=mixed_r["first"], n_slots=mixed_r["S"])
    N = smp.n_chains * mixed_r["S"]
    one = smp.aligned_summary("Z", rescale=r, probs=PROBS, **kw)
    few = smp.aligned_summary("Z", rescale=r, probs=PROBS, max_workspace_bytes=8 * N * 100, **kw)
    assert smp.timing("rescale_gather")[1] >= 2
    for k in STATS + ("quantiles",):
        assert one[k].tobytes() == few[k].tobytes(), k
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:9])
    one = smp.cluster_mean_bands(E, rescale=r, x=(0.3, -1.2), **kw)
    few = smp.cluster_mean_bands(E, rescale=r, x=(0.3, -1.2), max_workspace_bytes=8 * N * 10, **kw)
    assert smp.timing("rescale_project")[1] >= 2
    for k in ("mean", "sd", "quantiles"):
        assert one[k].tobytes() == few[k].tobytes(), k
    ckw = dict(simultaneous=0.1, trace=True, **kw)      # 6 x 9 x 9 rows, 100 to a chunk
    one = smp.cluster_cov_bands(E, rescale=r, **ckw)
    with pytest.raises(Exception) as ei:
        smp.cluster_cov_bands(E, rescale=r, max_workspace_bytes=1, **ckw)
    m = re.search(r"\((\d+) shared by all rows \+ (\d+) per row\)", str(ei.value))
    assert m and "bfmmm_chain_cluster_cov_bands_rescaled" in str(ei.value), str(ei.value)
    few = smp.cluster_cov_bands(E, rescale=r, max_workspace_bytes=int(m.group(1)) + 100 * int(m.group(2)), **ckw)
    assert smp.timing("cluster_cov")[1] >= 4      # two sweeps over at least two chunks
    for k in ("mean", "sd", "quantiles", "crit", "lower", "upper", "trace"):
        assert one[k].tobytes() == few[k].tobytes(), k


# ---- against the restatement of the reference's functions -----------------------------------------------------------------------
def test_single_chain_k2_matches_the_reference_functions():
    import bayesfmmm_amd as bf
    n, K, T = 40, 2, 12
    smp = _make(n, K, 1, T)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    ch = _copies(smp, ["Z", "nu"])[0]
    r = smp.rescale()
    assert r["n_singular"] == 0
    print(f"K = 2 chain: rcond {r['rcond'].min():.3e} .. {r['rcond'].max():.3e}, z_min {r['z_min'].min():.3e}")
    got = smp.aligned_summary("Z", rescale=r, probs=PROBS)
    ref = O.z_ci(ch["Z"], 0.05, True, 0.0)
    for c, nm in enumerate(("CI_Lower", "CI_50", "CI_Upper")):
        np.testing.assert_allclose(got["quantiles"][..., c], ref[nm], rtol=1e-11, atol=1e-12, err_msg=nm)
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:11])
    mb = smp.cluster_mean_bands(E, rescale=r, probs=PROBS)
    for k in (1, 2):
        ref = O.f_mean_ci(ch["nu"], E, k, 0.05, True, False, 0.0, Z=ch["Z"])
        for c, nm in enumerate(("CI_Lower", "CI_50", "CI_Upper")):
            np.testing.assert_allclose(mb["quantiles"][k - 1, :, c], ref[nm], rtol=1e-11, atol=1e-12, err_msg=nm)
    # ---- refusals, each with its message ----
    from bayesfmmm_amd._lib import BfmmmError
    with pytest.raises(BfmmmError, match="the reference defines no rescale for 'pi'"):
        smp.aligned_summary("pi", rescale=r)
    with pytest.raises(BfmmmError, match="'x' is given but the sampler has no covariates"):
        smp.cluster_mean_bands(E, rescale=r, x=[0.5])
    with pytest.raises(ValueError, match=r"rescale is of slots \[0, 12\), not of \[2, 12\)"):
        smp.aligned_summary("Z", rescale=r, first_slot=2)
    with pytest.raises(ValueError, match=r"transform must have shape \(1, 12, 2, 2\)"):
        smp.rescale(transform=np.zeros((1, 12, 2, 3)))
    ident = np.tile(np.arange(K, dtype=np.int32), (1, T, 1))
    with pytest.raises(ValueError, match="perm differs from the perm the rescale dict was computed with"):
        smp.aligned_summary("Z", ident, rescale=r)
    r2 = smp.rescale(perm=ident)
    with pytest.raises(ValueError, match="perm differs"):
        smp.cluster_cov_bands(E, ident[:, :, ::-1], rescale=r2)
    assert smp.aligned_summary("Z", ident, rescale=r2, probs=PROBS)["quantiles"].tobytes() == got["quantiles"].tobytes()
    with pytest.raises(ValueError, match="'x' is honoured only with rescale="):
        smp.cluster_mean_bands(E, ident, x=[0.5])
    other = dict(r, transform=np.zeros((2, T, K, K)))
    with pytest.raises(ValueError, match=r"rescale\['transform'\] has shape \(2, 12, 2, 2\), not \(1, 12, 2, 2\)"):
        smp.aligned_summary("Z", rescale=other)
    with pytest.raises(ValueError, match="rescale must be the dict"):
        smp.cluster_mean_bands(E, rescale=ident)
    smp.close()
