"""The fitted function of held-out, partly observed curves from the chain slots on the device (Sampler.predict_fit,
bfmmm_chain_predict_fit) against the numpy restatement of tests/predict_fit_ref.py in its dense form.

Tolerances.  TOL = 10 x the floor of tests/test_predict_fit_ref.py (the worst |dense - table form| / max(1, |value|) of mu_j and s_j
over 2000 random curves, measured again here by the same function).  A quantity that does not depend on the importance weights (a
path given its sample, the result where all samples are equal) is held within TOL max(1, max |value|); one that does (mean_trace,
var_trace, mean, sd) within 4 TOL max(1, max |value|), as the memberships of 7m are.  The sd is held as a variance: the square root
near 0 has no bounded error."""
import math
import re

import numpy as np
import pytest

import curve_fit_ref as CF
import oracle_lib as O
import predict_fit_ref as F
import predict_ref as R

pytestmark = pytest.mark.gpu

NCH, T, NTRAIN = 2, 6, 24
LENGTHS = (1, 3, 17, 40, 40)
POOLED = ("lpd", "Z_mean", "Z_sd", "ess_mean", "ess_min")
TRACES = ("lpd_trace", "ess_trace", "Z_trace")
FIT = ("mean", "sd", "quantiles")
FIT_TRACES = ("mean_trace", "var_trace", "path_trace", "path_index", "path_u", "path_xi")


@pytest.fixture(scope="module")
def tol():
    floor, floor_ld, _ = F.fit_floor()
    print(f"floors: dense against table {floor:.3e}, float64 against longdouble {floor_ld:.3e}")
    return 10.0 * floor


def _simulate(n, P, M, K, seed, lengths=None, D=0):
    """n curves on cubic B-splines with P functions over t = 0 .. 990: {"t", "y", "B"} lists, knots, the full-domain basis and X"""
    rng = np.random.default_rng(seed)
    t_full = np.arange(0.0, 1000.0, 10.0)
    n_int = P - 4
    ik = np.quantile(t_full, np.arange(1, n_int + 1) / (n_int + 1))
    bk = np.array([t_full[0], t_full[-1]])
    B_full = O.bspline_basis(t_full, ik, 3, bk)
    nu = 2.0 * rng.standard_normal((K, P))
    Phi = 0.4 * rng.uniform(size=(K, P, M))
    X = rng.standard_normal((n, D)) if D > 0 else None
    eta = rng.standard_normal((P, D, K)) if D > 0 else None
    ts, ys, Bs = [], [], []
    for i in range(n):
        z = rng.dirichlet(np.ones(K))
        c = z @ nu + np.einsum("k,kpm,m->p", z, Phi, rng.standard_normal(M))
        if D > 0:
            c = c + np.einsum("pdk,d,k->p", eta, X[i], z)
        ln = 40 if lengths is None else lengths[i]
        keep = np.sort(rng.choice(len(t_full), size=ln, replace=False))
        ts.append(t_full[keep]); Bs.append(B_full[keep]); ys.append(B_full[keep] @ c + 0.1 * rng.standard_normal(ln))
    return dict(t=ts, y=ys, B=Bs, ik=ik, bk=bk, B_full=B_full, t_full=t_full, X=X)


def _left_half(sim, i, ln, seed):
    """curve i observed at ln points of the left half of the domain only"""
    rng = np.random.default_rng(seed)
    keep = np.sort(rng.choice(len(sim["t_full"]) // 2, size=ln, replace=False))
    full = np.linalg.lstsq(sim["B"][i], sim["y"][i], rcond=None)[0] if len(sim["y"][i]) >= sim["B_full"].shape[1] else np.zeros(sim["B_full"].shape[1])
    sim["t"][i], sim["B"][i] = sim["t_full"][keep], sim["B_full"][keep]
    sim["y"][i] = sim["B"][i] @ full + 0.1 * rng.standard_normal(ln)


def _start(smp, seed, mask=None):
    import bayesfmmm_amd as bf
    for q in range(smp.n_chains):
        smp.select_chain(q)
        smp.init_state(1, seed, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM if mask is None else mask, smp.T, seed=seed)


def _chains(smp, cov=False):
    names = ["nu", "Phi", "sigma_sq", "pi", "alpha_3"] + (["eta", "xi"] if cov else [])
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in names})
    smp.select_chain(0)
    return out


def _theta(ch, s, x=None, cadj=False):
    return R.directions(ch["nu"][..., s], ch["Phi"][..., s], ch["eta"][..., s] if x is not None else None,
                        ch["xi"][..., s] if x is not None else None, x, cadj)


def _functional(P, M, K, seed, lengths=LENGTHS, slots=T, D=0, cadj=False):
    import bayesfmmm_amd as bf
    m = len(lengths)
    sim = _simulate(NTRAIN + m, P, M, K, seed, [40] * NTRAIN + list(lengths), D=D)
    if m >= 3:
        _left_half(sim, NTRAIN + 2, lengths[2], seed + 1)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=slots)
    smp = bf.Sampler(cfg, sim["y"][:NTRAIN], sim["t"][:NTRAIN], sim["ik"], sim["bk"], n_chains=NCH)
    mask = None
    if D > 0:
        smp.set_covariates(sim["X"][:NTRAIN], covariance_adj=cadj)
        mask = bf.sampler.SWEEP_WARM | bf.sampler.COV_MEAN | (bf.sampler.COV_XI if cadj else 0)
    _start(smp, 7, mask)
    E = sim["B_full"][np.linspace(0, len(sim["t_full"]) - 1, 17).astype(int)]          # 17 rows over the whole domain
    return dict(smp=smp, chains=_chains(smp, D > 0), sim=sim, yn=sim["y"][NTRAIN:], tn=sim["t"][NTRAIN:], Bn=sim["B"][NTRAIN:], E=E,
                Xn=None if D == 0 else sim["X"][NTRAIN:], cadj=cadj)


@pytest.fixture(scope="module")
def base():
    """24 training curves, P = 12, M = 3, K = 3, 2 chains x 6 slots; 5 new curves of 1, 3, 17, 40 and 40 points, the third on the left
    half of the domain only; E: 17 rows over the whole domain"""
    d = _functional(12, 3, 3, 41)
    assert d["smp"].P == 12 and d["tn"][2].max() < 500.0 and d["E"].shape == (17, 12)
    yield d
    d["smp"].close()


def _zs(rng, C, S, J, Kc):
    z = rng.dirichlet(np.full(Kc, 0.8), size=(C, S, J))
    z[0, 0, 0, 0] = R.TINY
    return np.ascontiguousarray(np.maximum(z, R.TINY))


def _check_dense(got, chains, Bn, yn, E, zs, tol, label, Xn=None, cadj=False, noise=False, weights=True):
    """mean_trace, var_trace, mean and sd of a given-samples call (R = 1) against the dense reference; weights False: all samples are
    equal, the single-Gaussian closed form and the bound without the factor 4"""
    fac = 4.0 if weights else 1.0
    worst = 0.0
    for r in range(len(yn)):
        x = None if Xn is None else Xn[r]
        y = np.asarray(yn[r], dtype=np.float64)
        mts, vts, scale_m, scale_v = [], [], 1.0, 1.0
        for q, ch in enumerate(chains):
            for s in range(zs.shape[1]):
                th, sig = _theta(ch, s, x, cadj), float(ch["sigma_sq"][s])
                if weights:
                    mu, sv = F.fit_dense_batch(Bn[r], y, th, zs[q, s], sig, E, noise)
                    ell = R.ell_dense_batch(Bn[r], y, th, zs[q, s], sig)
                    mt, vt = F.mixture(np.exp(ell - ell.max()), mu, sv)
                else:
                    mt, vt = F.fit_dense(Bn[r], y, th, zs[q, s, 0], sig, E, noise)
                    mu, sv = mt[None], vt[None]
                scale_m, scale_v = max(scale_m, np.abs(mu).max()), max(scale_v, (sv + (mu - mt) ** 2).max())
                e_m = np.abs(got["mean_trace"][r, :, q, s] - mt).max() / (fac * tol * max(1.0, np.abs(mu).max()))
                e_v = np.abs(got["var_trace"][r, :, q, s] - vt).max() / (fac * tol * max(1.0, (sv + (mu - mt) ** 2).max()))
                worst = max(worst, e_m, e_v)
                assert e_m <= 1.0 and e_v <= 1.0, (label, r, q, s, e_m, e_v)
                mts.append(mt); vts.append(vt)
        mean, sd = F.pooled_fit(np.array(mts), np.array(vts))
        e_m = np.abs(got["mean"][r] - mean).max() / (fac * tol * scale_m)
        e_v = np.abs(got["sd"][r] ** 2 - sd ** 2).max() / (fac * tol * max(scale_v, scale_m ** 2))
        worst = max(worst, e_m, e_v)
        assert e_m <= 1.0 and e_v <= 1.0, (label, r, "pooled", e_m, e_v)
    print(f"{label}: worst error / bound = {worst:.3e} (bound {fac:g} x {tol:.2e} x max(1, max |value|))")


def _bits(d, keys):
    return {k: np.ascontiguousarray(d[k]).tobytes() for k in keys}


@pytest.mark.parametrize("J", [64, 256, 300])
def test_given_samples_against_the_dense_reference(base, tol, J):
    """J = 300 takes the loop path: l(z) is evaluated again for every block of 256 samples"""
    smp, E = base["smp"], base["E"]
    zs = _zs(np.random.default_rng(J), NCH, T, J, 3)
    got = smp.predict_fit(base["yn"], E, base["tn"], n_samples=J, n_stages=1, trace=True, z_samples=zs)
    assert got["mean"].shape == (5, 17) and got["quantiles"].shape == (5, 17, 3) and got["mean_trace"].shape == (5, 17, NCH, T)
    _check_dense(got, base["chains"], base["Bn"], base["yn"], E, zs, tol, f"J={J}")
    same = smp.predict(base["yn"], base["tn"], n_samples=J, n_stages=1, trace=True, z_samples=zs)
    assert _bits(got, POOLED + TRACES) == _bits(same, POOLED + TRACES)


def test_equal_samples_give_the_single_gaussian(base, tol):
    smp, E = base["smp"], base["E"]
    z0 = np.array([0.2, 0.5, 0.3])
    zs = np.ascontiguousarray(np.broadcast_to(z0, (NCH, T, 64, 3)))
    got = smp.predict_fit(base["yn"], E, base["tn"], n_samples=64, n_stages=1, trace=True, z_samples=zs)
    _check_dense(got, base["chains"], base["Bn"], base["yn"], E, zs, tol, "equal samples", weights=False)


@pytest.mark.parametrize("G", [1, 33])
def test_other_grids(base, tol, G):
    """G = 1; G = 33: three tiles of 16 rows and five groups of eight"""
    smp = base["smp"]
    E = base["sim"]["B_full"][np.linspace(0, 99, G).astype(int)]
    zs = _zs(np.random.default_rng(G), NCH, T, 64, 3)
    got = smp.predict_fit(base["yn"], E, base["tn"], n_samples=64, n_stages=1, trace=True, z_samples=zs)
    _check_dense(got, base["chains"], base["Bn"], base["yn"], E, zs, tol, f"G={G}")


def _variant(d, tol, label):
    smp = d["smp"]
    zs = _zs(np.random.default_rng(4), NCH, smp.T, 64, smp.K)
    kw = dict(n_samples=64, n_stages=1, trace=True, z_samples=zs, X_new=d["Xn"], **d.get("inputs", {}))
    got = smp.predict_fit(d["yn"], d["E"], **kw)
    _check_dense(got, d["chains"], d["Bn"], d["yn"], d["E"], zs, tol, label, Xn=d["Xn"], cadj=d["cadj"])
    same = smp.predict(d["yn"], **kw)
    assert _bits(got, POOLED + TRACES) == _bits(same, POOLED + TRACES)
    smp.close()


@pytest.mark.parametrize("P,M,K", [(12, 3, 5), (12, 1, 3)])
def test_other_shapes(tol, P, M, K):
    """K = 5: the instance with eight memberships a lane; M = 1"""
    d = _functional(P, M, K, 50 + K + M, slots=3)
    d["inputs"] = dict(time_new=d["tn"])
    _variant(d, tol, f"K={K} M={M}")


def test_covariates_with_covariance_adjustment(tol):
    d = _functional(12, 2, 3, 61, slots=3, D=2, cadj=True)
    d["inputs"] = dict(time_new=d["tn"])
    _variant(d, tol, "D=2 covariance-adjusted")


def test_from_basis_handle(tol):
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    sim = simulate_tensor(NTRAIN + 3, 2, 2, [1, 2], [1, 1], seed=12, n_pts=30)      # 3 x 4 = 12 basis functions, band 6
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=2, n_eigen=2, basis_degree=2, tot_mcmc_iters=3)
    smp = bf.Sampler(cfg, sim["y"][:NTRAIN], basis=sim["B"][:NTRAIN], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    _start(smp, 9)
    Bn = [b[:ln] for b, ln in zip(sim["B"][NTRAIN:], (30, 11, 2))]
    yn = [y[:ln] for y, ln in zip(sim["y"][NTRAIN:], (30, 11, 2))]
    d = dict(smp=smp, chains=_chains(smp), yn=yn, Bn=Bn, E=sim["B"][0][:17], Xn=None, cadj=False, inputs=dict(basis_new=Bn))
    _variant(d, tol, "from-basis 3 x 4")


def test_multivariate_with_the_identity(tol):
    import bayesfmmm_amd as bf
    P = 8
    Y = np.random.default_rng(P).standard_normal((NTRAIN + 3, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=3, n_eigen=2, tot_mcmc_iters=3)
    smp = bf.Sampler(cfg, Y[:NTRAIN], n_chains=NCH)
    _start(smp, 17)
    d = dict(smp=smp, chains=_chains(smp), yn=Y[NTRAIN:], Bn=[np.eye(P)] * 3, E=np.eye(P), Xn=None, cadj=False)
    _variant(d, tol, "multivariate P=8")


def test_path_rule(base, tol):
    smp, E = base["smp"], base["E"]
    J = 64
    zs = _zs(np.random.default_rng(8), NCH, T, J, 3)
    got = smp.predict_fit(base["yn"], E, base["tn"], n_samples=J, n_stages=1, seed=5, trace=True, z_samples=zs)
    assert got["path_index"].dtype == np.int32 and np.all((got["path_u"] > 0) & (got["path_u"] < 1))
    worst = 0.0
    for r in range(5):
        for q, ch in enumerate(base["chains"]):
            for s in range(T):
                th, sig = _theta(ch, s), float(ch["sigma_sq"][s])
                ell = R.ell_dense_batch(base["Bn"][r], base["yn"][r], th, zs[q, s], sig)
                cum = np.cumsum(np.exp(ell - ell.max()))
                js, target, slack = int(got["path_index"][r, q, s]), got["path_u"][r, q, s] * cum[-1], 1e-12 * cum[-1]
                assert 0 <= js < J and cum[js] > target - slack and (js == 0 or cum[js - 1] <= target + slack), (r, q, s, js)
                ref = F.path_dense(base["Bn"][r], base["yn"][r], th, zs[q, s, js], sig, E, got["path_xi"][r, q, s])
                err = np.abs(got["path_trace"][r, :, q, s] - ref).max() / (tol * max(1.0, np.abs(ref).max()))
                worst = max(worst, err)
                assert err <= 1.0, (r, q, s, err)
    print(f"paths given the device's j*, U and xi: worst error / bound = {worst:.3e}")
    # the quantiles: a selection or interpolation of the stored paths
    ref_q = CF.quantiles(got["path_trace"].reshape(5, 17, NCH * T), got["probs"])
    assert np.all(np.abs(got["quantiles"] - ref_q) <= 1e-14 * np.abs(ref_q))


def test_path_normals_at_a_fixed_seed():
    """10 new curves x 2 chains x 40 slots x M = 3: 2400 standard normals"""
    d = _functional(12, 3, 3, 41, slots=40)
    got = d["smp"].predict_fit(d["yn"] + d["yn"], d["E"], d["tn"] + d["tn"], n_samples=16, n_stages=1, seed=123, trace=True)
    xi = got["path_xi"].reshape(-1)
    n = xi.size
    print(f"path_xi: n = {n}, mean {xi.mean():.4f} (bound {5 / math.sqrt(n):.4f}), var - 1 = {xi.var() - 1:.4f} (bound {5 * math.sqrt(2 / n):.4f})")
    assert n >= 2000 and abs(xi.mean()) <= 5.0 / math.sqrt(n) and abs(xi.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert len(np.unique(xi)) == n and len(np.unique(got["path_u"])) == got["path_u"].size
    d["smp"].close()


@pytest.mark.parametrize("RS", [1, 3])
def test_bits_against_predict_chunks_repeats_and_noise(base, tol, RS):
    from bayesfmmm_amd import _lib
    smp, E = base["smp"], base["E"]
    kw = dict(n_samples=37, n_stages=RS, seed=9, trace=True)
    one = smp.predict_fit(base["yn"], E, base["tn"], **kw)
    same = smp.predict(base["yn"], base["tn"], **kw)
    assert _bits(one, POOLED + TRACES + ("proposal",)) == _bits(same, POOLED + TRACES + ("proposal",))
    ALL = POOLED + TRACES + FIT + FIT_TRACES
    assert _bits(smp.predict_fit(base["yn"], E, base["tn"], **kw), ALL) == _bits(one, ALL)
    # one curve a chunk, from the refusal's own figures
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict_fit: 'max_workspace_bytes' below the") as ei:
        smp.predict_fit(base["yn"], E, base["tn"], max_workspace_bytes=1, **kw)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    few = smp.predict_fit(base["yn"], E, base["tn"], max_workspace_bytes=shared + per_curve, **kw)
    assert _bits(few, ALL) == _bits(one, ALL)
    assert smp.timing("predict_fit")[1] == 4 * 5 and smp.timing("predict_stats")[1] == 1
    # noise: sigma^2 more variance in every draw, the same mean
    noisy = smp.predict_fit(base["yn"], E, base["tn"], noise=True, **kw)
    assert noisy["mean"].tobytes() == one["mean"].tobytes() and noisy["mean_trace"].tobytes() == one["mean_trace"].tobytes()
    sig = np.stack([ch["sigma_sq"] for ch in base["chains"]])                      # (C, S)
    bound = 4.0 * tol * np.maximum(1.0, noisy["var_trace"].max())
    assert np.all(np.abs(noisy["var_trace"] - one["var_trace"] - sig[None, None]) <= bound)
    assert np.all(np.abs(noisy["sd"] ** 2 - one["sd"] ** 2 - sig.mean()) <= bound)
    assert noisy["path_index"].tobytes() == one["path_index"].tobytes() and noisy["path_trace"].tobytes() != one["path_trace"].tobytes()


def test_refusals_by_name(base):
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    from bayesfmmm_amd.sampler import _dp
    smp, E, yn, tn = base["smp"], base["E"], base["yn"], base["tn"]
    FN = "bfmmm_chain_predict_fit: "
    bad = E.copy(); bad[3, 2] = np.inf
    with pytest.raises(_lib.BfmmmError, match=FN + r"'E'\[3, 2\] is not finite"):
        smp.predict_fit(yn, bad, tn)
    with pytest.raises(_lib.BfmmmError, match=FN + "'G' must be at least 1"):
        smp.predict_fit(yn, np.zeros((0, 12)), tn)
    big = np.zeros((4000, 12))
    with pytest.raises(_lib.BfmmmError, match=FN + r"k_predict_fit: the tables of a draw .* need \d+ bytes of LDS, above the limit of 163840"):
        smp.predict_fit(yn, big, tn)
    with pytest.raises(_lib.BfmmmError, match=FN + r"'max_workspace_bytes' below the \d+ bytes one curve needs"):
        smp.predict_fit(yn, E, tn, max_workspace_bytes=64)
    with pytest.raises(_lib.BfmmmError, match=FN + "'zs' takes the place of the stage-0 samples: 'n_stages' must be 1, got 2"):
        smp.predict_fit(yn, E, tn, n_samples=4, n_stages=2, z_samples=_zs(np.random.default_rng(0), NCH, T, 4, 3))
    with pytest.raises(_lib.BfmmmError, match=FN + "new curve 1 is empty"):
        smp.predict_fit([yn[0], yn[1][:0]], E, [tn[0], tn[1][:0]])
    with pytest.raises(_lib.BfmmmError, match=FN + "'X' is given but the sampler has no covariates"):
        smp.predict_fit(yn, E, tn, X_new=np.zeros((5, 2)))
    with pytest.raises(_lib.BfmmmError, match=FN + r"'probs'\[0\] outside \[0, 1\]"):
        smp.predict_fit(yn, E, tn, probs=(1.5,))
    # a null E, straight at the C ABI
    y, t = np.ascontiguousarray(yn[3]), np.ascontiguousarray(tn[3])
    off = np.array([0, len(y)], dtype=np.int64)
    o = [np.zeros(17 * 3) for _ in range(8)]
    rc = smp.lib.bfmmm_chain_predict_fit(smp.h, _dp(y), _dp(t), None, off.ctypes.data_as(_lib.c_int64_p), 1, None, None, 0, T, 4, 1, 1, None,
                                         None, 17, 0, None, 0, 0, *(_dp(a) for a in o), *([None] * 11), 1)
    assert rc != 0 and FN + "'E' is null" in smp.lib.bfmmm_last_error().decode()
    sim = base["sim"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=3, n_eigen=3, basis_degree=3, tot_mcmc_iters=2)
    cov = bf.Sampler(cfg, sim["y"][:NTRAIN], sim["t"][:NTRAIN], sim["ik"], sim["bk"])
    cov.set_covariates(np.random.default_rng(2).standard_normal((NTRAIN, 2)))
    with pytest.raises(_lib.BfmmmError, match=FN + "'X' is null but the sampler has 2 covariates"):
        cov.predict_fit(yn, E, tn)
    cov.close()


def test_state_and_slots_do_not_see_a_predict_fit(base):
    import bayesfmmm_amd as bf
    from gpu_parity import STATE_NAMES
    sim = base["sim"]
    outs = []
    for with_call in (False, True):
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=3, n_eigen=3, basis_degree=3, tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, sim["y"][:NTRAIN], sim["t"][:NTRAIN], sim["ik"], sim["bk"], n_chains=NCH)
        for q in range(NCH):
            smp.select_chain(q)
            smp.init_state(1, 7, chain=q)
        smp.select_chain(0)
        smp.run(bf.SWEEP_WARM, T - 1, seed=7)
        before = [c_[nm].tobytes() for c_ in _chains(smp) for nm in ("nu", "Phi", "sigma_sq", "pi", "alpha_3")]
        if with_call:
            smp.predict_fit(base["yn"], base["E"], base["tn"], n_samples=37, n_stages=2, n_slots=T - 1)
            assert before == [c_[nm].tobytes() for c_ in _chains(smp) for nm in ("nu", "Phi", "sigma_sq", "pi", "alpha_3")]
        smp.run(bf.SWEEP_WARM, 1, first_iter=T - 1, seed=7)
        state = []
        for q in range(NCH):
            smp.select_chain(q)
            state.append([smp.get_state(nm).tobytes() for nm in STATE_NAMES] + [smp.get_chain(nm).tobytes() for nm in ("nu", "Phi", "Z", "pi", "sigma_sq", "loglik")])
        smp.select_chain(0)
        outs.append(state)
        smp.close()
    assert outs[0] == outs[1]
