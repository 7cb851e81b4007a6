"""Marginal PSIS-LOO over curves with the memberships integrated out (Sampler.loo_marginal, bfmmm_chain_loo_marginal)
against Sampler.predict on the training data, api.psis_loo and the numpy restatement of tests/loo_marginal_ref.py.

Tolerances, as DESIGN.md 7m: TOL_L = 10 x the floor of tests/test_predict_ref.py (the worst |dense - Gamma form| / max(1, |l|) over
2000 random curves); a refined log-density is held within TOL_L max(1, max |l|) and ess / J2 within four times that, against the
restated stage on the device's own refinement samples with the dense l at them.  TOL_RULE0 = 10 x the floor of the refinement's stage
0 (tests/test_loo_marginal_ref.py: float64 against np.longdouble): every later stage's proposal is held within it, relative to
max(1, |.|).  Neither is tuned against the kernel."""
import re

import numpy as np
import pytest

import loo_marginal_ref as L
import predict_ref as R
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

K, M, N_CURVES, NCH, T = 3, 2, 8, 2, 24      # PSIS wants at least 21 draws a row
POINTWISE = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic")
ARRAYS = POINTWISE + ("ess_mean", "ess_min", "n_refined", "n_below", "lpd_trace", "ess_trace", "ess_trace_first", "refined_index",
                      "refine_prop", "refine_samples")


@pytest.fixture(scope="module")
def tol():
    floor_l, _ = R.ell_floor()
    floor_rule0 = L.stage0_floor()
    print(f"floors: l {floor_l:.3e}, refinement stage 0 {floor_rule0:.3e}")
    return {"l": 10.0 * floor_l, "rule0": 10.0 * floor_rule0}


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


def _start(smp, seed, mask=None):
    import bayesfmmm_amd as bf
    for q in range(smp.n_chains):
        smp.select_chain(q)
        smp.init_state(1, seed, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM if mask is None else mask, smp.T, seed=seed)


def _ragged(sim, rng, lengths):
    ts, ys, Bs = [], [], []
    for i, ln in enumerate(lengths):
        keep = np.sort(rng.choice(len(sim["t"][i]), size=int(ln), replace=False))
        ts.append(sim["t"][i][keep]); ys.append(sim["y"][i][keep]); Bs.append(sim["B"][i][keep])
    return ts, ys, Bs


def _functional_data(seed=41, D=0):
    sim = simulate_functional(n=N_CURVES, M=M, sigma_sq=0.05, seed=seed, K=K, D=D)
    rng = np.random.default_rng(3)
    lengths = rng.integers(5, 26, size=N_CURVES)
    lengths[1], lengths[6] = 5, 25
    ts, ys, Bs = _ragged(sim, rng, lengths)
    return sim, ts, ys, Bs


def tiny_sampler(sim, ys, ts, n_chains=NCH, iters=T):
    import bayesfmmm_amd as bf
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=iters)
    return bf.Sampler(cfg, ys, ts, sim["internal_knots"], sim["boundary_knots"], n_chains=n_chains)


@pytest.fixture(scope="module")
def base():
    """8 curves of 5 .. 25 points, K = 3, M = 2, cubic splines with P = 8, 2 chains x 24 slots after a short run"""
    sim, ts, ys, Bs = _functional_data()
    smp = tiny_sampler(sim, ys, ts)
    _start(smp, 7)
    d = dict(smp=smp, chains=_chains(smp), t=ts, y=ys, B=Bs, sim=sim, data=dict(Y_new=ys, time_new=ts))
    yield d
    smp.close()


def _same_bits(a, b, keys):
    for k in keys:
        assert k in a and k in b, k
        assert np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def _check_first_pass(smp, data, J, RS, seed=5):
    """refine=False: the traces are predict's on the training data, the pointwise arrays api.psis_loo's on that matrix, bit for bit"""
    from bayesfmmm_amd import api
    n, Cn, S = smp.n, smp.n_chains, smp.T
    lm = smp.loo_marginal(n_samples=J, n_stages=RS, seed=seed, refine=False, trace=True)
    pr = smp.predict(n_samples=J, n_stages=RS, seed=seed, trace=True, **data)
    assert lm["lpd_trace"].shape == (n, Cn, S)
    _same_bits(lm, pr, ("lpd_trace", "ess_trace"))
    assert lm["ess_trace_first"].tobytes() == pr["ess_trace"].tobytes()
    ps = api.psis_loo(lm["lpd_trace"].reshape(n, -1))
    _same_bits(lm, ps, POINTWISE)
    tot = api.loo_totals({k: lm[k] for k in POINTWISE}, Cn * S)
    for k, v in tot.items():
        assert np.array_equal(np.asarray(lm[k]), np.asarray(v)), k
    assert not lm["n_refined"].any() and lm["refined_index"].shape == (0, 3) and lm["refine"] is False
    assert (lm["n_samples"], lm["n_stages"]) == (J, RS)
    return lm, pr


def _check_refinement(smp, data, Bs, ys, chains, tol, J, RS, J2, R2, floor=None, X=None, cadj=False, seed=5, label=""):
    """every listed pair against the restated stages on the device's own samples; returns the call's dict"""
    n, Cn, S, Kc = smp.n, smp.n_chains, smp.T, smp.K
    pr = smp.predict(n_samples=J, n_stages=RS, seed=seed, trace=True, return_samples=True, **data)
    if floor is None:
        floor = float(np.median(pr["ess_trace"]))
    lm = smp.loo_marginal(n_samples=J, n_stages=RS, seed=seed, ess_floor=floor, refine_samples=J2, refine_stages=R2, trace=True)
    idx, cnt = L.select_list(pr["lpd_trace"], pr["ess_trace"], floor)
    assert lm["refined_index"].dtype == np.int32 and np.array_equal(lm["refined_index"], idx) and np.array_equal(lm["n_refined"], cnt)
    assert lm["ess_trace_first"].tobytes() == pr["ess_trace"].tobytes()
    prop, smpl = lm["refine_prop"], lm["refine_samples"]
    assert prop.shape == (len(idx), R2, Kc) and smpl.shape == (len(idx), R2, J2, Kc)
    i_, q_, s_ = idx[:, 0], idx[:, 1], idx[:, 2]
    # the refinement starts from the last proposal of the first pass
    assert np.ascontiguousarray(prop[:, 0]).tobytes() == np.ascontiguousarray(pr["proposal"][i_, q_, s_, RS - 1]).tobytes()
    # pairs not listed keep their first-pass bits
    keep = np.ones((n, Cn, S), dtype=bool)
    keep[i_, q_, s_] = False
    for k in ("lpd_trace", "ess_trace"):
        assert lm[k][keep].tobytes() == pr[k][keep].tobytes(), k
    assert np.all(smpl >= R.TINY) and np.allclose(smpl.sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    worst_l = worst_e = worst_p = 0.0
    for e, (i, q, s) in enumerate(idx):
        ch = chains[q]
        x = None if X is None else X[i]
        th, sig = _theta(ch, s, x, cadj), float(ch["sigma_sq"][s])
        prior = ch["alpha_3"][s] * ch["pi"][:, s]
        # another update id: the first samples are not the first pass's last ones
        Jc = min(J, J2)
        assert np.intersect1d(smpl[e, 0, :Jc].ravel(), pr["samples"][i, q, s, RS - 1, :Jc].ravel()).size == 0
        for st in range(R2):
            z = smpl[e, st]
            ell = R.ell_dense_batch(Bs[i], np.asarray(ys[i], dtype=np.float64), th, z, sig)
            ref = R.stage(R.log_weights(ell, z, prior, prop[e, st]), z)
            if st + 1 < R2:
                err = np.max(np.abs(prop[e, st + 1] - ref["next"]) / np.maximum(1.0, np.abs(ref["next"])))
                worst_p = max(worst_p, err)
                assert err <= tol["rule0"], (label, "proposal", e, st, err, tol["rule0"])
        scale = max(1.0, np.abs(ell).max())
        e_l = abs(lm["lpd_trace"][i, q, s] - ref["lpd"])
        e_e = abs(lm["ess_trace"][i, q, s] - ref["ess"]) / J2
        worst_l, worst_e = max(worst_l, e_l / (tol["l"] * scale)), max(worst_e, e_e / (4 * tol["l"] * scale))
        assert e_l <= tol["l"] * scale and e_e <= 4 * tol["l"] * scale, (label, e, e_l, e_e, tol["l"] * scale)
    print(f"{label} J2={J2} R2={R2}: {len(idx)} pairs refined of {n * Cn * S}; worst lpd error {worst_l:.3g} of its bound, ess / J2 "
          f"{worst_e:.3g} of its bound, proposal {worst_p:.2e} (bound {tol['rule0']:.2e})")
    # what is reported: the pairs the rule still picks, the least and the mean ess after the refinement
    assert np.all(np.isfinite(lm["lpd_trace"]))
    below = L.selected(lm["lpd_trace"], lm["ess_trace"], floor).reshape(n, -1).sum(axis=1)
    assert np.array_equal(lm["n_below"], below) and np.array_equal(below, (lm["ess_trace"] < floor).reshape(n, -1).sum(axis=1))
    flat = lm["ess_trace"].reshape(n, -1)
    assert np.array_equal(lm["ess_min"], flat.min(axis=1))
    assert np.all(np.abs(lm["ess_mean"] - flat.mean(axis=1)) <= 1e-12 * flat.mean(axis=1))      # sums of 48 terms in another order
    assert (lm["refine_stages"], lm["ess_floor"], lm["refine"]) == (R2, floor, True)
    return lm


@pytest.mark.parametrize("J,RS", [(64, 1), (64, 3), (300, 1), (300, 3)])
def test_first_pass_is_predict(base, J, RS):
    _check_first_pass(base["smp"], base["data"], J, RS)


def test_selection(base):
    smp = base["smp"]
    J, RS = 64, 2
    n, N = smp.n, NCH * T
    kw = dict(n_samples=J, n_stages=RS, seed=3, trace=True)
    first = smp.loo_marginal(refine=False, **kw)
    floor = float(np.median(first["ess_trace"]))
    got = smp.loo_marginal(ess_floor=floor, **kw)
    assert got["refine_samples"].shape[2] == 4 * J            # the default
    sel = first["ess_trace"] < floor
    assert 0 < sel.sum() < sel.size
    assert np.array_equal(got["refined_index"], np.argwhere(sel)) and np.array_equal(got["n_refined"], sel.reshape(n, -1).sum(axis=1))
    _same_bits(got, first, ("ess_trace_first",))
    assert got["ess_trace_first"].tobytes() == first["ess_trace"].tobytes()
    for k in ("lpd_trace", "ess_trace"):
        assert got[k][~sel].tobytes() == first[k][~sel].tobytes(), k
        assert not np.any(got[k][sel] == first[k][sel]), k
    # a floor of 0 refines nothing and is refine=False
    zero = smp.loo_marginal(ess_floor=0.0, **kw)
    _same_bits(zero, first, POINTWISE + ("ess_mean", "ess_min", "n_refined", "lpd_trace", "ess_trace", "ess_trace_first", "refined_index"))
    assert not zero["n_below"].any() and zero["refine_prop"].shape[0] == 0      # (n_below goes with the floor: none is below 0)
    assert np.array_equal(first["n_below"], (first["ess_trace"] < 10.0).reshape(n, -1).sum(axis=1))
    # a floor above J refines every pair
    every = smp.loo_marginal(ess_floor=J + 1.0, refine_samples=32, refine_stages=1, **kw)
    assert np.all(every["n_refined"] == N) and every["refined_index"].shape == (n * N, 3)
    assert np.array_equal(every["refined_index"], np.argwhere(np.ones((n, NCH, T), dtype=bool)))


@pytest.mark.parametrize("J2,R2", [(128, 1), (128, 2), (600, 1), (600, 2)])
def test_refinement_against_the_reference(base, tol, J2, R2):
    _check_refinement(base["smp"], base["data"], base["B"], base["y"], base["chains"], tol, 64, 2, J2, R2, label="base")


def test_bits_under_budget_and_repeat(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    kw = dict(n_samples=64, n_stages=2, seed=9, ess_floor=20.0, refine_samples=128, refine_stages=2, trace=True)
    one = smp.loo_marginal(**kw)
    assert 0 < one["n_refined"].sum() < N_CURVES * NCH * T
    assert smp.timing("loo_marginal_psis")[1] == 1 and smp.timing("loo_marginal")[1] == 5
    _same_bits(smp.loo_marginal(**kw), one, ARRAYS)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_marginal: .*'max_workspace_bytes'") as ei:
        smp.loo_marginal(max_workspace_bytes=1, **kw)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    assert shared == 0
    single = smp.loo_marginal(max_workspace_bytes=per_curve, **kw)
    assert smp.timing("loo_marginal_psis")[1] == N_CURVES          # one curve a chunk
    _same_bits(single, one, ARRAYS)
    for k in ("elpd_loo", "p_loo", "elpd_waic", "n_khat_above"):
        assert single[k] == one[k], k
    # without the traces: the same results
    plain = smp.loo_marginal(**dict(kw, trace=False))
    _same_bits(plain, one, POINTWISE + ("ess_mean", "ess_min", "n_refined", "n_below"))
    assert "lpd_trace" not in plain and plain["refine_samples"] == 128


def test_state_and_run_do_not_see_the_call(base):
    import bayesfmmm_amd as bf
    from gpu_parity import STATE_NAMES
    outs = []
    for with_call in (False, True):
        smp = tiny_sampler(base["sim"], base["y"], base["t"])
        for q in range(NCH):
            smp.select_chain(q)
            smp.init_state(1, 7, chain=q)
        smp.select_chain(0)
        smp.run(bf.SWEEP_WARM, T - 2, seed=7)
        if with_call:
            smp.loo_marginal(n_slots=T - 2, n_samples=37, n_stages=2, ess_floor=20.0, refine_samples=64)
        smp.run(bf.SWEEP_WARM, 2, first_iter=T - 2, seed=7)
        state = []
        for q in range(NCH):
            smp.select_chain(q)
            state.append([smp.get_state(nm).tobytes() for nm in STATE_NAMES] + [smp.get_chain(nm).tobytes() for nm in ("nu", "Phi", "Z", "pi", "sigma_sq", "loglik")])
        outs.append(state)
        smp.close()
    assert outs[0] == outs[1]


def _check_instance(smp, data, Bs, ys, tol, label, cov=False, X=None, cadj=False):
    chains = _chains(smp, cov)
    _check_first_pass(smp, data, 64, 2)
    _check_refinement(smp, data, Bs, ys, chains, tol, 64, 2, 128, 2, X=X, cadj=cadj, label=label)


@pytest.mark.parametrize("Kc,Mc,P", [(5, 2, 6), (3, 6, 8), (3, 2, 5)])
def test_multivariate_instances(tol, Kc, Mc, P):
    """K = 5: the KMAX instance; M = 6: K (M + 1) = 21 directions, padded to 32; the multivariate model at K = 3, M = 2, P = 5"""
    import bayesfmmm_amd as bf
    Y = np.random.default_rng(P + Kc).standard_normal((N_CURVES, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=Kc, n_eigen=Mc, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    _start(smp, 17)
    _check_instance(smp, dict(Y_new=Y), [np.eye(P)] * N_CURVES, list(Y), tol, f"multivariate K={Kc} M={Mc} P={P}")
    smp.close()


def test_covariates_with_covariance_adjustment(tol):
    import bayesfmmm_amd as bf
    S_ = bf.sampler
    sim, ts, ys, Bs = _functional_data(seed=33, D=2)
    smp = tiny_sampler(sim, ys, ts)
    smp.set_covariates(sim["X"], covariance_adj=True)
    _start(smp, 5, S_.SWEEP_WARM | S_.COV_MEAN | S_.COV_XI)
    _check_instance(smp, dict(Y_new=ys, time_new=ts, X_new=sim["X"]), Bs, ys, tol, "covariates D=2", cov=True, X=sim["X"], cadj=True)
    smp.close()


def test_tensor_product_basis_on_the_wide_band(tol):
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    sim = simulate_tensor(N_CURVES, 2, 2, [1, 2], [1, 1], seed=12, n_pts=30)      # 3 x 4 = 12 basis functions, band 6
    assert sim["P"] == 12 and sim["band"] == 6
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=2, n_eigen=2, basis_degree=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    _start(smp, 9)
    _check_instance(smp, dict(Y_new=sim["y"], basis_new=sim["B"]), sim["B"], sim["y"], tol, "tensor 3 x 4")
    smp.close()


def test_refusals_by_name(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    name = "bfmmm_chain_loo_marginal: "
    with pytest.raises(_lib.BfmmmError, match=name + r"n x refine_stages x refine_samples x K = 8 x 2 x 2000000000 x 3 exceeds the 4294967296"):
        smp.loo_marginal(refine_samples=2_000_000_000)
    with pytest.raises(_lib.BfmmmError, match=name + r"n x n_stages x n_samples x K = 8 x 3 x 2000000000 x 3 exceeds the 4294967296"):
        smp.loo_marginal(n_samples=2_000_000_000, refine_samples=8)
    with pytest.raises(_lib.BfmmmError, match=name + r"k_lz_refine: .*'refine_samples'\) need \d+ bytes of LDS, above the limit of 163840") as ei:
        smp.loo_marginal(n_samples=64, refine_samples=8192)
    assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) > 163840
    with pytest.raises(_lib.BfmmmError, match=name + r"k_predict: the tables of a draw .* above the limit of 163840"):
        smp.loo_marginal(n_samples=8192, refine=False)
    with pytest.raises(_lib.BfmmmError, match=name + "'ess_floor' must be finite and not negative"):
        smp.loo_marginal(ess_floor=-1.0)
    with pytest.raises(_lib.BfmmmError, match=name + "'ess_floor' must be finite and not negative"):
        smp.loo_marginal(ess_floor=float("nan"))
    with pytest.raises(_lib.BfmmmError, match=name + "'refine_stages' must be at least 1, got 0"):
        smp.loo_marginal(refine_stages=0)
    with pytest.raises(_lib.BfmmmError, match=name + "'refine_samples' must be at least 1, got 0"):
        smp.loo_marginal(refine_samples=0)
    with pytest.raises(_lib.BfmmmError, match=name + "'n_samples' must be at least 1"):
        smp.loo_marginal(n_samples=0)
    with pytest.raises(_lib.BfmmmError, match=name + "'n_stages' must be at least 1"):
        smp.loo_marginal(n_stages=0)
    with pytest.raises(_lib.BfmmmError, match=name + "'n_slots' out of range"):
        smp.loo_marginal(first_slot=2, n_slots=T)
    with pytest.raises(_lib.BfmmmError, match=name + "'first_slot' out of range"):
        smp.loo_marginal(first_slot=T)
    with pytest.raises(_lib.BfmmmError, match=name + "'max_workspace_bytes' must not be negative"):
        smp.loo_marginal(max_workspace_bytes=-1)
    with pytest.raises(_lib.BfmmmError, match=name + r"'refine_samples_out' of one curve .* need \d+ bytes"):
        smp.loo_marginal(n_samples=64, refine_samples=600, trace=True, max_workspace_bytes=100_000)
