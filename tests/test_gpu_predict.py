"""Prediction of held-out curves from the chain slots on the device (Sampler.predict, bfmmm_chain_predict) against the
numpy restatement of tests/predict_ref.py.

Tolerances.  TOL_L = 10 x the floor of tests/test_predict_ref.py (the worst |dense - Gamma form| / max(1, |l|) over 2000 random
curves, measured again here by the same function): the margin is for the different summation order and is not tuned against the
kernel.  A log-density is held within TOL_L max(1, max |l|); a weight's relative error is bounded by twice the error of l, so
memberships and ess / J are held within 4 TOL_L max(1, max |l|).  TOL_RULE = 10 x the floor of the stage rule (float64 against
np.longdouble on the same inputs): the proposals are held against the rule applied to the device's own previous-stage samples with the
device's own l at those samples, which the deterministic hook (z_samples, one sample a call) returns bit for bit -- the rule is then
all that differs."""
import math
import re

import numpy as np
import pytest

import oracle_lib as O
import predict_ref as R
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

K, M, NTRAIN, NNEW, NCH, T = 3, 2, 24, 7, 2, 5


@pytest.fixture(scope="module")
def tol():
    floor_l, _ = R.ell_floor()
    floor_rule = R.rule_floor()
    print(f"floors: l {floor_l:.3e}, stage rule {floor_rule:.3e}")
    return {"l": 10.0 * floor_l, "rule": 10.0 * floor_rule}


def _chains(smp, cov=False):
    names = ["nu", "Phi", "sigma_sq", "pi", "alpha_3", "Z"] + (["eta", "xi"] if cov else [])
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
    """curve i of the simulation cut down to lengths[i] of its points"""
    ts, ys, Bs = [], [], []
    for i, ln in enumerate(lengths):
        keep = np.sort(rng.choice(len(sim["t"][i]), size=int(ln), replace=False))
        ts.append(sim["t"][i][keep]); ys.append(sim["y"][i][keep]); Bs.append(sim["B"][i][keep])
    return ts, ys, Bs


@pytest.fixture(scope="module")
def base():
    """24 training curves and 7 new ones of 1 .. 40 points (one of each with a single point), K = 3, M = 2, cubic splines with P = 8,
    2 chains x 5 slots after a short run"""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=NTRAIN + NNEW, M=M, sigma_sq=0.01, seed=41, K=K)
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 41, size=NTRAIN + NNEW)
    lengths[5], lengths[NTRAIN + 2], lengths[NTRAIN + 4] = 1, 1, 40
    ts, ys, Bs = _ragged(sim, rng, lengths)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, ys[:NTRAIN], ts[:NTRAIN], sim["internal_knots"], sim["boundary_knots"], n_chains=NCH)
    _start(smp, 7)
    d = dict(smp=smp, chains=_chains(smp), t=ts, y=ys, B=Bs, tn=ts[NTRAIN:], yn=ys[NTRAIN:], Bn=Bs[NTRAIN:], sim=sim)
    yield d
    smp.close()


def _zs(rng, C, S, J, Kc):
    z = rng.dirichlet(np.full(Kc, 0.8), size=(C, S, J))
    z[0, 0, 0, 0] = R.TINY                       # an entry at the clamp
    return np.ascontiguousarray(np.maximum(z, R.TINY))


def _ells(B, y, chains, zs_of, first=0, S=None, x=None, cadj=False):
    """l[q][s] (J,) of one curve by the dense form at the samples zs_of(q, s) (J, K)"""
    out = []
    for q, ch in enumerate(chains):
        S_ = (ch["sigma_sq"].shape[-1] - first) if S is None else S
        out.append([R.ell_dense_batch(B, y, _theta(ch, first + s, x, cadj), zs_of(q, s), float(ch["sigma_sq"][first + s])) for s in range(S_)])
    return out


def _check_last_stage(got, r, B, y, chains, tol, zs_of, prop_of=None, x=None, cadj=False, first=0, label=""):
    """lpd_trace, Z_trace and ess_trace of new curve r against the reference on the samples zs_of(q, s) (proposal prop_of(q, s), None:
    the prior); returns the per-draw reference dicts [q][s]"""
    ells = _ells(B, y, chains, zs_of, first, got["lpd_trace"].shape[2], x, cadj)
    refs = []
    for q, ch in enumerate(chains):
        refs.append([])
        for s in range(got["lpd_trace"].shape[2]):
            z = zs_of(q, s)
            prior = ch["alpha_3"][first + s] * ch["pi"][:, first + s]
            lw = R.log_weights(ells[q][s], z, prior, None if prop_of is None else prop_of(q, s))
            ref = R.stage(lw, z)
            scale = max(1.0, np.abs(ells[q][s]).max())
            J = len(lw)
            e_l = abs(got["lpd_trace"][r, q, s] - ref["lpd"])
            e_z = np.abs(got["Z_trace"][r, q, s] - ref["m"]).max()
            e_e = abs(got["ess_trace"][r, q, s] - ref["ess"]) / J
            print(f"{label} curve {r} chain {q} slot {s}: |lpd| err {e_l:.2e} (bound {tol['l'] * scale:.2e}), Z {e_z:.2e}, ess / J {e_e:.2e} "
                  f"(bound {4 * tol['l'] * scale:.2e}); max |l| {scale:.3g}")
            assert e_l <= tol["l"] * scale and e_z <= 4 * tol["l"] * scale and e_e <= 4 * tol["l"] * scale, label
            ref["scale"] = scale
            refs[-1].append(ref)
    return refs


@pytest.mark.parametrize("J", [37, 300])
def test_given_samples_against_the_dense_reference(base, tol, J):
    smp = base["smp"]
    zs = _zs(np.random.default_rng(J), NCH, T, J, K)
    got = smp.predict(base["yn"], base["tn"], n_samples=J, n_stages=1, trace=True, z_samples=zs)
    assert got["lpd_trace"].shape == (NNEW, NCH, T) and got["Z_trace"].shape == (NNEW, NCH, T, K) and got["proposal"].shape == (NNEW, NCH, T, 1, K)
    for r in range(NNEW):
        _check_last_stage(got, r, base["Bn"][r], base["yn"][r], base["chains"], tol, lambda q, s: zs[q, s], label=f"J={J}")
    for q, ch in enumerate(base["chains"]):
        np.testing.assert_array_equal(got["proposal"][:, q, :, 0, :], np.broadcast_to((ch["alpha_3"] * ch["pi"]).T, (NNEW, T, K)))
    assert np.all(got["ess_mean"] >= got["ess_min"]) and np.all(got["ess_min"] >= 1.0 - 1e-9)
    assert got["elpd"] == float(np.sum(got["lpd"])) and got["n_samples"] == J and got["n_stages"] == 1


def test_own_memberships_reproduce_curve_loglik(base, tol):
    """new curve = training curve i, one sample = the draw's own Z_i.: the density Sampler.curve_loglik evaluates"""
    smp = base["smp"]
    ll = smp.curve_loglik()
    for i in range(NNEW):
        zs = np.ascontiguousarray(np.stack([ch["Z"][i].T for ch in base["chains"]])[:, :, None, :])      # (C, S, 1, K)
        got = smp.predict([base["y"][i]], [base["t"][i]], n_samples=1, n_stages=1, trace=True, z_samples=zs)
        err = np.abs(got["lpd_trace"][0] - ll[i])
        bound = 2 * tol["l"] * np.maximum(1.0, np.abs(ll[i]))
        print(f"curve {i}: worst err {err.max():.2e}, bound {bound.min():.2e}")
        assert np.all(err <= bound)
        assert np.allclose(got["ess_trace"], 1.0, rtol=0, atol=1e-15) and np.array_equal(got["Z_trace"][0], zs[:, :, 0, :])


def _device_ell(smp, y, t, zj):
    """l of one curve at zj (C, S, K) for every draw, from the device by the deterministic hook"""
    return smp.predict([y], [t], n_samples=1, n_stages=1, trace=True, z_samples=np.ascontiguousarray(zj[:, :, None, :]))["lpd_trace"][0]


def test_three_stages_against_the_reference_rule(base, tol):
    smp = base["smp"]
    J, RS = 37, 3
    got = smp.predict(base["yn"], base["tn"], n_samples=J, n_stages=RS, seed=11, trace=True, return_samples=True)
    smpl, prop = got["samples"], got["proposal"]
    assert smpl.shape == (NNEW, NCH, T, RS, J, K) and np.all(smpl >= R.TINY) and np.allclose(smpl.sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    worst = 0.0
    for r in (0, 2, 5):          # (2: the curve of a single point)
        for st in range(RS - 1):
            ell = np.stack([_device_ell(smp, base["yn"][r], base["tn"][r], smpl[r, :, :, st, j, :]) for j in range(J)], axis=-1)   # (C, S, J)
            for q, ch in enumerate(base["chains"]):
                for s in range(T):
                    prior = ch["alpha_3"][s] * ch["pi"][:, s]
                    z = smpl[r, q, s, st]
                    lw = R.log_weights(ell[q, s], z, prior, None if st == 0 else prop[r, q, s, st])
                    nxt = R.stage(lw, z)["next"]
                    err = np.max(np.abs(prop[r, q, s, st + 1] - nxt) / np.maximum(1.0, np.abs(nxt)))
                    worst = max(worst, err)
                    assert err <= tol["rule"], (r, st, q, s, err, tol["rule"])
    print(f"proposals: worst relative error {worst:.2e}, bound {tol['rule']:.2e}")
    q_ref, scales = np.zeros((NNEW, NCH, T, K)), np.zeros(NNEW)
    for r in range(NNEW):
        refs = _check_last_stage(got, r, base["Bn"][r], base["yn"][r], base["chains"], tol, lambda q, s: smpl[r, q, s, RS - 1],
                                 lambda q, s: prop[r, q, s, RS - 1], label="R=3")
        q_ref[r] = [[ref["q"] for ref in row] for row in refs]
        scales[r] = max(ref["scale"] for row in refs for ref in row)
    _check_pooled(got, q_ref, scales, tol)


def _check_pooled(got, q_ref, scales, tol):
    """the pooled results against the traces; Z_sd takes the reference's q of every draw, whose weights carry up to 4 TOL_L max |l|"""
    m = got["lpd"].shape[0]
    for r in range(m):
        Kc = got["Z_trace"].shape[-1]
        ref = R.pooled(got["lpd_trace"][r].reshape(-1), got["ess_trace"][r].reshape(-1), got["Z_trace"][r].reshape(-1, Kc), q_ref[r].reshape(-1, Kc))
        for k, g in (("lpd", got["lpd"][r]), ("Z_mean", got["Z_mean"][r]), ("ess_mean", got["ess_mean"][r]), ("ess_min", got["ess_min"][r])):
            assert np.all(np.abs(g - ref[k]) <= 1e-12 * np.maximum(1.0, np.abs(ref[k]))), k      # sums of N = 10 terms in another order
        # held as variances: the square root near 0 has no bounded error
        assert np.all(np.abs(got["Z_sd"][r] ** 2 - ref["Z_sd"] ** 2) <= 4 * tol["l"] * scales[r] + 1e-12), "Z_sd"
    assert abs(got["se_elpd"] - math.sqrt(m * np.var(got["lpd"]))) < 1e-12


def test_three_stages_with_more_samples_than_lanes(base, tol):
    """J = 300: the second pass of the lanes in a staged run"""
    smp = base["smp"]
    J, RS = 300, 3
    got = smp.predict(base["yn"][:3], base["tn"][:3], n_samples=J, n_stages=RS, seed=5, trace=True, return_samples=True)
    smpl, prop = got["samples"], got["proposal"]
    for r in range(3):
        _check_last_stage(got, r, base["Bn"][r], base["yn"][r], base["chains"], tol, lambda q, s: smpl[r, q, s, RS - 1],
                          lambda q, s: prop[r, q, s, RS - 1], label="J=300 R=3")
    # the later stages have moved towards the posterior
    assert np.median(got["ess_trace"]) > np.median(smp.predict(base["yn"][:3], base["tn"][:3], n_samples=J, n_stages=1, seed=5, trace=True)["ess_trace"])


def test_sampling_law():
    """alpha_3 pi = (0.3, 1.2, 2.5), a shape below 1 among them: the moments of J = 4096 prior samples"""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=6, M=M, sigma_sq=0.01, seed=5, K=K)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=1)
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"])
    smp.init_state(1, 3)
    a3, pi = 4.0, np.array([0.075, 0.3, 0.625])
    smp.set_state(pi=pi, alpha_3=np.array([a3]))
    smp.run(bf.sampler.U_LOGLIK, 1, seed=1)
    assert np.array_equal(smp.get_chain("pi")[:, 0], pi) and smp.get_chain("alpha_3")[0] == a3
    J = 4096
    got = smp.predict([sim["y"][0][:9]], [sim["t"][0][:9]], n_samples=J, n_stages=1, seed=77, trace=True, return_samples=True)
    z = got["samples"][0, 0, 0, 0]
    assert z.shape == (J, K) and np.all(z >= R.TINY) and np.all(np.isfinite(np.log(z)))
    se = np.sqrt(pi * (1 - pi) / (a3 + 1) / J)
    print("means", z.mean(axis=0), "pi", pi, "se", se, "variances", z.var(axis=0), "expected", pi * (1 - pi) / (a3 + 1))
    assert np.all(np.abs(z.mean(axis=0) - pi) <= 5 * se)
    assert np.all(np.abs(z.var(axis=0) / (pi * (1 - pi) / (a3 + 1)) - 1.0) <= 0.25)
    np.testing.assert_array_equal(got["proposal"][0, 0, 0, 0], a3 * pi)
    smp.close()


def _bits(d, keys):
    return {k: np.asarray(d[k]).tobytes() for k in keys}


ALL_KEYS = ("lpd", "Z_mean", "Z_sd", "ess_mean", "ess_min", "lpd_trace", "ess_trace", "Z_trace", "proposal", "samples")


def test_bits_repeat_chunks_subsets_and_perm(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    kw = dict(n_samples=37, n_stages=3, seed=9, trace=True, return_samples=True)
    one = smp.predict(base["yn"], base["tn"], **kw)
    assert _bits(smp.predict(base["yn"], base["tn"], **kw), ALL_KEYS) == _bits(one, ALL_KEYS)
    # several chunks, from the refusal's own figures
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict.*'max_workspace_bytes'") as ei:
        smp.predict(base["yn"], base["tn"], max_workspace_bytes=1, **kw)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    few = smp.predict(base["yn"], base["tn"], max_workspace_bytes=shared + 3 * per_curve, **kw)
    assert _bits(few, ALL_KEYS) == _bits(one, ALL_KEYS)
    assert smp.timing("predict")[1] == 6 and smp.timing("predict_stats")[1] == 1          # three chunks of k_predict and k_predict_pool
    # the first curves of the call alone: the same positions, the same variates
    head = smp.predict(base["yn"][:3], base["tn"][:3], **kw)
    for k in ALL_KEYS:
        assert np.asarray(head[k]).tobytes() == np.asarray(one[k][:3]).tobytes(), k
    # another order: the variates go with the position in the call, the curve's own results with the curve once the samples are given
    sel = [4, 0, 2]
    moved = smp.predict([base["yn"][i] for i in sel], [base["tn"][i] for i in sel], **kw)
    assert moved["samples"][:, :, :, 0].tobytes() == one["samples"][:3, :, :, 0].tobytes()
    zs = _zs(np.random.default_rng(1), NCH, T, 37, K)
    hook = smp.predict(base["yn"], base["tn"], n_samples=37, n_stages=1, trace=True, z_samples=zs)
    hook_sel = smp.predict([base["yn"][i] for i in sel], [base["tn"][i] for i in sel], n_samples=37, n_stages=1, trace=True, z_samples=zs)
    for k in ("lpd", "Z_mean", "Z_sd", "ess_mean", "ess_min", "lpd_trace", "ess_trace", "Z_trace"):
        assert np.asarray(hook_sel[k]).tobytes() == np.ascontiguousarray(hook[k][sel]).tobytes(), k
    # a constant relabelling permutes the membership columns and nothing else
    p = np.array([2, 0, 1], dtype=np.int32)
    relab = smp.predict(base["yn"], base["tn"], perm=np.broadcast_to(p, (NCH, T, K)), **kw)
    for k in ("Z_mean", "Z_sd", "Z_trace"):
        assert np.ascontiguousarray(relab[k]).tobytes() == np.ascontiguousarray(one[k][..., p]).tobytes(), k
    for k in ("lpd", "ess_mean", "ess_min", "lpd_trace", "ess_trace", "proposal", "samples"):
        assert relab[k].tobytes() == one[k].tobytes(), k
    bad = np.zeros((NCH, T, K), dtype=np.int32)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'perm' of chain 0, slot 0 is not a permutation"):
        smp.predict(base["yn"], base["tn"], perm=bad, **kw)


def test_state_and_run_do_not_see_a_predict(base):
    import bayesfmmm_amd as bf
    from gpu_parity import STATE_NAMES
    outs = []
    for with_predict in (False, True):
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, base["y"][:NTRAIN], base["t"][:NTRAIN], base["sim"]["internal_knots"], base["sim"]["boundary_knots"], n_chains=NCH)
        for q in range(NCH):
            smp.select_chain(q)
            smp.init_state(1, 7, chain=q)
        smp.select_chain(0)
        smp.run(bf.SWEEP_WARM, 3, seed=7)
        if with_predict:
            smp.predict(base["yn"], base["tn"], n_samples=37, n_stages=2, n_slots=3)
        state = []
        for q in range(NCH):
            smp.select_chain(q)
            state.append([smp.get_state(nm).tobytes() for nm in STATE_NAMES])
        smp.select_chain(0)
        smp.run(bf.SWEEP_WARM, T - 3, first_iter=3, seed=7)
        for q in range(NCH):
            smp.select_chain(q)
            state.append([smp.get_state(nm).tobytes() for nm in STATE_NAMES] + [smp.get_chain(nm).tobytes() for nm in ("nu", "Phi", "Z", "pi", "sigma_sq", "loglik")])
        outs.append(state)
        smp.close()
    assert outs[0] == outs[1]


def _check_shape(smp, y_new, B_new, tol, label, cov=False, X_new=None, cadj=False, **inputs):
    """one given-samples call (J = 37, R = 1) and one staged call (R = 2) of a sampler of another shape against the dense reference"""
    chains = _chains(smp, cov)
    Kc, C_, S_ = smp.K, smp.n_chains, smp.T
    zs = _zs(np.random.default_rng(2), C_, S_, 37, Kc)
    got = smp.predict(y_new, n_samples=37, n_stages=1, trace=True, z_samples=zs, X_new=X_new, **inputs)
    for r in range(len(B_new)):
        x = None if X_new is None else X_new[r]
        _check_last_stage(got, r, B_new[r], np.asarray(y_new[r], dtype=np.float64), chains, tol, lambda q, s: zs[q, s], x=x, cadj=cadj, label=label)
    got = smp.predict(y_new, n_samples=37, n_stages=2, seed=3, trace=True, return_samples=True, X_new=X_new, **inputs)
    smpl, prop = got["samples"], got["proposal"]
    q_ref, scales = np.zeros((len(B_new), C_, S_, Kc)), np.zeros(len(B_new))
    for r in range(len(B_new)):
        x = None if X_new is None else X_new[r]
        refs = _check_last_stage(got, r, B_new[r], np.asarray(y_new[r], dtype=np.float64), chains, tol, lambda q, s: smpl[r, q, s, 1],
                                 lambda q, s: prop[r, q, s, 1], x=x, cadj=cadj, label=label + " R=2")
        q_ref[r] = [[ref["q"] for ref in row] for row in refs]
        scales[r] = max(ref["scale"] for row in refs for ref in row)
    _check_pooled(got, q_ref, scales, tol)


@pytest.mark.parametrize("Kc,Mc,P", [(3, 2, 5), (8, 1, 8), (3, 6, 8), (2, 2, 33)])
def test_multivariate_shapes(tol, Kc, Mc, P):
    """P = 5; K (M + 1) = 16 exactly; 21, padded to 32; P = 33"""
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(P)
    Y = rng.standard_normal((NTRAIN + 3, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=Kc, n_eigen=Mc, tot_mcmc_iters=3)
    smp = bf.Sampler(cfg, Y[:NTRAIN], n_chains=2)
    _start(smp, 17)
    _check_shape(smp, Y[NTRAIN:], [np.eye(P)] * 3, tol, f"multivariate K={Kc} M={Mc} P={P}")
    smp.close()


def test_covariates_with_covariance_adjustment(tol):
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=NTRAIN + 3, M=M, sigma_sq=0.01, seed=33, K=K, D=2)
    rng = np.random.default_rng(8)
    ts, ys, Bs = _ragged(sim, rng, rng.integers(2, 41, size=NTRAIN + 3))
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=3)
    smp = bf.Sampler(cfg, ys[:NTRAIN], ts[:NTRAIN], sim["internal_knots"], sim["boundary_knots"], n_chains=2)
    smp.set_covariates(sim["X"][:NTRAIN], covariance_adj=True)
    _start(smp, 5, S.SWEEP_WARM | S.COV_MEAN | S.COV_XI)
    _check_shape(smp, ys[NTRAIN:], Bs[NTRAIN:], tol, "covariates D=2", cov=True, X_new=sim["X"][NTRAIN:], cadj=True, time_new=ts[NTRAIN:])
    smp.close()


def test_tensor_product_basis_on_the_wide_band(tol):
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    sim = simulate_tensor(NTRAIN + 3, 2, 2, [1, 2], [1, 1], seed=12, n_pts=30)      # 3 x 4 = 12 basis functions, band 6
    assert sim["P"] == 12 and sim["band"] == 6
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=2, n_eigen=2, basis_degree=2, tot_mcmc_iters=3)
    smp = bf.Sampler(cfg, sim["y"][:NTRAIN], basis=sim["B"][:NTRAIN], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=2)
    _start(smp, 9)
    _check_shape(smp, sim["y"][NTRAIN:], sim["B"][NTRAIN:], tol, "tensor 3 x 4", basis_new=sim["B"][NTRAIN:])
    assert smp.timing("predict_stats")[1] == 0
    smp.close()


def test_refusals_by_name(base):
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    yn, tn = base["yn"], base["tn"]
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'zs' takes the place of the stage-0 samples: 'n_stages' must be 1, got 2"):
        smp.predict(yn, tn, n_samples=4, n_stages=2, z_samples=_zs(np.random.default_rng(0), NCH, T, 4, K))
    # the RNG index, reached without any allocation that grows with J
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict: n_new x n_stages x n_samples x K = 7 x 3 x 2000000000 x 3 exceeds the 4294967296"):
        smp.predict(yn, tn, n_samples=2_000_000_000, n_stages=3)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict: 'max_workspace_bytes' below the \d+ bytes one curve needs"):
        smp.predict(yn, tn, max_workspace_bytes=64)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict: 'samples' of one curve .* need \d+ bytes"):
        smp.predict(yn, tn, n_samples=300, return_samples=True, max_workspace_bytes=100_000)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: new curve 1 is empty"):
        smp.predict([yn[0], yn[1][:0]], [tn[0], tn[1][:0]])
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'n_samples' must be at least 1"):
        smp.predict(yn, tn, n_samples=0)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'n_stages' must be at least 1"):
        smp.predict(yn, tn, n_stages=0)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'n_slots' out of range"):
        smp.predict(yn, tn, first_slot=2, n_slots=T)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict: k_predict: the tables of a draw .* above the limit of 163840"):
        smp.predict(yn, tn, n_samples=8192)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'X' is given but the sampler has no covariates"):
        smp.predict(yn, tn, X_new=np.zeros((NNEW, 2)))
    assert smp.predict([], []) ["lpd"].shape == (0,)
    # a covariate sampler without X_new
    sim = base["sim"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=2)
    cov = bf.Sampler(cfg, base["y"][:NTRAIN], base["t"][:NTRAIN], sim["internal_knots"], sim["boundary_knots"])
    cov.set_covariates(np.random.default_rng(2).standard_normal((NTRAIN, 2)))
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict: 'X' is null but the sampler has 2 covariates"):
        cov.predict(yn, tn)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict: 'X'\[1, 0\] is not finite"):
        X = np.zeros((NNEW, 2)); X[1, 0] = np.nan
        cov.predict(yn, tn, X_new=X)
    cov.close()
