"""The Laplace mixture proposal of Sampler.predict on the device (bfmmm_chain_predict_laplace) against the numpy
restatement of tests/predict_laplace_ref.py.

Tolerances.  Given the device's own components and eta samples, the restatement recomputes lw = g - log q with the dense l, so what
differs is l in its Gamma form (the floor of tests/test_gpu_predict.py, measured again here) and log q in float64 (the floor of
tests/test_predict_laplace_ref.py, measured again here): TOL_L = 10 x their sum, held against max(1, max |g|, max |log q|) for
lpd and 4 TOL_L of it for the memberships and ess / J, as DESIGN.md 7m builds them.  The modes are held by a property, not by the
search's path: under the reference's long-double derivatives -H is positive definite at every reported component and the Newton
decrement is below 1e-5 (ten times the rule's threshold) plus the float64 floor of the decrement."""
import re

import numpy as np
import pytest

import oracle_lib as O
import predict_laplace_ref as Lr
import predict_ref as R
import test_gpu_predict as TP
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

K, M, NTRAIN, NNEW, NCH, T = 3, 2, 24, 5, 2, 3
UPD_PREDICT_LAPLACE = 45
LD = np.longdouble


@pytest.fixture(scope="module")
def tol():
    floor_l, _ = R.ell_floor()
    fl = Lr.derivative_floor()
    print(f"floors: l {floor_l:.3e}, log q {fl['logq']:.3e}, decrement {fl['dec']:.3e}")
    return {"l": 10.0 * (floor_l + fl["logq"]), "dec": fl["dec"]}


@pytest.fixture(scope="module")
def base():
    """test_gpu_predict.py's base fixture with 5 new curves and 2 chains x 3 slots"""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=NTRAIN + NNEW, M=M, sigma_sq=0.01, seed=41, K=K)
    rng = np.random.default_rng(3)
    lengths = rng.integers(2, 41, size=NTRAIN + NNEW)
    lengths[NTRAIN + 2], lengths[NTRAIN + 4] = 1, 40
    ts, ys, Bs = TP._ragged(sim, rng, lengths)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, ys[:NTRAIN], ts[:NTRAIN], sim["internal_knots"], sim["boundary_knots"], n_chains=NCH)
    TP._start(smp, 7)
    yield dict(smp=smp, chains=TP._chains(smp), t=ts, y=ys, B=Bs, tn=ts[NTRAIN:], yn=ys[NTRAIN:], Bn=Bs[NTRAIN:], sim=sim)
    smp.close()


def _components(row, Kc):
    """the component slots of one pair as predict_laplace_ref's dicts, slot order kept (a slot that is all zero is unused)"""
    d = Kc - 1
    out = []
    for c, v in enumerate(row):
        if c > 0 and not np.any(v):
            continue
        out.append({"slot": c, "eta": v[:d].copy(), "L": Lr.unpack_L(v[d:d + d * (d + 1) // 2], d), "g": v[-2], "J": int(v[-1])})
    return out


def _check_call(got, y_new, B_new, chains, tol, J, X_new=None, cadj=False, label=""):
    """every (curve, chain, slot) of a traced call: the component rule's invariants, the modes under long double, and lpd, ess and
    memberships against the restatement on the device's own components and samples with the dense l; then the pooled arrays"""
    m, C_, S_ = got["lpd_trace"].shape
    Kc = got["Z_trace"].shape[-1]
    assert got["components"].shape == (m, C_, S_, Kc + 2, (Kc - 1) + (Kc - 1) * Kc // 2 + 2) and got["eta_samples"].shape == (m, C_, S_, J, Kc - 1)
    assert got["n_modes"].dtype == np.int32 and np.all(got["n_modes"] >= 1) and np.all(got["n_modes"] <= Kc + 1)
    q_ref, scales, worst_dec = np.zeros((m, C_, S_, Kc)), np.zeros(m), 0.0
    for r in range(m):
        x = None if X_new is None else X_new[r]
        for q, ch in enumerate(chains):
            for s in range(S_):
                case = Lr.make_case(B_new[r], np.asarray(y_new[r], dtype=np.float64), TP._theta(ch, s, x, cadj), float(ch["sigma_sq"][s]),
                                    ch["alpha_3"][s] * ch["pi"][:, s])
                comps = _components(got["components"][r, q, s], Kc)
                assert comps[0]["slot"] == 0 and [c["slot"] for c in comps] == list(range(len(comps))) and len(comps) - 1 == got["n_modes"][r, q, s]
                assert sum(c["J"] for c in comps) == J and comps[0]["J"] == max(1, J // 16) and all(c["J"] >= 0 for c in comps)
                # the condition these checks lean on: the reference's own search finds a mode for the pair too
                assert any(Lr.search(case, e)["conv"] for e in Lr.starts(case["alpha"])), (label, r, q, s)
                c0, L0 = Lr.defensive(case["alpha"])
                assert np.allclose(comps[0]["eta"], c0, rtol=0, atol=1e-12) and np.allclose(comps[0]["L"], L0, rtol=1e-12, atol=0)
                for c in comps[1:]:
                    g, grad, H = Lr.evaluate(case, c["eta"].astype(LD), LD)
                    dec = Lr.decrement(grad, H)
                    assert dec is not None, (label, r, q, s, c["slot"], "-H is not positive definite")
                    worst_dec = max(worst_dec, float(dec))
                    assert dec < 1e-5 + tol["dec"] * max(1.0, float(dec)), (label, r, q, s, c["slot"], float(dec))
                    assert abs(c["g"] - float(g)) <= tol["l"] * max(1.0, abs(float(g)))
                    Sg = np.linalg.inv(-np.asarray(H, dtype=np.float64))
                    assert np.allclose(c["L"] @ c["L"].T, Sg, rtol=0, atol=1e-6 * np.abs(Sg).max()), "L L' is not (-H)^-1"
                    assert all(np.max(np.abs(c["eta"] - o["eta"])) >= Lr.SAME for o in comps[1:c["slot"]])
                eta = got["eta_samples"][r, q, s]
                active = [c for c in comps if c["J"] > 0]
                gd = Lr.g_dense(case, eta)
                ref = Lr.weigh(gd, eta, active)
                scale = max(1.0, np.abs(gd).max(), np.abs(gd - ref["lw"]).max())
                e_l = abs(got["lpd_trace"][r, q, s] - ref["lpd"])
                e_z = np.abs(got["Z_trace"][r, q, s] - ref["m"]).max()
                e_e = abs(got["ess_trace"][r, q, s] - ref["ess"]) / J
                print(f"{label} curve {r} chain {q} slot {s}: J_c {[c['J'] for c in comps]}, ess {got['ess_trace'][r, q, s]:.1f}, |lpd| err {e_l:.2e} "
                      f"(bound {tol['l'] * scale:.2e}), Z {e_z:.2e}, ess / J {e_e:.2e} (bound {4 * tol['l'] * scale:.2e})")
                assert e_l <= tol["l"] * scale and e_z <= 4 * tol["l"] * scale and e_e <= 4 * tol["l"] * scale, label
                q_ref[r, q, s] = ref["q"]
                scales[r] = max(scales[r], scale)
    print(f"{label}: largest long-double Newton decrement at a reported mode {worst_dec:.2e}")
    TP._check_pooled(got, q_ref, scales, tol)
    assert np.allclose(got["n_modes_mean"], got["n_modes"].reshape(m, -1).mean(axis=1)) and got["n_samples"] == J and got["n_stages"] == 1


@pytest.mark.parametrize("J", [37, 300])
def test_against_the_restatement_on_the_devices_own_mixture(base, tol, J):
    got = base["smp"].predict(base["yn"], base["tn"], n_samples=J, seed=11, trace=True, proposal="laplace")
    _check_call(got, base["yn"], base["Bn"], base["chains"], tol, J, label=f"J={J}")
    assert "proposal" not in got and "samples" not in got


def test_samples_follow_the_variates_component_by_component(base):
    """eta_j = eta_c + L_c eps_j sqrt(4 / chi2_j) from the counter's own normals and uniforms at index (r J + j)(d + 2) + i, the samples
    of a component contiguous and in component order"""
    J, d, seed = 37, K - 1, 11
    got = base["smp"].predict(base["yn"], base["tn"], n_samples=J, seed=seed, trace=True, proposal="laplace")
    for q in range(NCH):
        for s in range(T):
            nrm = O.fill(1, NNEW * J * (d + 2), seed=seed, chain=q, it=s, upd=UPD_PREDICT_LAPLACE).reshape(NNEW, J, d + 2)
            uni = O.fill(0, NNEW * J * (d + 2), seed=seed, chain=q, it=s, upd=UPD_PREDICT_LAPLACE).reshape(NNEW, J, d + 2)
            for r in range(NNEW):
                comps = _components(got["components"][r, q, s], K)
                owner = np.repeat(np.arange(len(comps)), [c["J"] for c in comps])
                assert len(owner) == J
                sc = np.sqrt(4.0 / (-2.0 * np.log(uni[r, :, d] * uni[r, :, d + 1])))
                want = np.stack([comps[c]["eta"] + (comps[c]["L"] @ nrm[r, j, :d]) * sc[j] for j, c in enumerate(owner)])
                assert np.allclose(got["eta_samples"][r, q, s], want, rtol=1e-12, atol=1e-12), (r, q, s)


def test_sampling_law():
    """one pair with J = 4096: the share of standardised coordinates L_c^-1 (eta - eta_c) inside the t4 quartile 0.7407 is 1 / 2 within
    four binomial standard deviations"""
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=6, M=M, sigma_sq=0.01, seed=5, K=K)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=1)
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"])
    smp.init_state(1, 3)
    smp.run(bf.sampler.U_LOGLIK, 1, seed=1)
    J = 4096
    got = smp.predict([sim["y"][0][:9]], [sim["t"][0][:9]], n_samples=J, seed=77, trace=True, proposal="laplace")
    comps = _components(got["components"][0, 0, 0], K)
    owner = np.repeat(np.arange(len(comps)), [c["J"] for c in comps])
    eta = got["eta_samples"][0, 0, 0]
    xs = np.concatenate([np.linalg.solve(c["L"], (eta[owner == i] - c["eta"]).T).T.reshape(-1) for i, c in enumerate(comps) if c["J"] > 0])
    share = np.mean(np.abs(xs) < 0.7407)
    print(f"J_c {[c['J'] for c in comps]}: share inside the quartile {share:.4f} of {xs.size} coordinates, ess {got['ess_trace'][0, 0, 0]:.0f}")
    assert xs.size == J * (K - 1) and abs(share - 0.5) <= 4 * np.sqrt(0.25 / xs.size)
    smp.close()


LAP_KEYS = ("lpd", "Z_mean", "Z_sd", "ess_mean", "ess_min", "lpd_trace", "ess_trace", "Z_trace", "n_modes", "components", "eta_samples")


def test_bits_repeat_chunks_subsets_and_perm(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    kw = dict(n_samples=37, seed=9, trace=True, proposal="laplace")
    one = smp.predict(base["yn"], base["tn"], **kw)
    assert TP._bits(smp.predict(base["yn"], base["tn"], **kw), LAP_KEYS) == TP._bits(one, LAP_KEYS)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict_laplace.*'max_workspace_bytes'") as ei:
        smp.predict(base["yn"], base["tn"], max_workspace_bytes=1, **kw)
    shared, per_curve = (int(v) for v in re.search(r"\((\d+) shared by all curves \+ (\d+) per curve\)", str(ei.value)).groups())
    few = smp.predict(base["yn"], base["tn"], max_workspace_bytes=shared + 2 * per_curve, **kw)
    assert TP._bits(few, LAP_KEYS) == TP._bits(one, LAP_KEYS)
    assert smp.timing("predict_laplace")[1] == 6 and smp.timing("predict_stats")[1] == 1       # three chunks of k_predict_lap and k_predict_pool
    head = smp.predict(base["yn"][:3], base["tn"][:3], **kw)
    for k in LAP_KEYS:
        assert np.asarray(head[k]).tobytes() == np.asarray(one[k][:3]).tobytes(), k
    p = np.array([2, 0, 1], dtype=np.int32)
    relab = smp.predict(base["yn"], base["tn"], perm=np.broadcast_to(p, (NCH, T, K)), **kw)
    for k in ("Z_mean", "Z_sd", "Z_trace"):
        assert np.ascontiguousarray(relab[k]).tobytes() == np.ascontiguousarray(one[k][..., p]).tobytes(), k
    for k in ("lpd", "ess_mean", "ess_min", "lpd_trace", "ess_trace", "n_modes", "components", "eta_samples"):
        assert relab[k].tobytes() == one[k].tobytes(), k


def test_defaults_keep_their_bits_and_the_state_is_untouched(base):
    from gpu_parity import STATE_NAMES
    smp = base["smp"]
    E = base["Bn"][4][:5]

    def snapshot():
        a = smp.predict(base["yn"], base["tn"], n_samples=37, seed=4, trace=True, return_samples=True)
        b = smp.predict_fit(base["yn"][:2], E, base["tn"][:2], n_samples=37, seed=4, trace=True)
        c = smp.loo_marginal(n_samples=37, seed=4, trace=True)
        keys = lambda d: sorted(k for k, v in d.items() if isinstance(v, np.ndarray))
        out = [TP._bits(d, keys(d)) for d in (a, b, c)]
        for q in range(NCH):
            smp.select_chain(q)
            out.append([smp.get_state(nm).tobytes() for nm in STATE_NAMES] + [smp.get_chain(nm).tobytes() for nm in ("nu", "Phi", "Z", "pi", "sigma_sq")])
        smp.select_chain(0)
        return out

    before = snapshot()
    smp.predict(base["yn"], base["tn"], n_samples=37, seed=4, proposal="laplace")
    smp.loo_marginal(n_samples=37, seed=4, proposal="laplace")
    assert snapshot() == before


def _shape_case(smp, y_new, B_new, tol, label, cov=False, X_new=None, cadj=False, **inputs):
    chains = TP._chains(smp, cov)
    got = smp.predict(y_new, n_samples=37, seed=3, trace=True, proposal="laplace", X_new=X_new, **inputs)
    _check_call(got, y_new, B_new, chains, tol, 37, X_new=X_new, cadj=cadj, label=label)


@pytest.mark.parametrize("Kc,Mc,P", [(2, 2, 33), (3, 6, 8), (5, 3, 7), (8, 1, 8)])
def test_multivariate_shapes(tol, Kc, Mc, P):
    """K = 2 (one log-ratio); K (M + 1) = 21 padded to 32; K = 5 with the KT = 8 instance; K = 8, nine starts"""
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(P)
    Y = rng.standard_normal((NTRAIN + 4, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=Kc, n_eigen=Mc, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y[:NTRAIN], n_chains=2)
    TP._start(smp, 17)
    _shape_case(smp, Y[NTRAIN:], [np.eye(P)] * 4, tol, f"multivariate K={Kc} M={Mc} P={P}")
    smp.close()


def test_covariates_with_covariance_adjustment(tol):
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=NTRAIN + 4, M=M, sigma_sq=0.01, seed=33, K=K, D=2)
    rng = np.random.default_rng(8)
    ts, ys, Bs = TP._ragged(sim, rng, rng.integers(2, 41, size=NTRAIN + 4))
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, ys[:NTRAIN], ts[:NTRAIN], sim["internal_knots"], sim["boundary_knots"], n_chains=2)
    smp.set_covariates(sim["X"][:NTRAIN], covariance_adj=True)
    TP._start(smp, 5, S.SWEEP_WARM | S.COV_MEAN | S.COV_XI)
    _shape_case(smp, ys[NTRAIN:], Bs[NTRAIN:], tol, "covariates D=2", cov=True, X_new=sim["X"][NTRAIN:], cadj=True, time_new=ts[NTRAIN:])
    smp.close()


def test_tensor_product_basis_on_the_wide_band(tol):
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    sim = simulate_tensor(NTRAIN + 4, 2, 2, [1, 2], [1, 1], seed=12, n_pts=30)      # 3 x 4 = 12 basis functions, band 6
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=2, n_eigen=2, basis_degree=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"][:NTRAIN], basis=sim["B"][:NTRAIN], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=2)
    TP._start(smp, 9)
    _shape_case(smp, sim["y"][NTRAIN:], sim["B"][NTRAIN:], tol, "tensor 3 x 4", basis_new=sim["B"][NTRAIN:])
    smp.close()


def test_against_the_staged_dirichlet_on_sharp_curves():
    """predict_laplace_ref.sharp_fixture: 4 curves of 100 points, sigma^2 = 0.0002, the chain slots set to its 2 x 3 draws.  The staged
    Dirichlet (R = 3) of the restatement stays below half of J in the median there, whatever the seed (tests/test_predict_laplace_ref.py);
    the comparison is with the device's own staged call on the same 24 pairs, not with a number: the mixture's median ess exceeds it."""
    import bayesfmmm_amd as bf
    sim, draws = Lr.sharp_fixture()
    f = Lr.SHARP
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=f["K"], n_eigen=f["M"], basis_degree=3, tot_mcmc_iters=f["S"])
    smp = bf.Sampler(cfg, sim["y"], sim["t"], sim["internal_knots"], sim["boundary_knots"], n_chains=f["C"])
    for q in range(f["C"]):
        smp.select_chain(q)
        smp.init_state(1, 3, chain=q)
    for s in range(f["S"]):
        for q in range(f["C"]):
            d = draws[q][s]
            smp.select_chain(q)
            smp.set_state(nu=d["nu"], Phi=d["Phi"], sigma_sq=np.array([d["sigma_sq"]]), pi=d["pi"], alpha_3=np.array([d["alpha_3"]]))
        smp.select_chain(0)
        smp.run(bf.sampler.U_LOGLIK, 1, first_iter=s, seed=1)
    ch = TP._chains(smp)
    for q in range(f["C"]):
        for s in range(f["S"]):
            assert np.array_equal(ch[q]["nu"][..., s], draws[q][s]["nu"]) and ch[q]["sigma_sq"][s] == draws[q][s]["sigma_sq"]
    J = 256
    old = smp.predict(sim["y"], sim["t"], n_samples=J, n_stages=3, seed=2, trace=True)
    new = smp.predict(sim["y"], sim["t"], n_samples=J, seed=2, trace=True, proposal="laplace")
    print(f"median ess over {old['ess_trace'].size} pairs: staged Dirichlet {np.median(old['ess_trace']):.1f}, Laplace mixture {np.median(new['ess_trace']):.1f}; "
          f"least {old['ess_trace'].min():.1f} and {new['ess_trace'].min():.1f}; modes {new['n_modes'].reshape(-1)}")
    assert old["ess_trace"].size == 24 and new["ess_trace"].size == 24
    assert np.median(new["ess_trace"]) > np.median(old["ess_trace"])
    smp.close()


def test_refusals_by_name(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    yn, tn = base["yn"], base["tn"]
    with pytest.raises(ValueError, match="predict: 'n_stages' has no meaning with proposal='laplace'"):
        smp.predict(yn, tn, n_stages=2, proposal="laplace")
    with pytest.raises(ValueError, match="predict: 'z_samples' has no meaning with proposal='laplace'"):
        smp.predict(yn, tn, z_samples=np.full((NCH, T, 4, K), 1.0 / K), n_samples=4, proposal="laplace")
    with pytest.raises(ValueError, match="proposal must be 'dirichlet' or 'laplace'"):
        smp.predict(yn, tn, proposal="gauss")
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict_laplace: n_new x n_samples x \(K \+ 1\) = 5 x 2000000000 x 4 exceeds the 4294967296"):
        smp.predict(yn, tn, n_samples=2_000_000_000, proposal="laplace")
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_predict_laplace: k_predict_lap: the tables of a draw .* need \d+ bytes of LDS, above the limit of 163840"):
        smp.predict(yn, tn, n_samples=8192, proposal="laplace")
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_predict_laplace: 'n_samples' must be at least 1"):
        smp.predict(yn, tn, n_samples=0, proposal="laplace")
    assert smp.predict([], [], proposal="laplace")["lpd"].shape == (0,)
