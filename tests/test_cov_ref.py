"""CPU tests of tests/cov_ref.py: both float64 emulations of the eta / Xi block pass every bound on every case (and the constants
G_* are still 4 x what they show), every mutation of the kernel-order emulation is rejected by the check it was written for on a
named case at >= 10 x the bound, and the restated block agrees with the oracle's updateEta, updateXi, updateTauEta,
updateDeltaXi and updateGammaXi under the same keyed variates (1e-9), which pins the step order."""
import numpy as np
import pytest

import cov_ref as V
import curve_update_ref as R
import factor_ref as F
import oracle_lib as O

pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 here")

HYP = dict(beta_eta=O.HYPER_DEFAULTS["beta_eta"], nu_1=O.HYPER_DEFAULTS["nu_1"])
FULL = V.COV_MEAN | V.COV_XI
_cache = {}


def inputs(c):
    if c.name not in _cache:
        st, X, rec = V.case_state(c), R.case_X(c), R.host_rec(c)
        c0, g0 = V.host_c0(c, rec, st, X)
        rng = np.random.default_rng(11)
        gstd2 = rng.gamma(4.0, 1.0, size=c.K * c.D + c.K * c.M * c.D + c.K * c.D * c.P * c.M)
        _cache.clear()
        _cache[c.name] = (st, X, rec, c0, g0, V.normals(c), gstd2)
    return _cache[c.name]


def run(c, mask, beta, variant="kernel", mut=None):
    st, X, rec, c0, g0, z, gstd2 = inputs(c)
    emu = V.emulate(c, rec, st, X, c0, g0, mask, beta, z, gstd2, HYP, variant=variant, mut=mut)
    emu["sigma2"] = float(np.ravel(st["sigma_sq"])[0])
    return V.check_all(c, rec, st, X, c0, g0, mask, beta, emu, HYP, gstd2=gstd2)


def ratios(res):
    return dict(h2aa=res["h2aa"]["worst"], step=res["steps"]["worst"], cfull=res["final"]["worst"], gfull=res["final"]["worst_g"],
                rss=res["rss"]["worst"], tau=res["hyper"]["worst_tau"], delta=res["hyper"]["worst_delta"], gamma=res["hyper"]["worst_gamma"], C=res["factor"]["worst_C"], L=res["factor"]["worst_L"])


def runs_of(c):
    out = [(FULL, 1.0)]
    if c.name == "cubic_P30_D2-benign":
        out += [(V.COV_MEAN, 1.0), (V.COV_XI, 1.0), (0, 1.0), (FULL, 0.37)]
    return out


GNAMES = dict(h2aa="G_H", step="G_STEP", cfull="G_CF", gfull="G_GF", rss="G_RSS2", tau="G_TAU", delta="G_DELTA", gamma="G_GAMMA")


def _sweep_cases(judge):
    for c in V.CPU_CASES:
        for mask, beta in runs_of(c):
            for variant in ("kernel", "plain"):
                judge(c, mask, beta, variant, run(c, mask, beta, variant))


def test_emulations_pass_and_constants_hold(monkeypatch):
    """both emulations pass every bound on every case with the constants as they stand; then, with every G set to 1, the largest
    error / bound they show is what the constants were set from (and 4 x that is the constant)"""
    vac = [0.0, ""]

    def must_pass(c, mask, beta, variant, res):
        fails = [m for r in res.values() for m in r["fails"]]
        assert not fails, f"{variant} emulation, mask {mask:#x}, beta {beta}:\n" + "\n".join(fails[:8])
        for k in ("worst_C", "worst_L"):      # factor_ref's constants carry over unchanged
            assert res["factor"][k] <= 1.0
        if c.regime == "stiff":      # the smallest Cholesky pivot stays a factor 1000 above the kernels' 1e-12 decision
            print(f"{c.name}: kappa_s {res['factor']['kappa']:.3g}, smallest pivot ratio {res['factor']['rho']:.3g}")
            assert res["factor"]["rho"] >= 1e-9
        if c.empty is not None and mask & V.U_ETA:
            assert ("pinv", "eta") in res["factor"]["routes"] and ("pinv", "xi") not in res["factor"]["routes"]
        if res["steps"]["vacuous"] > vac[0]:
            vac[:] = [res["steps"]["vacuous"], c.name]

    _sweep_cases(must_pass)
    print(f"largest step bound / |delta|: {vac[0]:.3g} ({vac[1]})")
    assert vac[0] <= V.NONVACUOUS, vac
    G = {k: getattr(V, nm) for k, nm in GNAMES.items()}
    for nm in GNAMES.values():
        monkeypatch.setattr(V, nm, 1.0)
    worst = {v: {k: (0.0, "") for k in GNAMES} for v in ("kernel", "plain")}

    def measure(c, mask, beta, variant, res):
        for k, v in ratios(res).items():
            if k in GNAMES and v > worst[variant][k][0]:
                worst[variant][k] = (v, c.name)

    _sweep_cases(measure)
    for variant in worst:
        for k, (w, where) in worst[variant].items():
            print(f"largest error / (bound at G = 1), {k:6s} {variant:6s}: {w:.3g} ({where})")
    for k, meas in (("h2aa", V.MEASURED_H), ("step", V.MEASURED_STEP), ("cfull", V.MEASURED_CF), ("gfull", V.MEASURED_GF), ("rss", V.MEASURED_RSS2),
                    ("tau", V.MEASURED_TAU), ("delta", V.MEASURED_DELTA), ("gamma", V.MEASURED_GAMMA)):
        top = max(worst["kernel"][k][0], worst["plain"][k][0])
        assert top <= 1.02 * max(meas.values()), f"{k}: the emulations now show {top:.3g}, the constant was set from {meas}"
        assert 3.95 * max(meas.values()) <= G[k] <= 4.1 * max(meas.values()), f"{k}: G = {G[k]} is not 4 x {meas}"


@pytest.mark.parametrize("mut", sorted(V.MUTATIONS))
def test_mutation_is_rejected(mut):
    name, mask, beta, which = V.MUTATIONS[mut]
    c = V.BY_NAME[name]
    res = run(c, mask, beta, "kernel", mut=mut)
    r = res[which]
    if which == "wdir":
        assert r["fails"], f"{mut}: Wdir in the wrong direction order was accepted"
        return
    if mut == "rss_tail_nonzero":
        assert any("beyond" in m for m in r["fails"]), r["fails"]
        return
    key = {"factor": "worst_C", "final": "worst_g"}.get(which, "worst")
    print(f"{mut} on {name}: {which} error / bound {r[key]:.3g}")
    assert r[key] >= 10.0, f"{mut} on {name}: the {which} check sees only {r[key]:.3g} x its bound"
    assert r["fails"]


def test_restated_block_matches_the_oracle():
    """theta from the longdouble restatement of every step (each from the reference's OWN earlier steps), then tau_eta, delta_xi
    and gamma_xi from hyper_ref with the oracle's keyed standard gamma variates, against the oracle's updates"""
    c = V.BY_NAME["cubic_P30_D2-benign"]
    st, X, rec, _, _, _, _ = inputs(c)
    d = F.case_data(c)
    model = O.Model(d["y"], d["B"], c.K, c.M, X=X, Pmat=d["Pmat"])
    ch = O.Chain(model, 2)
    ch.set_slot0(nu=st["nu"], chi=st["chi"], Z=st["Z"], sigma=float(st["sigma_sq"][0]), Phi=st["Phi"], eta=st["eta"], xi=st["xi"],
                 tau_eta=st["tau_eta"], gamma_xi=st["gamma_xi"], delta_xi=st["delta_xi"], A_xi=st["A_xi"], delta=st["delta"], gamma=st["gamma"],
                 tau=st["tau"], pi=st["pi"], alpha3=float(st["alpha_3"][0]), A=st["A"])
    # the oracle's updates write slot `it` and read the current state of slot `it` for what they do not update: run them at it = 0
    O.updateEta(model, ch, 0, seed=V.SEED)
    tt = np.cumprod(st["delta_xi"], axis=1)
    O.updateXi(model, ch, 0, tt, seed=V.SEED)
    # the restatement: the whole block in longdouble from the oracle's own normals and G_i, s_i of the basis rows
    Gd = np.stack([B.T @ B for B in d["B"]]).astype(V.LD)
    sd = np.stack([B.T @ y for B, y in zip(d["B"], d["y"])]).astype(V.LD)
    W = V.wdir64(c, st, X).astype(V.LD)
    th, _ = R.theta_rows(c, st, X, c.M)
    u = np.einsum("ik,ikmp->imp", V._ld(st["Z"]), th[:, :, 1:])
    cc = np.einsum("ik,ikp->ip", V._ld(st["Z"]), th[:, :, 0]) + np.einsum("im,imp->ip", V._ld(st["chi"]), u)
    z = V.normals(c).astype(V.LD)
    f = 1 / V.LD(st["sigma_sq"][0])
    t0 = V.theta_of(c, st).astype(V.LD)
    for a in range(c.A2):
        Haa = np.einsum("i,ipq->pq", W[:, a] ** 2, Gd)
        Rf = F.inverse_ld(f * Haa + V.prior_ld(c, st, a))
        r = np.einsum("i,ip->p", W[:, a], sd - np.einsum("ipq,iq->ip", Gd, cc))
        new = Rf.C @ (f * (r + Haa @ t0[a])) + Rf.L @ z[a]
        j, mt, dd = V.dir2_of(c, a)
        got = ch.eta[:, dd, j, 0] if mt == 0 else ch.xi[:, dd, mt - 1, j, 0]
        assert np.abs(np.asarray(new, dtype=np.float64) - got).max() <= 1e-9 * max(1.0, np.abs(got).max()), (a, (j, mt, dd))
        cc = cc + np.outer(W[:, a], new - t0[a])
        t0[a] = new
    # the hyper parameters: standard gamma variates with k_cov_prep's shapes (the reference's integer divisions) and indices
    K, M, P, D = c.K, c.M, c.P, c.D
    hy = O.HYPER_DEFAULTS
    one = lambda upd, idx, shape: O.fill(2, idx + 1, seed=V.SEED, it=0, upd=upd, p1=shape, p2=1.0)[idx]      # noqa: E731
    g_tau = [one(17, e, hy["alpha_eta"] + P // 2) for e in range(K * D)]
    g_del = []
    for idx in range(K * M * D):      # (d K + k) M + i
        i, k, dd = idx % M, (idx // M) % K, idx // (M * K)
        g_del.append(one(19, idx, st["A_xi"][k, 0, dd] + P * M * 0.5 if i == 0 else st["A_xi"][k, 1, dd] + P * (M - i) * 0.5))
    g_gam = O.fill(2, K * D * P * M, seed=V.SEED, it=0, upd=22, p1=(hy["nu_1"] + 1) / 2, p2=1.0)
    hr = V.hyper_ref(c, st, np.asarray(t0, dtype=np.float64), np.concatenate([g_tau, g_del, g_gam]), HYP, FULL)
    O.updateTauEta(model, ch, 0, hy["alpha_eta"], hy["beta_eta"], seed=V.SEED)
    O.updateDeltaXi(model, ch, 0, seed=V.SEED)
    O.updateGammaXi(model, ch, 0, hy["nu_1"], seed=V.SEED)
    for nm, got in (("tau_eta", ch.tau_eta[..., 0]), ("delta_xi", ch.delta_xi[..., 0]), ("gamma_xi", ch.gamma_xi[..., 0])):
        ref = np.asarray(hr[nm], dtype=np.float64)
        assert ref.shape == got.shape, (nm, ref.shape, got.shape)
        assert np.abs(ref - got).max() <= 1e-9 * np.abs(got).max(), nm
    # A_xi: the reference's decision from the oracle's keyed proposal and uniform leaves no cell undecided and is the oracle's
    hyp = dict(hy)
    assert not V.check_gstd2(c, st, np.concatenate([g_tau, g_del, g_gam]), np.zeros(len(g_tau) + len(g_del) + len(g_gam)), hyp, FULL)
    cells = V.axi_reference(c, st, ch.delta_xi[..., 0], hyp)
    want = np.array(st["A_xi"], dtype=np.float64)
    for r in cells:
        a0, Sa = r["acc"](r["na"])
        assert abs(r["logu"] - a0) > 1e3 * 16 * V.U * (Sa + 1), r["cell"]
        if r["logu"] < a0:
            want[r["cell"]] = r["na"]
    O.updateAXi(model, ch, 0, O.make_hyper(c.K), seed=V.SEED)
    assert np.array_equal(ch.A_xi[..., 0], want), (ch.A_xi[..., 0], want)
    assert not V.check_axi(c, st, ch.A_xi[..., 0], ch.delta_xi[..., 0], hyp, FULL)
    assert len({bool(r["logu"] < r["acc"](r["na"])[0]) for r in cells}) == 2, "the case should see an accepted and a rejected cell"
