"""CPU tests of tests/scalar_jobs_ref.py: both float64 emulations of the scalar jobs pass every bound on every case (and the
constants G_* are still 4 x what they show), every mutation of the emulation is rejected by the check it was written for, each of
the four Metropolis steps is accepted and rejected at least once by the reference over the case list, the longdouble restatement
agrees with the oracle's updateDelta / updateA / updateGamma / updateTau / updatePi_PM / updateAlpha3 / updateSigma under the same
keyed variates, and lgamma_ld agrees with scipy's gammaln on the arguments the tables use."""
import numpy as np
import pytest

import curve_update_ref as R
import factor_ref as F
import oracle_lib as O
import scalar_jobs_ref as J

pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 here")

_cache = {}


def inputs(c):
    if c.name not in _cache:
        st, hyp, dims = J.case_state(c), J.hyp_of(c), J.dims_of(c)
        var = J.variates(c, st["A"], hyp, dims, seed=c.seed)
        _cache[c.name] = (st, hyp, dims, var, 0.37 * dims["n_obs_total"])
    return _cache[c.name]


def gstd_of(c, var):
    g = np.zeros(J.gstd_layout(c)["len"])
    g[:var["g"].shape[0]] = var["g"]
    return g


def run(c, variant="kernel", mut=None, mask=J.SEVEN):
    """the emulation's iteration as if it were the device's, under every check: dict(check: result)"""
    st, hyp, dims, var, rss = inputs(c)
    vm = J.variates(c, st["A"], hyp, dims, seed=c.seed, mut=mut) if mut in ("tau_shape_real_div", "sigma_half_sum_real") else var
    emu = J.emulate(c, st, st["Z"], st["nu"], st["Phi"], vm["g"], hyp, mask, rss, variant=variant, mut=mut, seed=c.seed, pcz=c.pcz)
    lay = J.gstd_layout(c)
    res = dict(gstd=J.check_gstd(c, gstd_of(c, vm), var))
    res["pi_alpha"] = J.check_pi_alpha(c, st["pi"], st["alpha_3"], st["Z"], emu["pi"], emu["alpha_3"], hyp, mask, seed=c.seed, acc_dev=emu["acc"])
    res["hyper"] = J.check_hyper(c, st, emu, st["nu"], st["Phi"], vm["g"], np.zeros_like(vm["g"]), hyp, mask, c.pcz)
    res["A"] = J.check_A(c, st["A"], emu["A"], emu["delta"], var, hyp, mask, c.pcz, acc_emu=emu["acc_A"])
    res["sigma"] = J.check_sigma(c, rss, vm["g"][lay["sigma"][0]], 0.0, emu["sigma_sq"], hyp)
    return res


GNAMES = dict(delta="G_DELTA", gamma="G_GAMMA", tau="G_TAU", sigma="G_SIGMA", acc="G_ACC", aacc="G_AACC")
MEAS = dict(delta="MEASURED_DELTA", gamma="MEASURED_GAMMA", tau="MEASURED_TAU", sigma="MEASURED_SIGMA", acc="MEASURED_ACC", aacc="MEASURED_AACC")


def ratios(res):
    return dict(delta=res["hyper"]["worst_delta"], gamma=res["hyper"]["worst_gamma"], tau=res["hyper"]["worst_tau"], sigma=res["sigma"]["worst"],
                acc=res["pi_alpha"]["worst"], aacc=res["A"]["worst"])


def test_emulations_pass_and_constants_hold(monkeypatch):
    """both emulations pass every bound on every case with the constants as they stand; then, with every G set to 1, the largest
    error / bound they show is what the constants were set from (and 4 x that is the constant)"""
    vac = [0.0, ""]
    for c in J.CPU_CASES:
        for variant in ("kernel", "plain"):
            res = run(c, variant)
            fails = [m for r in res.values() for m in r["fails"]]
            assert not fails, f"{c.name}, {variant} emulation:\n" + "\n".join(fails[:8])
            v = max(res["pi_alpha"]["vacuous"], res["A"]["vacuous"])
            if v > vac[0]:
                vac[:] = [v, c.name]
    print(f"largest decision bound / margin: {vac[0]:.3g} ({vac[1]})")
    assert vac[0] <= J.NONVACUOUS, vac
    G = {k: getattr(J, nm) for k, nm in GNAMES.items()}
    for nm in GNAMES.values():
        monkeypatch.setattr(J, nm, 1.0)
    worst = {v: {k: (0.0, "") for k in GNAMES} for v in ("kernel", "plain")}
    for c in J.CPU_CASES:
        for variant in ("kernel", "plain"):
            for k, v in ratios(run(c, variant)).items():
                if v > worst[variant][k][0]:
                    worst[variant][k] = (v, c.name)
    for variant in worst:
        for k, (w, where) in worst[variant].items():
            print(f"largest error / (bound at G = 1), {k:6s} {variant:6s}: {w:.3g} ({where})")
    for k in GNAMES:
        meas = getattr(J, MEAS[k])
        top = max(worst["kernel"][k][0], worst["plain"][k][0])
        assert top <= 1.02 * max(meas.values()), f"{k}: the emulations now show {top:.3g}, the constant was set from {meas}"
        assert 3.95 * max(meas.values()) <= G[k] <= 4.1 * max(meas.values()), f"{k}: G = {G[k]} is not 4 x {meas}"


@pytest.mark.parametrize("mut", sorted(J.MUTATIONS))
def test_mutation_is_rejected(mut):
    name, which = J.MUTATIONS[mut]
    res = run(J.BY_NAME[name], "kernel", mut=mut)
    if which == "gstd":
        assert res["gstd"]["fails"], f"{mut} on {name}: the variate of the wrong shape was accepted"
        print(f"{mut} on {name}: gstd error / allowance {res['gstd']['worst']:.3g}")
        return
    r, key = {"delta": (res["hyper"], "worst_delta"), "gamma": (res["hyper"], "worst_gamma"), "tau": (res["hyper"], "worst_tau"),
              "A": (res["A"], "worst"), "pi": (res["pi_alpha"], "worst"), "alpha_3": (res["pi_alpha"], "worst")}[which]
    print(f"{mut} on {name}: {which} error / bound {r[key]:.3g}")
    assert r[key] >= 10.0, f"{mut} on {name}: the {which} check sees only {r[key]:.3g} x its bound"
    assert any(which in m or (which in ("pi", "alpha_3") and "job_pi_alpha" in m) for m in r["fails"]), r["fails"]


def reference_outcomes(c, q=0, it=0):
    st, hyp, dims, _, _ = inputs(c)
    return J.reference_iteration(c, st, st["Z"], st["nu"], st["Phi"], hyp, dims, seed=c.seed, q=q, it=it, pcz=c.pcz)["outcome"]


def test_every_metropolis_step_is_accepted_and_rejected_by_the_reference():
    """iteration 0 from the pushed state of every single-chain case (the runs that do not move Z, theta and delta first)"""
    seen = {k: set() for k in ("pi", "alpha_3", "A0", "A1")}
    for c in J.CPU_CASES:
        oc = reference_outcomes(c)
        print(c.name, {k: (v if isinstance(v, bool) else "".join("ar"[not x] for x in v)) for k, v in oc.items()})
        for k, v in oc.items():
            seen[k] |= set(v) if isinstance(v, list) else {v}
    for k, v in seen.items():
        assert v == {True, False}, f"{k}: the reference only ever {'accepts' if True in v else 'rejects'} over the case list"


@pytest.mark.parametrize("name", ["cubic_P30", "mv_P7", "cubic_P30-reject"])
def test_restatement_matches_the_oracle(name):
    """the oracle's own updates at iteration 0 of a two-slot chain, against reference_iteration with the same keyed variates"""
    c = J.BY_NAME[name]
    st, hyp, dims, var, _ = inputs(c)
    d = F.case_data(c)
    mv = c.kind == "mv"
    model = O.Model(list(d["Y"]), [np.eye(c.P)] * c.n, c.K, c.M, mv=True, Pmat=np.eye(c.P)) if mv else O.Model(d["y"], d["B"], c.K, c.M, Pmat=d["Pmat"])
    ch = O.Chain(model, 2)
    ch.set_slot0(nu=st["nu"], chi=st["chi"], Z=st["Z"], sigma=float(st["sigma_sq"][0]), Phi=st["Phi"], delta=st["delta"], gamma=st["gamma"],
                 tau=st["tau"], pi=st["pi"], alpha3=float(st["alpha_3"][0]), A=st["A"])
    kw = dict(seed=c.seed)
    O.updatePi_PM(model, ch, 0, hyp["c"], hyp["a_pi_PM"], **kw)
    O.updateAlpha3(model, ch, 0, hyp["b"], hyp["var_alpha3"], **kw)
    O.updateDelta(model, ch, 0, **kw)
    O.updateA(model, ch, 0, O.make_hyper(c.K, **{k: v for k, v in hyp.items() if k != "c"}), **kw)
    O.updateGamma(model, ch, 0, hyp["nu_1"], **kw)
    O.updateTau(model, ch, 0, hyp["alpha_nu"], hyp["beta_nu"], **kw)
    O.updateSigma(model, ch, 0, hyp["alpha_0"], hyp["beta_0"], **kw)
    # the RSS the oracle's sigma step saw, from the fitted values of the state (longdouble)
    coef = np.einsum("ik,kp->ip", J._ld(st["Z"]), J._ld(st["nu"])) + np.einsum("ik,im,kpm->ip", J._ld(st["Z"]), J._ld(st["chi"]), J._ld(st["Phi"]))
    Bs, ys = ([np.eye(c.P)] * c.n, list(d["Y"])) if mv else (d["B"], d["y"])
    rss = float(sum(((J._ld(y) - J._ld(B) @ coef[i]) ** 2).sum() for i, (B, y) in enumerate(zip(Bs, ys))))
    ref = J.reference_iteration(c, st, st["Z"], st["nu"], st["Phi"], hyp, dims, seed=c.seed, rss=rss)
    got = dict(pi=ch.pi[:, 0], alpha_3=ch.alpha3[0], delta=ch.delta[..., 0], A=ch.A[..., 0], gamma=ch.gamma[..., 0], tau=ch.tau[0], sigma_sq=ch.sigma[0])
    for nm, g in got.items():
        r = np.asarray(ref[nm], dtype=np.float64).reshape(np.shape(g))
        assert np.abs(r - g).max() <= 1e-9 * np.abs(g).max(), (nm, r, g)
    assert not J.check_gstd(c, gstd_of(c, var), var)["fails"]


def test_lgamma_ld_against_scipy():
    sp = pytest.importorskip("scipy.special")
    args = set()
    for c in J.CPU_CASES:
        st, hyp, _, _, _ = inputs(c)
        for sc in (hyp["a_pi_PM"], float(st["alpha_3"][0])):
            args |= {sc * float(p) for p in st["pi"]} | {sc}
        args |= {float(a) for a in np.ravel(st["A"])}
    args |= {1.0, 2.0, 1e-3, 171.5}
    for x in sorted(args):
        ref = float(sp.gammaln(x))
        assert abs(float(R.lgamma_ld(x)) - ref) <= 4e-16 * max(abs(ref), 1.0) + 1e-15, (x, float(R.lgamma_ld(x)), ref)
    for x in (0.4, 1.0, 2.0, 7.5, 333.0):      # the kernels' lgamma_pos in float64 stays inside its absolute bound
        assert abs(J.lgamma_pos64(x) - float(R.lgamma_ld(x))) <= J.lg_bound(x), x
