"""The main model's scalar jobs (csrc/scalar_jobs.hpp) on the device, entry by entry against tests/scalar_jobs_ref.py.

One sampler per case, and every case makes every run.  Every run pushes the case's state (the follow-up run at first_iter = 3
excepted: it crosses the hand-over between two runs), runs a mask (with the case's carrier bits, which put the jobs on the
route the case was written for) with the curve record on and judges EVERY iteration t, slot t - 1 -> slot t: the state it started
from is the pushed one (t = 0) or chain slot t - 1.  The run's last iteration is judged from the working state and the device's own
"gstd", "piprep", "logz_part", "rss"; an earlier one from chain slots alone with the oracle's keyed variates and their allowances
(what its mask does not move is the pushed state) -- under Ctx::defer_hyper these are the iterations whose job_hyper rode the
next k_pair_gram, the last one's rode k_loglik_flush; on the lean route they rode the lean k_curve_z, the last one k_curve_chi.
The groups: "core" all seven bits once and a residual-only tau run with the log-likelihood; "bits" each of U_PI, U_ALPHA3, U_DELTA,
U_A, U_GAMMA, U_TAU, U_SIGMA alone, everything else bit-equal; "multi" the seven bits for two and for three iterations (iteration 0
evaluates the pi tables in place, 1 and 2 take the prepared ones), a second run of one iteration at first_iter = 3 on the same
sampler, and SWEEP_WARM for three iterations; "lean" (cubic_P30) U_Z | U_NU and the seven bits for three iterations: no chi pass,
so the Z update trails as the lean k_curve_z and hosts delta, A, gamma and tau.  Every run ends with status 0, asserts
"hyper_route" against scalar_jobs_ref.expected_route and "pi_prepared" of its last iteration.  cubic_P30 and cubic_P30-n48 make
the "core" and "multi" runs again with bfmmm_set_solo_pair_gram(0) and with bfmmm_set_solo_pair_gram_tail(0) (the switches act on
the pair-Gram launch alone).  The last test prints the routes taken and the largest error / bound per (job, host of that
iteration's job) and asserts that every host judged delta, gamma and tau, and that both table paths and both outcomes of all four
Metropolis steps were seen.

(sigma^2 is judged in a run's last iteration where the run has no chi pass: a chi pass overwrites the sweep's "rss" with its own,
and "rss" is the last iteration's.)"""
import numpy as np
import pytest

import curve_update_ref as R
import factor_ref as F
import scalar_jobs_ref as J

pytestmark = pytest.mark.gpu

T_SLOTS = 12
SCALARS = ("pi", "alpha_3", "delta", "A", "gamma", "tau", "sigma_sq")
OTHERS = (("nu", J.U_NU), ("Phi", J.U_PHI), ("chi", J.U_CHI), ("Z", J.U_Z))
_records = {}


@pytest.fixture(autouse=True)
def _switches_back():
    from bayesfmmm_amd import _lib
    L = _lib.load()
    L.bfmmm_set_curve_record(1)
    try:
        yield
    finally:
        L.bfmmm_set_curve_record(0)
        L.bfmmm_set_solo_pair_gram(1)
        L.bfmmm_set_solo_pair_gram_tail(1)


class Run:
    def __init__(self, mask, iters=1, tag=None, judged=None, follow=False):
        self.mask, self.iters, self.follow = mask, iters, follow
        self.judged = judged or tuple(range(iters))      # the iterations of the run that are judged (relative to its first): all
        self.tag = tag or f"mask{mask:#x}" + ("" if iters == 1 else f":{iters}it") + (":first3" if follow else "")


GROUPS = {
    "core": [Run(J.SEVEN), Run(J.U_TAU | J.U_LOGLIK, tag="tau+loglik")],
    "bits": [Run(b, tag=nm + " alone") for nm, b in J.BITS.items()],
    "multi": [Run(J.SEVEN, iters=2), Run(J.SEVEN, iters=3), Run(J.SEVEN, follow=True), Run(J.SWEEP_WARM, iters=3, tag="sweep_warm:3it")],
    "lean": [Run(J.MASK_LEAN, iters=3, tag="lean:3it")],
}


def make_sampler(c):
    import bayesfmmm_amd as bf
    d = F.case_data(c)
    kw = dict(K=c.K, n_eigen=c.M, tot_mcmc_iters=T_SLOTS, **c.cfg)
    if c.kind == "mv":
        smp = bf.Sampler(bf.default_config(model=bf.MODEL_MULTIVARIATE, **kw), d["Y"], n_chains=c.nch)
    elif c.kind == "spline":
        smp = bf.Sampler(bf.default_config(model=bf.MODEL_FUNCTIONAL, basis_degree=c.deg, **kw), d["y"], d["t"], d["ik"], d["bk"], n_chains=c.nch)
    else:
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, basis_degree=max(c.degs) if c.degs else 1, **kw)
        smp = bf.Sampler(cfg, d["y"], basis=d["B"], band=c.band, penalty=d["Pmat"], penalty_band=c.pen_band, n_chains=c.nch)
    if c.nch > 1:
        smp.set_chain_id_stride(c.stride)
    return smp


def run_sampler(smp, what, *a, **kw):
    try:
        smp.run(*a, **kw)
    except Exception as e:      # noqa: BLE001 -- the binding raises on every non-zero status
        pytest.fail(f"{what}: bfmmm_run did not return 0: {e}")
    for q in range(smp.n_chains):
        smp.select_chain(q)
        status = int(smp.get_state("status")[0])
        assert status == 0, f"{what}, chain {q}: status word {status}"


def slot_of(smp, nm, t):
    ch = smp.get_chain(nm, t + 1)
    if nm == "tau":
        return np.array(ch[t])
    return np.array(ch[..., t] if ch.ndim > 1 else [ch[t]])


def judge(smp, c, what, q, st0, mask, it, last, route, rec):
    """every check of scalar_jobs_ref on the selected chain for iteration `it` (last: the run's last, the device's arrays are its)"""
    hyp, dims, cid = J.hyp_of(c, smp.cfg), smp.dims(), q * c.stride
    st_in = dict(st0) if it == 0 else {nm: slot_of(smp, nm, it - 1) for nm in SCALARS}
    if last:
        new = {nm: smp.get_state(nm) for nm in SCALARS}
        Z, nu, Phi = smp.get_state("Z"), smp.get_state("nu"), smp.get_state("Phi")
    else:
        new = {nm: slot_of(smp, nm, it) for nm in SCALARS}
        # (an iteration before the last: what its mask moves is in chain slot `it`, what it does not is the pushed state)
        Z, nu, Phi = (slot_of(smp, nm, it) if mask & bit else np.asarray(st0[nm], dtype=np.float64) for nm, bit in (("Z", J.U_Z), ("nu", J.U_NU), ("Phi", J.U_PHI)))
    fails = []
    var = J.variates(c, st_in["A"], hyp, dims, q=cid, it=it, seed=c.seed)
    nv = var["g"].shape[0]
    acc_dev = None
    w = {}
    if last:
        gstd = smp.debug("gstd")
        r = J.check_gstd(c, gstd, var)
        fails += r["fails"]
        w["gstd"] = r["worst"]
        g, gtol = gstd[:nv], np.zeros(nv)
        acc_dev = gstd[slice(*J.gstd_layout(c)["acc"])]
        for nm in SCALARS:      # the chain slot of the judged iteration is the working state, bit for bit, updated or not
            if not np.array_equal(np.ravel(slot_of(smp, nm, it)), np.ravel(new[nm])):
                fails.append(f"chain slot {it} of {nm} differs from the working state")
    else:
        g, gtol = var["g"], var["tol"]
    r = J.check_pi_alpha(c, st_in["pi"], st_in["alpha_3"], Z, new["pi"], new["alpha_3"], hyp, mask, q=cid, it=it, seed=c.seed, acc_dev=acc_dev)
    fails += r["fails"]
    w["acc"], vac = r["worst"], r["vacuous"]
    for k, v in r["outcome"].items():
        rec["outcomes"].setdefault(k, set()).add(v)
    if last and mask & (J.U_PI | J.U_ALPHA3):
        fails += R.check_logz(c, Z, smp.debug("logz_part"))
        r = J.check_piprep(c, smp.debug("piprep"), new["pi"], new["alpha_3"], hyp, cid, it + 1, seed=c.seed)
        fails += r["fails"]
        w["piprep"] = r["worst"]
    r = J.check_hyper(c, st_in, new, nu, Phi, g, gtol, hyp, mask, c.pcz)
    fails += r["fails"]
    w.update(delta=r["worst_delta"], gamma=r["worst_gamma"], tau=r["worst_tau"])
    r = J.check_A(c, st_in["A"], new["A"], new["delta"], var, hyp, mask, c.pcz)
    fails += r["fails"]
    vac = max(vac, r["vacuous"])
    for k, v in r["outcome"].items():
        rec["outcomes"].setdefault(k, set()).update(v)
    s2 = float(np.ravel(new["sigma_sq"])[0])
    if not mask & J.U_SIGMA:
        if s2 != float(np.ravel(st_in["sigma_sq"])[0]):
            fails.append("sigma^2 changed although its mask bit is off")
    elif last and not (mask & J.U_CHI and not c.pcz):
        lay = J.gstd_layout(c)
        r = J.check_sigma(c, float(smp.debug("rss")[0]), g[lay["sigma"][0]], gtol[lay["sigma"][0]], s2, hyp)
        fails += r["fails"]
        w["sigma"] = r["worst"]
    if last and mask & J.U_LOGLIK and not mask & J.U_SIGMA:      # the residual pass behind the jobs: Dyn::rss and the closed form (mv: its own)
        fails += R.check_total_and_loglik(c, smp.debug("rss_part"), float(smp.debug("rss")[0]), float(smp.get_state("loglik").ravel()[0]), s2, dims["n_obs_total"])
    if not vac <= J.NONVACUOUS:
        fails.append(f"a decision bound is {vac:.3g} of the margin it judges")
    host = {"acc": route["pi"], "piprep": "k_factor", "gstd": "k_factor", "sigma": "sweep"}
    # the host of THIS iteration's job_hyper: a run's last iteration closes in k_curve_chi (lean route) or k_loglik_flush (deferred)
    hh = {"lean_z": ("lean_z", "chi (closing)"), "deferred": ("deferred (k_pair_gram)", "deferred (flush)")}.get(route["hyper"], (route["hyper"],) * 2)[int(last)]
    for k, v in w.items():
        key = (k, host.get(k, hh))
        rec["worst"][key] = max(rec["worst"].get(key, 0.0), v)
    print(f"{what}, iteration {it}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()) + f"; decision bound / margin {vac:.3g}")
    rec["fails"] += [f"{what}, iteration {it}: {m}" for m in fails]


def run_case(name, solo=1, tail=1):
    key = (name, solo, tail)
    if key not in _records:
        try:
            _records[key] = _run_case(name, solo, tail)
        except BaseException as e:      # noqa: BLE001 -- pytest.fail raises outside Exception
            _records[key] = e
    if isinstance(_records[key], BaseException):
        raise _records[key]
    return _records[key]


def _run_case(name, solo, tail):
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    L = _lib.load()
    L.bfmmm_set_solo_pair_gram(solo)
    L.bfmmm_set_solo_pair_gram_tail(tail)
    assert (J.SWEEP_WARM, J.U_LOGLIK, J.U_CHI) == (bf.sampler.SWEEP_WARM, bf.sampler.U_LOGLIK, bf.sampler.U_CHI)
    c = J.BY_NAME[name]
    rec = dict(routes=[], worst={}, fails=[], outcomes={}, prepared=set())
    smp = make_sampler(c)
    states = [J.case_state(c, q) for q in range(c.nch)]
    groups = c.groups if (solo and tail) else tuple(g for g in c.groups if g in ("core", "multi"))
    first = 0
    for run in [r for g in groups for r in GROUPS[g]]:
        mask = run.mask | c.carrier
        what = f"{name}{'' if solo else ':general body'}{'' if tail else ':no tail'}:{run.tag}"
        if run.follow:
            first = 3      # (behind the three-iteration run of the same mask: no state is pushed in between)
        else:
            first = 0
            for q, st in enumerate(states):
                smp.select_chain(q)
                smp.set_state(**st)
        run_sampler(smp, what, mask, run.iters, first_iter=first, seed=c.seed, chain=0, phi_chi_zero=c.pcz)
        route = smp.hyper_route()
        exp = J.expected_route(c, mask, run.iters)
        if not (solo and tail) and exp["pi"] == "pair_gram_solo_ll":
            exp["pi"] = "pair_gram"
        assert route == exp, f"{what}: the run's scalar jobs rode {route}, the case was written for {exp}"
        rec["routes"].append((what, route))
        for q, st in enumerate(states):
            smp.select_chain(q)
            for rel in run.judged:
                it, last = first + rel, rel == run.iters - 1
                judge(smp, c, f"{what}, chain {q}", q, st, mask, it, last, route, rec)
            if mask & (J.U_PI | J.U_ALPHA3):
                pre = int(smp.debug("pi_prepared")[0])
                want = int(run.iters > 1 or run.follow)
                rec["prepared"].add((pre, route["pi"]))
                if pre != want:
                    rec["fails"].append(f"{what}, chain {q}: \"pi_prepared\" of the last iteration is {pre}, the run was written for {want}")
            if run.iters == 1 and not run.follow:      # whatever the mask does not name is bit-equal to the pushed state
                for nm, bit in tuple(J.BITS.items()) + OTHERS:
                    off = not mask & bit or (c.pcz and nm in ("delta", "A", "gamma", "chi"))
                    if off and not np.array_equal(np.ravel(smp.get_state(nm)), np.ravel(np.asarray(st[nm], dtype=np.float64).reshape(smp.get_state(nm).shape, order="F"))):
                        rec["fails"].append(f"{what}, chain {q}: {nm} changed although the mask does not name it")
        if c.nch > 1 and mask & J.U_TAU:      # every chain has its own keys: a chain id that ignored the stride would repeat a draw
            taus = []
            for q in range(c.nch):
                smp.select_chain(q)
                taus.append(smp.get_state("tau"))
            assert all(not np.array_equal(taus[0], t) for t in taus[1:]), f"{what}: two chains hold the same tau"
    smp.close()
    return rec


PARAMS = [(c.name, 1, 1) for c in J.CASES] + [(nm, s, t) for nm in ("cubic_P30", "cubic_P30-n48") for s, t in ((0, 1), (1, 0))]


def _id(p):
    return p[0] + ("" if p[1] else ":general body") + ("" if p[2] else ":no tail")


@pytest.mark.parametrize("name,solo,tail", PARAMS, ids=[_id(p) for p in PARAMS])
def test_scalar_jobs_against_longdouble(name, solo, tail):
    rec = run_case(name, solo, tail)
    assert not rec["fails"], f"{len(rec['fails'])} failures\n" + "\n".join(rec["fails"][:12])


def test_routes_taken_and_largest_errors():
    recs = {p: run_case(*p) for p in PARAMS}
    worst, hosts, outcomes, prepared = {}, set(), {}, set()
    for p, rec in recs.items():
        for what, ro in rec["routes"]:
            hosts |= {("job_hyper", ro["hyper"]), ("job_pi_alpha", ro["pi"]), ("job_pi_prepare", ro["pi_prepare"])}
            print(f"{what:64s} job_hyper: {ro['hyper']:9s} job_pi_alpha: {ro['pi']:18s} job_pi_prepare: {int(ro['pi_prepare'])}")
        for k, v in rec["worst"].items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, _id(p))
        for k, v in rec["outcomes"].items():
            outcomes.setdefault(k, set()).update(v)
        prepared |= rec["prepared"]
    for (job, host), (v, where) in sorted(worst.items()):
        print(f"largest device error / bound, {job:7s} hosted by {host:18s}: {v:.3g} ({where})")
    print("Metropolis outcomes seen:", {k: sorted(v) for k, v in outcomes.items()}, "; (pi_prepared, host) seen:", sorted(prepared))
    need = {("job_hyper", h) for h in ("chi", "lean_z", "deferred")} | {("job_pi_alpha", h) for h in ("pair_gram", "pair_gram_solo_ll", "factor")}
    need |= {("job_pi_prepare", True), ("job_pi_prepare", False)}
    assert need <= hosts, f"hosts not taken: {sorted(need - hosts, key=str)}"
    rows = {(job, h) for job in ("delta", "gamma", "tau") for h in ("chi", "lean_z", "chi (closing)", "deferred (k_pair_gram)", "deferred (flush)")}
    assert rows <= set(worst), f"(job, host) pairs never judged: {sorted(rows - set(worst))}"
    for k in ("pi", "alpha_3", "A0", "A1"):
        assert outcomes.get(k) == {True, False}, f"{k}: the runs only ever saw {outcomes.get(k)}"
    assert {p for p, _ in prepared} == {0, 1}, prepared
    assert all(v <= 1.0 for v, _ in worst.values())
