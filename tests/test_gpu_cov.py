"""The eta / Xi covariate block (csrc/kernels_cov.hip) on the device, quantity by quantity against tests/cov_ref.py.

Every run pushes a state, reads c_i^0 / g_i^0 ("cfull" / "gfull") behind a residual-only run of that state (mask U_LOGLIK: neither
U_ETA nor U_XI), runs the judged mask (always with U_LOGLIK; theta, Z and chi are left alone) and holds "Wdir", "H2aa", "C2", "Lz2",
every one of the K D + K M D draws, the final "cfull" / "gfull", "rss_part", Dyn::rss, the log-likelihood, "gstd2", tau_eta / delta_xi /
gamma_xi, the A_xi step and the chain slots to the longdouble bounds of cov_ref.  A run of several iterations is judged in its LAST iteration: the
state it started from is the pushed one with the eta / Xi blocks of the previous chain slot.  One run is a full SWEEP_WARM | COV_MEAN |
COV_XI trajectory of three iterations, judged in the last from chain slots alone, with c_i^0 restated in longdouble.  Every run asserts "cov_route" against
the route its case was written for; the stiff cases assert the pivot margin and the empty-cluster case its factor routes from the
device's own "H2aa"; cases of the cubic band class run a second time with bfmmm_set_exact_instances(0).  The last
test prints the routes taken and the largest device error / bound per quantity."""
import numpy as np
import pytest

import cov_ref as V
import curve_update_ref as R
import factor_ref as F

pytestmark = pytest.mark.gpu

T_SLOTS = 12
FULL = V.COV_MEAN | V.COV_XI
SWEEP_WARM = 0x207ff      # bayesfmmm_amd.sampler.SWEEP_WARM (asserted in run_case)
SWEEP_NAMES = ("nu", "Phi", "chi", "Z", "sigma_sq")
COV_NAMES = ("eta", "xi", "tau_eta", "delta_xi", "gamma_xi", "A_xi")
_records = {}


@pytest.fixture(autouse=True)
def _exact_instances_back_on():
    from bayesfmmm_amd import _lib
    try:
        yield
    finally:
        _lib.load().bfmmm_set_exact_instances(1)


class Run:
    def __init__(self, mask, beta=1.0, pcz=False, iters=1, tag=None, sweep=False):
        self.mask, self.beta, self.pcz, self.iters, self.sweep = mask | V.U_LOGLIK, beta, pcz, iters, sweep
        self.tag = tag or f"mask{mask:#x}" + ("" if beta == 1.0 else f":beta{beta}") + (":pcz" if pcz else "") + ("" if iters == 1 else f":{iters}it")


HYPER_BITS = (V.U_TAU_ETA, V.U_DELTA_XI, V.U_A_XI, V.U_GAMMA_XI)
GROUPS = {
    "full": [Run(FULL)],
    "masks": [Run(m | s) for m in (V.COV_MEAN, V.COV_XI, 0) for s in (0, V.U_SIGMA)] + [Run(FULL | V.U_SIGMA)],
    "hyperbits": [Run(V.U_ETA | V.U_XI | b) for b in HYPER_BITS] + [Run(V.U_ETA | V.U_XI)],
    "misc": [Run(FULL, beta=0.37), Run(FULL, pcz=True), Run(FULL, iters=3), Run(FULL, iters=12),
             Run(FULL | SWEEP_WARM, iters=3, sweep=True, tag="sweep_warm:3it")],
}
MAIN = "cubic_P30_D2-benign"


def make_sampler(c):
    import bayesfmmm_amd as bf
    d = F.case_data(c)
    if c.kind == "mv":
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=c.K, n_eigen=c.M, tot_mcmc_iters=T_SLOTS)
        smp = bf.Sampler(cfg, d["Y"], n_chains=c.nch)
    elif c.kind == "spline":
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=c.deg, tot_mcmc_iters=T_SLOTS)
        smp = bf.Sampler(cfg, d["y"], d["t"], d["ik"], d["bk"], n_chains=c.nch)
    else:
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=max(c.degs) if c.degs else 1, tot_mcmc_iters=T_SLOTS)
        smp = bf.Sampler(cfg, d["y"], basis=d["B"], band=c.band, penalty=d["Pmat"], penalty_band=c.pen_band, n_chains=c.nch)
    smp.set_covariates(R.case_X(c), covariance_adj=c.cov_adj)
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


def push(smp, states):
    for q, st in enumerate(states):
        smp.select_chain(q)
        smp.set_state(**st)


HYP_NAMES = ("alpha_eta", "beta_eta", "nu_1", "alpha1l", "alpha2l", "beta1l", "beta2l", "var_epsilon1", "var_epsilon2")


def judge(smp, c, what, q, st_in, c0, g0, run, it, rec, g_before, e_c=None, e_g=None, tt=0):
    """every check of cov_ref on the selected chain's arrays after a run whose last iteration `it` started from st_in"""
    hyp = {nm: float(getattr(smp.cfg, nm)) for nm in HYP_NAMES}
    dev = dict(Wdir=smp.debug("Wdir"), H2aa=smp.debug("H2aa"), C2=smp.debug("C2"), Lz2=smp.debug("Lz2"), cfull=smp.debug("cfull"),
               gfull=smp.debug("gfull"), rss_part=smp.debug("rss_part"), sigma2=float(smp.get_state("sigma_sq").ravel()[0]))
    now = {nm: smp.get_state(nm) for nm in COV_NAMES}
    dev.update(now)
    dev["th_new"] = V.theta_of(c, now)
    fails = []
    if not np.array_equal(V.thetaX_rows(c, smp.debug("thetaX")), dev["th_new"]):
        fails.append(f"{what}: \"thetaX\" differs from the eta / xi of the working state")
    rc = smp.debug("rec")
    res = V.check_all(c, rc, st_in, R.case_X(c), c0, g0, run.mask, run.beta, dev, hyp, q=q, it=it, pcz=run.pcz, gstd2=smp.debug("gstd2"), e_c=e_c,
                      e_g=e_g, tt=tt)
    for k, r in res.items():
        fails += [f"{what}: {m}" for m in r["fails"]]
    fails += [f"{what}: {m}" for m in V.check_gstd2(c, st_in, smp.debug("gstd2"), g_before, hyp, run.mask, q, it, run.pcz, tt)]
    fails += [f"{what}: {m}" for m in V.check_axi(c, st_in, now["A_xi"], now["delta_xi"], hyp, run.mask, q, it, run.pcz, tt)]
    fac = res["factor"]
    if c.regime == "stiff" and c.kind != "mv" and not fac["rho"] >= 1e-9:      # (from the device's own H2aa; the diagonal model has no pivots)
        fails.append(f"{what}: the smallest Cholesky pivot ratio {fac['rho']:.3g} is not a factor 1000 above the kernels' 1e-12 decision")
    if c.empty is not None and (run.mask & V.U_ETA) and not (("pinv", "eta") in fac["routes"] and ("chol", "eta") in fac["routes"]):
        fails.append(f"{what}: the eta directions took {sorted(fac['routes'])}: the empty cluster's must take the pseudo-inverse, the others not")
    if ("pinv", "xi") in fac["routes"]:
        fails.append(f"{what}: a Xi direction was judged on the pseudo-inverse route")
    if not res["steps"]["vacuous"] <= V.NONVACUOUS:
        fails.append(f"{what}: a step bound is {res['steps']['vacuous']:.3g} of the |delta| it judges")
    part = smp.debug("rss_part")
    s2, ll = dev["sigma2"], float(smp.get_state("loglik").ravel()[0])
    fails += [f"{what}: {m}" for m in R.check_total_and_loglik(c, part, float(smp.debug("rss")[0]), ll, s2, smp.dims()["n_obs_total"])]
    for nm in COV_NAMES + ("loglik", "sigma_sq"):      # the chain slot of the judged iteration is the working state, bit for bit
        ch = smp.get_chain(nm, it + 1)
        slot = ch[..., it] if ch.ndim > 1 else ch[it]
        if not np.array_equal(np.asarray(slot).ravel(), np.asarray(smp.get_state(nm)).ravel()):
            fails.append(f"{what}: chain slot {it} of {nm} differs from the working state")
    w = rec["worst"]
    for k, v in dict(h2aa=res["h2aa"]["worst"], C=res["factor"]["worst_C"], Lz=res["factor"]["worst_L"], step=res["steps"]["worst"],
                     cfull=res["final"]["worst"], gfull=res["final"]["worst_g"], rss_part=res["rss"]["worst"], tau_eta=res["hyper"]["worst_tau"], delta_xi=res["hyper"]["worst_delta"],
                     gamma_xi=res["hyper"]["worst_gamma"],
                     vacuous=res["steps"]["vacuous"]).items():
        w[k] = max(w.get(k, 0.0), v)
    print(f"{what}: error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()) + f"; kappa_s {res['factor']['kappa']:.3g}, "
          f"smallest pivot ratio {res['factor']['rho']:.3g}, factor routes {sorted(res['factor']['routes'])}")
    rec["fails"] += fails
    return res


def run_case(name, exact, group):
    """every run of one group of one case on one sampler, checked: dict(routes, worst, fails, refused).  Memoised once it is
    complete; a run that stopped midway (a route assertion, a non-zero status) is remembered as its exception and raised again, so
    that no later caller takes a partial record for a clean one."""
    key = (name, exact, group)
    if key not in _records:
        try:
            _records[key] = _run_case(name, exact, group)
        except BaseException as e:      # noqa: BLE001 -- pytest.fail raises outside Exception
            _records[key] = e
    if isinstance(_records[key], BaseException):
        raise _records[key]
    return _records[key]


def _run_case(name, exact, group):
    from bayesfmmm_amd import _lib
    _lib.load().bfmmm_set_exact_instances(1 if exact else 0)
    import bayesfmmm_amd as bf
    assert SWEEP_WARM == bf.sampler.SWEEP_WARM
    c = V.BY_NAME[name]
    rec = dict(routes=[], worst={}, fails=[], refused=False)
    try:
        smp = make_sampler(c)
    except _lib.BfmmmError as e:      # the host-side refusal of cov_block_fits: only the case written for it may meet it
        assert name in V.REFUSED and "exceed the covariate kernels' on-chip staging" in str(e), e
        rec["refused"] = True
        return rec
    states = [V.case_state(c, q) for q in range(c.nch)]
    if not c.cov_adj:
        for st in states:
            st["xi"] = np.zeros_like(st["xi"])
    base = {}
    for run in GROUPS[group]:
        what = f"{name}{'' if exact else ':general'}:{run.tag}"
        kw = dict(seed=V.SEED, chain=0, phi_chi_zero=run.pcz)
        push(smp, states)
        if run.iters > 1:      # what the LAST iteration found in "gstd2" is what the one before left: run that far first
            run_sampler(smp, what + " (the iterations before the judged one)", run.mask, run.iters - 1, beta=run.beta, **kw)
            push(smp, states)
        g_before = []
        for q in range(c.nch):
            smp.select_chain(q)
            g_before.append(smp.debug("gstd2"))
        run_sampler(smp, what, run.mask, run.iters, beta=run.beta, **kw)
        route = smp.cov_route()
        exp = V.expected_route(c, run.mask, exact, run.pcz)
        assert route == exp, f"{what}: the run launched {route}, the case was written for {exp}"
        rec["routes"].append((what, route))
        it = run.iters - 1
        outs, starts = [], []
        for q, st in enumerate(states):
            smp.select_chain(q)
            st_in = dict(st)
            if it > 0:
                for nm in COV_NAMES:
                    st_in[nm] = np.array(smp.get_chain(nm, it)[..., it - 1])
                if run.sweep:      # a full sweep: nu, Phi, chi, Z, sigma^2 of the judged iteration itself
                    for nm in SWEEP_NAMES:
                        ch = smp.get_chain(nm, it + 1)
                        st_in[nm] = np.array(ch[..., it] if ch.ndim > 1 else [ch[it]])
            starts.append(st_in)
        if run.sweep:      # c^0, g^0 restated from the chain slots (cov_ref.restate_c0)
            for q, st_in in enumerate(starts):
                smp.select_chain(q)
                c0, g0, bc, bg = V.restate_c0(c, smp.debug("rec"), st_in, R.case_X(c))
                judge(smp, c, f"{what}, chain {q}", q, st_in, c0, g0, run, it, rec, g_before[q], e_c=bc, e_g=bg)
            continue
        # judged before the residual-only run below overwrites cfull / gfull: collect per chain what that run needs afterwards
        pend = []
        for q, st_in in enumerate(starts):
            smp.select_chain(q)
            ck = (q, run.pcz) if it == 0 else None
            if ck is not None and ck in base:
                c0, g0 = base[ck]
                judge(smp, c, f"{what}, chain {q}", q, st_in, c0, g0, run, it, rec, g_before[q])
                outs.append(smp.get_state("eta"))
            else:
                pend.append(q)
        if pend:
            saved = {}
            names = ("Wdir", "H2aa", "C2", "Lz2", "cfull", "gfull", "rss_part", "gstd2", "thetaX", "rss")
            for q in pend:
                smp.select_chain(q)
                saved[q] = (Snapshot(smp, names, it))
            push(smp, starts)
            run_sampler(smp, what + " (residual-only pass)", V.U_LOGLIK, 1, beta=run.beta, **kw)
            assert smp.cov_route()["launches"] == 1
            for q in pend:
                smp.select_chain(q)
                c0, g0 = smp.debug("cfull"), smp.debug("gfull")
                if it == 0:
                    base[(q, run.pcz)] = (c0, g0)
                judge(saved[q], c, f"{what}, chain {q}", q, starts[q], c0, g0, run, it, rec, g_before[q])
                outs.append(saved[q].get_state("eta"))
        if c.nch > 1:       # every chain has its own state: a chain offset would have compared (or written) the wrong one
            for q in range(1, c.nch):
                assert not np.array_equal(outs[0], outs[q]), f"{what}: chains 0 and {q} hold the same eta"
    smp.close()
    return rec


class Snapshot:
    """what `judge` reads of the selected chain, taken before a later run overwrites it"""
    def __init__(self, smp, names, it):
        self.cfg = smp.cfg
        self._dbg = {nm: smp.debug(nm) for nm in names + ("rec",)}
        self._st = {nm: smp.get_state(nm) for nm in COV_NAMES + ("sigma_sq", "loglik")}
        self._ch = {nm: smp.get_chain(nm, it + 1) for nm in COV_NAMES + ("loglik", "sigma_sq")}
        self._dims = smp.dims()

    def debug(self, nm):
        return self._dbg[nm]

    def get_state(self, nm):
        return self._st[nm]

    def get_chain(self, nm, n):
        return self._ch[nm]

    def dims(self):
        return self._dims


def _params():
    out = []
    for c in V.CASES:
        for exact in ((True, False) if c.BW == 3 and c.n <= 300 else (True,)):
            out.append((c.name, exact, "full"))
    out += [(MAIN, True, g) for g in ("masks", "hyperbits", "misc")]
    out += [("cubic_P30_D2_4chains-benign", True, "misc"), ("cubic_P30_D2_noadj-benign", True, "masks"), ("mv_P7_D2-benign", True, "masks")]
    return out


PARAMS = _params()


@pytest.mark.parametrize("name,exact,group", PARAMS, ids=[f"{n}{'' if e else ':general'}:{g}" for n, e, g in PARAMS])
def test_block_against_longdouble(name, exact, group):
    rec = run_case(name, exact, group)
    assert not rec["fails"], f"{len(rec['fails'])} failures\n" + "\n".join(rec["fails"][:12])
    assert rec["refused"] == (name in V.REFUSED), f"{name}: bfmmm_set_covariates {'refused' if rec['refused'] else 'admitted'} the shape"


def test_routes_taken_and_largest_errors():
    recs = {p: run_case(*p) for p in PARAMS}
    worst, seen = {}, set()
    for (name, exact, group), rec in recs.items():
        if rec["refused"]:
            print(f"{name}: refused by cov_block_fits (asserted message)")
            continue
        for what, ro in rec["routes"]:
            seen.add((ro["BW"], ro["LPC"], ro["DX"]))
            print(f"{what:60s} k_cov_group<{ro['BW']},{ro['LPC']},{ro['DX']}> x {ro['launches']}, k_cov_w2<{ro['W2D']}>, k_cov_factor<{ro['PP']}>, "
                  f"NB2 {ro['NB2']}, NBS {ro['NBS']}, NPG {ro['NPG']}, eta {int(ro['do_eta'])}, xi {int(ro['do_xi'])}")
        for k, v in rec["worst"].items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, f"{name}{'' if exact else ':general'}:{group}")
    for k, (v, where) in sorted(worst.items()):
        print(f"largest device {'bound / |delta|' if k == 'vacuous' else 'error / bound'}, {k}: {v:.3g} ({where})")
    need = {(bw, lpc, 0) for bw in (0, 1, 2, 4, 5) for lpc in (32, 64)} | {(15, 32, 0), (31, 64, 0)}
    need |= {(3, lpc, D) for lpc in (32, 64) for D in range(1, 9)} | {(3, lpc, 0) for lpc in (32, 64)}
    assert need <= seen, f"k_cov_group instances not taken: {sorted(need - seen)}"
    nb = {(ro["NB2"] > 16, ro["NBS"] > 128, ro["LPC"]) for rec in recs.values() for _, ro in rec["routes"]}
    assert (True, True, 64) in nb and any(b and lpc == 32 for _, b, lpc in nb), nb
