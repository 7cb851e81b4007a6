"""The tempered-transition block on the device, sweep by sweep and number by number against tests/tempered_ref.py and the step
references beneath it (sweep_ref, curve_update_ref, scalar_jobs_ref, cov_ref with tt passed through).

(a) Single tempered sweeps (Sampler.run_tt: the call the block's loop makes).  Every case of tempered_ref.ROUTED -- k_sweep_chain,
    k_sweep, k_sweep_diag, and D = 2 with the Xi block, asserted from "sweep_route" / "cov_route" -- runs at (beta 0.37, tt_step 2) and
    at (beta 1, tt_step 1), iteration 2, from a pushed state, twice: with U_NU | U_PHI | U_SIGMA (no chi pass: "rss" is the sweep's),
    which holds k_factor's C_a and L_a z_a (the keyed nu / Phi normals of (iteration, tt_step), f = beta / sigma^2; without covariates), the
    sweep steps, the RSS, the tempered sigma^2 and every entry of "gstd" to their references; and with the block's own
    mask, which holds the Z update (proposals, acceptance values, log_uu), the pi / alpha_3 job and the tables it leaves for iteration
    3 (tt_step 0 keys), the sweep steps, the chi steps and normals, delta / A / gamma / tau and, for D = 2, the eta / Xi block.
    "z_prepared" and "pi_prepared" must read 0, the Z update must be the stand-alone kernel and nothing fused, status 0.  (With
    covariates the chi pass rewrites "rss": there the tempered sigma^2 is held through its "gstd" entry alone.)
(b) The block on two samplers, every case of tempered_ref.CASES.  A: pushed state, a plain run up to `iter` (fused, asserted, where
    the model has no covariates), snapshot, tempered_transition, "tt_trace".  B: the same run, then the 2 N_t sweeps replayed with
    run_tt at the trace's betas: sigma^2 and RSS after every sweep bit-equal to the trace.  Ladder, schedule, logA, log u and the
    decision by tempered_ref; the outcome is the oracle's.  Accepted: A's state bit-equal to B's final state, gamma to the snapshot.
    Rejected: A's state and chain slot `iter` bit-equal to the snapshot, the log-likelihood slot the plain run's.
(c) The iteration after the block (tempered_ref.AFTER_BLOCK: one accepted, one rejected): a plain run of two iterations from
    iter + 1 on A; the Z update, the pi / alpha_3 job and the chi update of iteration iter + 1 from chain slots against the references
    with (iter + 1, tt_step 0) keys.  After the rejection Dyn's zprep_valid and piprep_valid read 0; after the acceptance they are printed.
(d) Edges: N_t = 1 (in the list: logA == 0.0, accepted, ladder [beta_N_t]); a second block on the sampler of the rejected one; a case
    with set_slot_base(1); a batch of two chains is refused with its message.
The last test prints the routes taken and the largest device error / bound per check."""
import numpy as np
import pytest

import cov_ref as V
import curve_update_ref as R
import factor_ref as F
import scalar_jobs_ref as J
import sweep_ref as S
import tempered_ref as T
import test_gpu_cov as TC
import test_gpu_curve_update as TCU
import test_gpu_sweep as TS

pytestmark = pytest.mark.gpu

U = F.U
IT_SINGLE = 2      # the iteration of the single sweeps
_single, _blocks = {}, {}


@pytest.fixture(autouse=True)
def _recording():
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    lib.bfmmm_set_curve_record(1)
    try:
        yield
    finally:
        lib.bfmmm_set_curve_record(0)


def case_of(name):
    return V.BY_NAME[name] if name in V.BY_NAME else R.BY_NAME[name]


def make_sampler(c, T_slots, n_chains=1):
    import bayesfmmm_amd as bf
    d = F.case_data(c)
    if c.kind == "mv":
        smp = bf.Sampler(bf.default_config(model=bf.MODEL_MULTIVARIATE, K=c.K, n_eigen=c.M, tot_mcmc_iters=T_slots), d["Y"], n_chains=n_chains)
    else:
        assert c.kind == "spline"
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=c.deg, tot_mcmc_iters=T_slots)
        smp = bf.Sampler(cfg, d["y"], d["t"], d["ik"], d["bk"], n_chains=n_chains)
    if c.D:
        smp.set_covariates(R.case_X(c), covariance_adj=c.cov_adj)
    return smp


def state_of(c):
    return V.case_state(c) if c.D else R.case_state(c)


def names_of(c):
    return T.STATE_NAMES + T.SCALAR_NAMES + (T.COV_STATE_NAMES if c.D else ())


def status_ok(smp, what):
    status = int(smp.get_state("status")[0])
    assert status == 0, f"{what}: status word {status}"


def run_tt(smp, what, *a, **kw):
    try:
        smp.run_tt(*a, **kw)
    except Exception as e:      # noqa: BLE001 -- the binding raises on every non-zero status
        pytest.fail(f"{what}: bfmmm_debug_run_tt did not return 0: {e}")
    status_ok(smp, what)


def run_plain(smp, what, *a, **kw):
    try:
        smp.run(*a, **kw)
    except Exception as e:      # noqa: BLE001
        pytest.fail(f"{what}: bfmmm_run did not return 0: {e}")
    status_ok(smp, what)


def slot_of(smp, nm, s):
    ch = smp.get_chain(nm, s + 1)
    if nm == "tau":
        return np.array(ch[s])
    return np.array(ch[..., s] if ch.ndim > 1 else [ch[s]])


def state_now(smp, names):
    return {nm: smp.get_state(nm) for nm in names}


def note(rec, key, v):
    rec["worst"][key] = max(rec["worst"].get(key, 0.0), float(v))


def assert_sweep_kernel(smp, what, c, kernel):
    route = smp.sweep_route()
    assert route["kernel"] == kernel, f"{what}: the sweep ran {route}, the case was written for {kernel}"
    if not c.D:      # (the covariate case is not in sweep_ref's table: its kernel alone is asserted)
        got = (route["kernel"], route["targ"], route["mv"], route["direct"], route["threads"])
        assert got == S.expected_route(c), f"{what}: the sweep ran {got}, sweep_ref.expected_route gives {S.expected_route(c)}"
    return route


def assert_unfused(smp, what, c, full):
    cr = smp.curve_route()
    assert not cr["chi"]["fuse"], f"{what}: a tempered sweep ran the fused k_curve_chi: {cr}"
    if full:
        assert cr["z"]["form"] == "standalone" and cr["chi"]["mode"] == 2, f"{what}: {cr}"
        exp = R.expected_route(c, "chi")["chi"]
        assert cr["chi"] == exp, f"{what}: k_curve_chi ran {cr['chi']}, the case was written for {exp}"
    return cr


# ---------------------------------------------------------------------------------------------------------------------
# (a) single tempered sweeps
# ---------------------------------------------------------------------------------------------------------------------
def sweep_part(smp, rec, what, c, st, mask, route, beta, th0, sigma_old):
    """the sweep steps (and, without a chi pass, the RSS) of the run that has just ended"""
    inp = TS.read_inputs(smp, c, c.MD)
    th1 = smp.debug("theta").reshape(c.A, c.P)
    f = beta / sigma_old
    rss = float(smp.debug("rss")[0])
    if c.D or mask & R.U_CHI:      # a chi pass rewrote "rss": the steps alone
        r = S.check_steps(c, mask, th0, th1, inp["H"], inp["Cmat"], inp["Lz"], inp["rvec"], inp["hq"], f, c.MD)
        rec["fails"] += [f"{what}, kernel {route['kernel']}: {r['msg']}"] if not r["ok"] else []
        for x in r["steps"]:
            if not x["bmax"] <= 1e-3 * x["dmax"]:
                rec["fails"].append(f"{what}: step {x['s']}: the bound ({x['bmax']:.3g}) is not small against the step ({x['dmax']:.3g})")
        note(rec, ("sweep step", route["kernel"]), r["worst"])
        print(f"{what}: sweep steps error / bound {r['worst']:.3g}")
        return None
    w, g, fails = TS.check_chain(what, c, mask, c.MD, route, th0, th1, inp, f, rss)
    rec["fails"] += fails
    note(rec, ("sweep step", route["kernel"]), w)
    note(rec, ("sweep RSS", route["kernel"]), g)
    return rss


def factor_part(smp, rec, what, c, st, kernel, beta, it, tt):
    """k_factor of the sweep that has just ended (every input of Prec_a is the pushed state): C_a against the longdouble inverse at
    f = beta / sigma^2 and L_a z_a against it with the keyed nu / Phi normals of (it, tt_step tt), as tests/test_gpu_factor.py"""
    d = smp.dims()
    H = smp.debug("H").reshape(d["R"], d["LG"])
    Cm, Lz = smp.debug("Cmat").reshape(c.A, c.P, c.P), smp.debug("Lz").reshape(c.A, c.P)
    z = F.normals(c, 0, it, tt)
    precs = F.precisions(c, F.hbands_from_H(c, H), T.tempered_state(st, beta))
    for a in range(c.A):
        r = F.check_direction(c, a, precs[a], Cm[a], Lz[a], z[a])
        note(rec, ("k_factor C", kernel), r["rC"])
        note(rec, ("k_factor L z (keyed normals)", kernel), r["rL"])
        if not r["ok"]:
            rec["fails"].append(f"{what}: k_factor: {r['msg']}")
    print(f"{what}: k_factor error / bound: C {rec['worst'][('k_factor C', kernel)]:.3g}, L z {rec['worst'][('k_factor L z (keyed normals)', kernel)]:.3g}")


def _single_case(name, beta, tt):
    import bayesfmmm_amd as bf
    assert (T.SWEEP_WARM, T.COV_FULL) == (bf.sampler.SWEEP_WARM, bf.sampler.COV_MEAN | bf.sampler.COV_XI)
    c = case_of(name)
    t0 = next(t for t in T.CASES if t.name == name)
    kernel, mask_full = t0.kernel, t0.mask
    it, seed = IT_SINGLE, F.SEED
    X = R.case_X(c) if c.D else None
    rec = dict(routes={}, worst={}, fails=[])
    smp = make_sampler(c, it + 2)
    st = state_of(c)
    hyp, dims = J.hyp_of(c, smp.cfg), smp.dims()
    assert (dims["n_obs_total"], dims["half_sum"]) == tuple(T.dims_of(c)[k] for k in ("n_obs_total", "half_sum"))
    lay = J.gstd_layout(c)
    var = J.variates(c, st["A"], hyp, dims, q=0, it=it, seed=seed, tt=tt, sigma_shape=T.sigma_shape(beta, dims, hyp))
    th0, s_old = S.theta_of(c, st), float(st["sigma_sq"][0])
    kw = dict(seed=seed, chain=0)

    # ---- the sweep alone: U_NU | U_PHI | U_SIGMA (run_tt adds the log-likelihood; with U_SIGMA that is no chi pass)
    what = f"{name}:beta{beta}:tt{tt}:sweep"
    smp.set_state(**st)
    mask = S.U_NU | S.U_PHI | S.U_SIGMA
    run_tt(smp, what, mask, it, beta, tt, **kw)
    route = rec["routes"]["sweep"] = assert_sweep_kernel(smp, what, c, kernel)
    assert_unfused(smp, what, c, False)
    dyn = smp.dyn()
    assert (dyn["tt_step"], dyn["beta"]) == (tt, beta), dyn
    rss = sweep_part(smp, rec, what, c, st, mask, route, beta, th0, s_old)
    if not c.D:      # (with covariates H is not the contraction factor_ref's cases are written for: the eta / Xi block's own check has tt)
        factor_part(smp, rec, what, c, st, kernel, beta, it, tt)
    gstd = smp.debug("gstd")
    s2 = float(smp.get_state("sigma_sq").ravel()[0])
    assert s2 != s_old
    if rss is not None:
        r = T.check_sigma(c, beta, tt, rss, gstd[lay["sigma"][0]], s2, dims, hyp, seed, it)
        rec["fails"] += [f"{what}: {m}" for m in r["fails"]]
        note(rec, ("tempered sigma^2 / 1e-12", kernel), r["worst"])
        note(rec, ("sigma^2 variate", kernel), r["worst_g"])
        print(f"{what}: tempered sigma^2 relative difference / 1e-12: {r['worst']:.3g}; its variate error / allowance {r['worst_g']:.3g}")
        plain = (0.5 * rss + hyp["beta_0"]) / gstd[lay["sigma"][0]]
        if beta != 1.0:
            assert abs(s2 - plain) > 1e-3 * s2, f"{what}: sigma^2 equals the plain form"
    g = J.check_gstd(c, gstd, var)
    rec["fails"] += [f"{what}: {m}" for m in g["fails"]]
    note(rec, ("gstd", "k_factor"), g["worst"])
    TS.slots_equal_state(smp, what, it)

    # ---- the block's own mask
    what = f"{name}:beta{beta}:tt{tt}:full"
    smp.set_state(**st)
    g2_before = smp.debug("gstd2") if c.D else None
    run_tt(smp, what, mask_full, it, beta, tt, **kw)
    assert_sweep_kernel(smp, what, c, kernel)
    cr = rec["routes"]["full"] = assert_unfused(smp, what, c, True)
    hr = rec["routes"]["hyper"] = smp.hyper_route()
    assert hr["hyper"] == "chi", f"{what}: {hr}"
    for nm in ("z_prepared", "pi_prepared"):
        v = smp.debug(nm)[0]
        if v != 0.0:
            rec["fails"].append(f"{what}: \"{nm}\" reads {v}: a tempered sweep took values prepared for another key")
    new = state_now(smp, names_of(c))
    # the Z update: from the pushed state
    sub = dict(worst={}, fails=[])
    TCU.check_z_run(smp, sub, what, c, 0, X, st, cr, it, beta, prepared=False, tt=tt)
    # the chi update: nu, Phi, Z, sigma^2 of the sweep itself, the chi (and eta / xi) of before
    TCU.check_chi_run(smp, sub, what, c, 0, X, dict(st, nu=new["nu"], Phi=new["Phi"], Z=new["Z"], sigma_sq=new["sigma_sq"]), cr, it, beta, tt=tt)
    rec["fails"] += sub["fails"]
    for (form, k), v in sub["worst"].items():
        note(rec, (k, form.split("<")[0]), v)
    # the sweep steps (a chi pass follows: no RSS)
    sweep_part(smp, rec, what, c, st, mask_full, route, beta, th0, s_old)
    # pi / alpha_3, the tables for iteration it + 1, delta / A / gamma / tau
    gstd = smp.debug("gstd")
    g = J.check_gstd(c, gstd, var)
    rec["fails"] += [f"{what}: {m}" for m in g["fails"]]
    note(rec, ("gstd", "k_factor"), g["worst"])
    nv = var["g"].shape[0]
    r = J.check_pi_alpha(c, st["pi"], st["alpha_3"], new["Z"], new["pi"], new["alpha_3"], hyp, mask_full, q=0, it=it, seed=seed,
                         acc_dev=gstd[slice(*lay["acc"])], tt=tt)
    rec["fails"] += [f"{what}: {m}" for m in r["fails"] + R.check_logz(c, new["Z"], smp.debug("logz_part"))]
    note(rec, ("pi / alpha_3 acceptance", hr["pi"]), r["worst"])
    vac = r["vacuous"]
    r = J.check_piprep(c, smp.debug("piprep"), new["pi"], new["alpha_3"], hyp, 0, it + 1, seed=seed)
    rec["fails"] += [f"{what}: {m}" for m in r["fails"]]
    note(rec, ("piprep (iter + 1, tt 0)", "k_factor"), r["worst"])
    r = J.check_hyper(c, st, new, new["nu"], new["Phi"], gstd[:nv], np.zeros(nv), hyp, mask_full)
    rec["fails"] += [f"{what}: {m}" for m in r["fails"]]
    for k in ("delta", "gamma", "tau"):
        note(rec, (k, "k_curve_chi"), r["worst_" + k])
    r = J.check_A(c, st["A"], new["A"], new["delta"], var, hyp, mask_full)
    rec["fails"] += [f"{what}: {m}" for m in r["fails"]]
    vac = max(vac, r["vacuous"])
    if not vac <= J.NONVACUOUS:
        rec["fails"].append(f"{what}: a decision bound is {vac:.3g} of the margin it judges")
    for nm in T.STATE_NAMES + T.SCALAR_NAMES:
        if not np.array_equal(np.ravel(slot_of(smp, nm, it)), np.ravel(new[nm])):
            rec["fails"].append(f"{what}: chain slot {it} of {nm} differs from the working state")
    # the eta / Xi block
    if c.D:
        cvr = rec["routes"]["cov"] = smp.cov_route()
        exp = V.expected_route(c, mask_full)
        assert cvr == exp and cvr["do_xi"], f"{what}: the covariate block launched {cvr}, the case was written for {exp}"
        st_in = dict(st, **{nm: new[nm] for nm in TC.SWEEP_NAMES})
        c0, g0, bc, bg = V.restate_c0(c, smp.debug("rec"), st_in, X)
        sub = dict(worst={}, fails=[])
        TC.judge(smp, c, what, 0, st_in, c0, g0, TC.Run(TC.FULL | TC.SWEEP_WARM, beta=beta, sweep=True), it, sub, g2_before, e_c=bc, e_g=bg, tt=tt)
        rec["fails"] += sub["fails"]
        for k, v in sub["worst"].items():
            if k != "vacuous":
                note(rec, (k, "eta / Xi block"), v)
    smp.close()
    return rec


def single_case(name, beta, tt):
    key = (name, beta, tt)
    if key not in _single:
        try:
            _single[key] = _single_case(name, beta, tt)
        except (Exception, pytest.fail.Exception) as e:      # noqa: BLE001 -- a later test must not take a partial record for a clean one
            _single[key] = e
    if isinstance(_single[key], BaseException):
        raise _single[key]
    return _single[key]


SINGLE = [(nm, b, tt) for nm in T.ROUTED for b, tt in T.SINGLE_SWEEPS]


@pytest.mark.parametrize("name,beta,tt", SINGLE, ids=[f"{n}:beta{b}:tt{tt}" for n, b, tt in SINGLE])
def test_single_tempered_sweep_against_longdouble(name, beta, tt):
    rec = single_case(name, beta, tt)
    assert not rec["fails"], f"{len(rec['fails'])} failures\n" + "\n".join(rec["fails"][:12])


# ---------------------------------------------------------------------------------------------------------------------
# (b), (c), (d) the block
# ---------------------------------------------------------------------------------------------------------------------
def check_trace(rec, what, t, tr, snap_sig, snap_rss, N, la, acc):
    """ladder, schedule, logA, log u, the decision and the block's return values against tempered_ref"""
    fails = []
    if tr["N_t"] != t.N_t:
        fails.append(f"the trace holds N_t = {tr['N_t']}")
    r = T.check_ladder(t.N_t, t.beta_N_t, tr["ladder"])
    fails += r["fails"]
    note(rec, ("ladder", "host"), r["worst"])
    fails += T.check_schedule(t.N_t, tr["ladder"], tr["betas"])
    if tr["sig"][0] != snap_sig or tr["rss"][0] != snap_rss:
        fails.append(f"sig[0], rss[0] = {tr['sig'][0]!r}, {tr['rss'][0]!r}; the state before the block has {snap_sig!r}, {snap_rss!r}")
    r = T.check_logA(t.N_t, tr["ladder"], tr["sig"], tr["rss"], N, tr["logA"])
    fails += r["fails"]
    note(rec, ("logA", "host"), r["worst"] if np.isfinite(r["worst"]) else 1e300)
    d = T.check_decision(tr["log_u"], tr["logA"], tr["accepted"], t.seed, t.it)
    fails += d["fails"]
    note(rec, ("log u", "host"), d["worst"])
    if la != tr["logA"] or bool(acc) != tr["accepted"]:
        fails.append(f"the call returned ({la!r}, {acc}), the trace holds ({tr['logA']!r}, {tr['accepted']})")
    if t.N_t > 1 and not abs(tr["logA"] - tr["log_u"]) > T.UNDECIDED * r["bound"]:
        fails.append(f"|logA - log u| = {abs(tr['logA'] - tr['log_u']):.3g} is within {T.UNDECIDED} x the bound {r['bound']:.3g}")
    print(f"{what}: logA {tr['logA']!r} (restated {r['ref']!r}, error / bound {r['worst']:.3g}), log u {tr['log_u']!r}, accepted {tr['accepted']}; "
          f"ladder error / allowance {rec['worst'][('ladder', 'host')]:.3g}")
    rec["fails"] += [f"{what}: {m}" for m in fails]


def after_block(A, rec, what, t, c, st_after, accepted):
    """(c): two plain iterations from iter + 1; iteration iter + 1 from chain slots with (iter + 1, tt_step 0) keys"""
    import oracle_lib as O
    it1, s1 = t.it + 1, t.it + 1 - t.base
    dyn = A.dyn()
    print(f"{what}: after the {'accepted' if accepted else 'rejected'} block Dyn reads zprep_valid {dyn['zprep_valid']} (iter {dyn['zprep_iter']}, tt {dyn['zprep_tt']}), "
          f"piprep_valid {dyn['piprep_valid']} (iter {dyn['piprep_iter']}), znorm_valid {dyn['znorm_valid']} (iter {dyn['znorm_iter']}, tt {dyn['znorm_tt']})")
    rec["flags"] = (accepted, dyn["zprep_valid"], dyn["piprep_valid"])
    if not accepted and (dyn["zprep_valid"] or dyn["piprep_valid"]):
        rec["fails"].append(f"{what}: after a rejected block zprep_valid = {dyn['zprep_valid']}, piprep_valid = {dyn['piprep_valid']}")
    run_plain(A, what, t.mask, 2, first_iter=it1, seed=t.seed)
    assert A.curve_route()["z"]["form"] == "fused", A.curve_route()
    hyp = J.hyp_of(c, A.cfg)
    rc = A.debug("rec")
    sl = {nm: slot_of(A, nm, s1) for nm in ("nu", "Phi", "chi", "Z", "pi", "alpha_3", "sigma_sq")}
    # the Z update of iteration iter + 1
    Z0 = np.asarray(st_after["Z"], dtype=np.float64)
    Zr, acc = R.reference_z(c, rc, st_after, 1.0, A.cfg.a_Z_PM, 0, it1)
    luu = np.log(O.fill(0, c.n, seed=t.seed, chain=0, it=it1, upd=R.UPD_Z_ACC))
    took_ref, took_dev = (Zr != Z0).any(axis=1), (sl["Z"] != Z0).any(axis=1)
    clear = np.abs(luu - acc) > 1e-6
    tol = R.PROP_MARGIN * R.MEASURED_PROP["Znew"] * U * np.abs(Zr)
    bad = [i for i in range(c.n) if clear[i] and (took_ref[i] != took_dev[i] or not (np.abs(sl["Z"][i] - Zr[i]) <= tol[i]).all())]
    note(rec, ("Z of iter + 1 (slots)", "fused"), float((np.abs(sl["Z"] - Zr) / np.maximum(tol, 1e-300))[clear].max()))
    if bad or not clear.all():
        rec["fails"].append(f"{what}: Z of iteration {it1}: curves {bad} differ from the update restated with (iteration {it1}, tt_step 0) keys "
                            f"({int((~clear).sum())} curves undecided by the reference)")
    print(f"{what}: Z of iteration {it1}: {int(took_dev.sum())} of {c.n} accepted, all as the reference has them: {not bad}")
    # pi / alpha_3
    r = J.check_pi_alpha(c, st_after["pi"], st_after["alpha_3"], sl["Z"], sl["pi"], sl["alpha_3"], hyp, t.mask, q=0, it=it1, seed=t.seed)
    rec["fails"] += [f"{what}: iteration {it1}: {m}" for m in r["fails"]]
    # the chi update, with the oracle's keyed normals of (iter + 1, tt_step 0) and their allowance (check_chi_norm)
    zn = O.fill(1, c.n * c.M, seed=t.seed, chain=0, it=it1, upd=R.UPD_CHI).reshape(c.n, c.M)
    st_chi = dict(st_after, nu=sl["nu"], Phi=sl["Phi"], Z=sl["Z"], sigma_sq=sl["sigma_sq"])
    r = R.check_chi(c, rc, st_chi, sl["chi"], zn, 1.0, None, ztol=32 * U * np.abs(zn) + 4 * U)
    rec["fails"] += [f"{what}: iteration {it1}: {m}" for m in r["fails"]]
    note(rec, ("chi of iter + 1 (slots)", "fused"), r["worst"])
    print(f"{what}: chi of iteration {it1} with the keyed normals of tt_step 0: error / bound {r['worst']:.3g}")


def second_block(A, rec, what, t, c):
    """(d): another block on the sampler of a rejected one (tt_save is reused), two iterations later"""
    it2 = t.it + 2
    names = names_of(c)
    snap, dyn0 = state_now(A, names), A.dyn()
    la, acc = A.tempered_transition(t.mask, it2, 2, 0.9, seed=t.seed)
    tr = A.tt_trace()
    t2 = T.TTCase(t.name, t.family, 2, 0.9, it2, t.seed, t.kernel, None, base=t.base)
    check_trace(rec, what + ": second block", t2, tr, dyn0["sigma2"], dyn0["rss"], A.dims()["n_obs_total"], la, acc)
    now = state_now(A, names)
    s2 = it2 - t.base
    if float(snap["sigma_sq"].ravel()[0]) != tr["sig"][0]:
        rec["fails"].append(f"{what}: second block: sig[0] = {tr['sig'][0]!r} is not the sigma^2 of the state before it")
    if tr["accepted"]:      # the slot holds the accepted draw (its gamma too), the state that draw with the gamma of before the block
        d = A.dyn()
        ok = (np.array_equal(now["gamma"], snap["gamma"]) and not np.array_equal(np.ravel(slot_of(A, "gamma", s2)), np.ravel(snap["gamma"]))
              and (d["sigma2"], d["rss"]) == (tr["sig"][-1], tr["rss"][-1]) and float(now["sigma_sq"].ravel()[0]) == tr["sig"][-1]
              and all(not np.array_equal(now[nm], snap[nm]) for nm in ("nu", "Phi", "chi", "Z", "delta", "tau", "sigma_sq"))
              and all(np.array_equal(np.ravel(slot_of(A, nm, s2)), np.ravel(now[nm])) for nm in names if nm != "gamma"))
    else:
        ok = all(np.array_equal(now[nm], snap[nm]) for nm in names) and all(np.array_equal(np.ravel(slot_of(A, nm, it2 - t.base)), np.ravel(snap[nm])) for nm in names)
    if not ok:
        rec["fails"].append(f"{what}: second block ({'accepted' if tr['accepted'] else 'rejected'}): the state does not follow the hand-over rule")
    rec["second"] = tr["accepted"]


def _block_case(tid):
    import bayesfmmm_amd as bf
    assert (T.SWEEP_WARM, T.COV_FULL) == (bf.sampler.SWEEP_WARM, bf.sampler.COV_MEAN | bf.sampler.COV_XI)
    t = T.BY_ID[tid]
    c = t.case
    rec = dict(routes={}, worst={}, fails=[], accepted=None, family=t.family, flags=None, second=None)
    names = names_of(c)
    st = T.case_state(t)
    slot = t.it - t.base
    smps = []
    for tag in "AB":
        smp = make_sampler(c, slot + 4)
        if t.base:
            smp.set_slot_base(t.base)
        smp.set_state(**st)
        run_plain(smp, f"{tid}: sampler {tag}, the plain run", t.mask, t.it + 1 - t.base, first_iter=t.base, seed=t.seed)
        assert_sweep_kernel(smp, tid, c, t.kernel)
        cr = smp.curve_route()
        assert cr["z"]["form"] == ("standalone" if c.D else "fused") and cr["chi"]["fuse"] == (not c.D), f"{tid}: the plain run took {cr}"
        smps.append(smp)
    A, B = smps
    rec["routes"] = dict(sweep=A.sweep_route(), plain=A.curve_route())
    snap, dyn0, ll0 = state_now(A, names), A.dyn(), float(slot_of(A, "loglik", slot)[0])
    for nm in names:
        assert np.array_equal(snap[nm], B.get_state(nm)), f"{tid}: samplers A and B differ in {nm} before the block"
        assert np.array_equal(np.ravel(slot_of(A, nm, slot)), np.ravel(snap[nm])), f"{tid}: chain slot {slot} of {nm} differs from the state before the block"
    la, acc = A.tempered_transition(t.mask, t.it, t.N_t, t.beta_N_t, seed=t.seed)
    tr = A.tt_trace()
    rec["accepted"] = tr["accepted"]
    check_trace(rec, tid, t, tr, dyn0["sigma2"], dyn0["rss"], A.dims()["n_obs_total"], la, acc)
    assert float(snap["sigma_sq"].ravel()[0]) == dyn0["sigma2"]
    if tr["accepted"] != t.accepted:
        rec["fails"].append(f"{tid}: the block was {'accepted' if tr['accepted'] else 'rejected'}, the oracle has the other outcome")
    if t.N_t == 1 and not (tr["logA"] == 0.0 and tr["accepted"] and tr["ladder"].tolist() == [t.beta_N_t]):
        rec["fails"].append(f"{tid}: N_t = 1: logA {tr['logA']!r}, accepted {tr['accepted']}, ladder {tr['ladder']}")
    # B replays the sweeps
    for l in range(1, 2 * t.N_t + 1):
        run_tt(B, f"{tid}: replay of sweep {l}", t.mask, t.it, float(tr["betas"][l - 1]), l, seed=t.seed)
        assert not B.curve_route()["chi"]["fuse"] and B.curve_route()["z"]["form"] == "standalone"
        d = B.dyn()
        if d["sigma2"] != tr["sig"][l] or d["rss"] != tr["rss"][l] or float(B.get_state("sigma_sq").ravel()[0]) != tr["sig"][l]:
            rec["fails"].append(f"{tid}: sweep {l} replayed with run_tt leaves sigma^2 {d['sigma2']!r}, RSS {d['rss']!r}; the trace holds {tr['sig'][l]!r}, {tr['rss'][l]!r}")
    replay = state_now(B, names)
    after = state_now(A, names)
    slots = {nm: slot_of(A, nm, slot) for nm in names}
    rec["fails"] += [f"{tid}: {m}" for m in T.check_handover(tr["accepted"], after, snap, replay, slots, names)]
    if tr["accepted"]:      # the slot holds the accepted draw, its gamma included
        for nm in names:
            if not np.array_equal(np.ravel(slots[nm]), np.ravel(replay[nm])):
                rec["fails"].append(f"{tid}: chain slot {slot} of {nm} is not the accepted state")
        if np.array_equal(replay["gamma"], snap["gamma"]) or np.array_equal(replay["nu"], snap["nu"]):
            rec["fails"].append(f"{tid}: the tempered sweeps left gamma or nu as they were")
    elif float(slot_of(A, "loglik", slot)[0]) != ll0:
        rec["fails"].append(f"{tid}: the log-likelihood slot reads {float(slot_of(A, 'loglik', slot)[0])!r} after the rejected block, the plain run wrote {ll0!r}")
    d = A.dyn()
    if tr["accepted"]:      # Dyn's scalars are those of the last sweep, which feed PZ(., 0) of a later block
        want = dict(sigma2=tr["sig"][-1], rss=tr["rss"][-1], alpha3=float(replay["alpha_3"].ravel()[0]))
    else:                   # ... and after a rejection those of before the block: sigma^2 and alpha_3 bit for bit
        want = {k: dyn0[k] for k in ("sigma2", "alpha3")}
        # RSS and the log-likelihood are formed AGAIN from the restored state, by k_curve_chi's residual-only pass where the plain run
        # had its update pass: the same block parts summed in another launch, under the counts curve_update_ref.check_total_and_loglik
        # gives the two (the slot's log-likelihood above is held bit for bit)
        tol = dict(rss=(c.nblk + 10) * U * abs(dyn0["rss"]), loglik=8 * U * (abs(dyn0["loglik"]) + dyn0["rss"] / dyn0["sigma2"]))
        for k, b in tol.items():
            note(rec, (f"Dyn::{k} after a rejection", "host"), abs(d[k] - dyn0[k]) / b)
            if not abs(d[k] - dyn0[k]) <= b:
                rec["fails"].append(f"{tid}: after the rejected block Dyn::{k} reads {d[k]!r}, before it {dyn0[k]!r} (allowance {b:.3g})")
    for k, v in want.items():
        if d[k] != v:
            rec["fails"].append(f"{tid}: after the {'accepted' if tr['accepted'] else 'rejected'} block Dyn::{k} reads {d[k]!r}, not {v!r}")
    if (d["iter"], d["slot"], d["tt_step"], d["beta"]) != (t.it + 1, slot + 1, 0, 1.0):
        rec["fails"].append(f"{tid}: after the block Dyn reads iter {d['iter']}, slot {d['slot']}, tt_step {d['tt_step']}, beta {d['beta']}")
    B.close()
    if tid in T.AFTER_BLOCK:
        after_block(A, rec, tid, t, c, dict(st, **after), tr["accepted"])
        if not tr["accepted"]:
            second_block(A, rec, tid, t, c)
    A.close()
    return rec


def block_case(tid):
    if tid not in _blocks:
        try:
            _blocks[tid] = _block_case(tid)
        except (Exception, pytest.fail.Exception) as e:      # noqa: BLE001 -- a later test must not take a partial record for a clean one
            _blocks[tid] = e
    if isinstance(_blocks[tid], BaseException):
        raise _blocks[tid]
    return _blocks[tid]


@pytest.mark.parametrize("tid", [t.id for t in T.CASES])
def test_block_on_two_samplers(tid):
    rec = block_case(tid)
    assert not rec["fails"], f"{len(rec['fails'])} failures\n" + "\n".join(rec["fails"][:12])


def test_chain_batch_is_refused():
    from bayesfmmm_amd import _lib
    c = R.BY_NAME["cubic_P30-benign"]
    smp = make_sampler(c, 4, n_chains=2)
    with pytest.raises(_lib.BfmmmError, match="accepts or rejects one chain: not available on a chain batch"):
        smp.tempered_transition(T.SWEEP_WARM, 1, 2, 0.5)
    with pytest.raises(_lib.BfmmmError, match="no tempered-transition block has run"):
        smp.tt_trace()
    smp.close()


def test_routes_taken_and_largest_errors():
    singles = {k: single_case(*k) for k in SINGLE}
    blocks = {t.id: block_case(t.id) for t in T.CASES}
    worst, kernels, cov = {}, set(), False
    for (name, beta, tt), rec in singles.items():
        ro = rec["routes"]
        kernels.add(ro["sweep"]["kernel"])
        cov |= bool(ro.get("cov", {}).get("do_xi"))
        print(f"{name:22s} beta {beta:<5} tt_step {tt}: k_sweep{'_' + ro['sweep']['kernel'] if ro['sweep']['kernel'] != 'general' else ''}<{ro['sweep']['targ']}>, "
              f"{TCU.z_form_name(ro['full'])}, {TCU.chi_form_name(ro['full'])}, job_hyper {ro['hyper']['hyper']}, job_pi_alpha {ro['hyper']['pi']}"
              + (f", k_cov_group<{ro['cov']['BW']},{ro['cov']['LPC']},{ro['cov']['DX']}> x {ro['cov']['launches']}" if "cov" in ro else ""))
        for k, v in rec["worst"].items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, f"{name}:beta{beta}:tt{tt}")
    outcomes = {}
    for tid, rec in blocks.items():
        if T.BY_ID[tid].N_t > 1:      # (N_t = 1 is always accepted)
            outcomes.setdefault(rec["family"], set()).add(rec["accepted"])
        print(f"{tid:30s} {rec['routes']['sweep']['kernel']:8s} plain run {rec['routes']['plain']['z']['form']:10s} accepted {rec['accepted']}"
              + (f"; flags after the block (accepted, zprep_valid, piprep_valid) {rec['flags']}" if rec["flags"] else "")
              + (f"; second block accepted {rec['second']}" if rec["second"] is not None else ""))
        for k, v in rec["worst"].items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, tid)
    for (what, host), (v, where) in sorted(worst.items()):
        print(f"largest device error / bound, {what:28s} ({host:14s}): {v:.3g} ({where})")
    assert kernels == {"chain", "general", "diag"} and cov, (kernels, cov)
    assert outcomes == {f: {True, False} for f in ("functional", "multivariate", "covariates")}, outcomes
    assert all(v <= 1.0 for v, _ in worst.values()), {k: v for k, v in worst.items() if not v[0] <= 1.0}
