"""The per-curve kernels (k_curve_chi in its general, SMALL and exact instances; k_curve_z stand-alone, lean and fused into
k_curve_chi) on their own, curve by curve: every case of curve_update_ref.CASES pushes a state and runs, on one sampler,

    chi       U_CHI | U_LOGLIK, one iteration: theta, Z, sigma^2 are the pushed state
    z         U_Z alone, one iteration: the stand-alone kernel with in-place proposals
    lean      U_Z | U_PI | U_ALPHA3 | U_NU | U_TAU | U_SIGMA, two iterations: the lean trailing form; the judged update starts from
              chain slot 0 and its output is slot 1
    fused     SWEEP_WARM, two iterations: the form fused into k_curve_chi, judged likewise, and the chi update of iteration 1
    prepared  U_Z alone at first_iter = 2 on the same sampler: the stand-alone kernel taking the PREPARED proposals (asserted
              through "z_prepared"; the z run, behind a pushed state, must report proposals evaluated in place)
    logz      U_PI | U_ALPHA3 without U_Z (do_update == 0): only the block sums of log Z, and Z bit-equal

asserts the instances the run launched (bfmmm_debug_get "curve_route") against the route the case was written for, and holds
every Gauss-Seidel step of every curve, every recorded acceptance value, the block sums and the log-likelihood to the
longdouble bounds of tests/curve_update_ref.py.  Cases on the exact list run a second time with bfmmm_set_exact_instances(0), so
the general instances are judged by the same reference.  The last test prints the routes taken and the largest error / bound
per kernel form."""
import numpy as np
import pytest

import curve_update_ref as R
import factor_ref as F

pytestmark = pytest.mark.gpu

_records = {}
T_SLOTS = 4


@pytest.fixture(autouse=True)
def _recording():
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    lib.bfmmm_set_curve_record(1)
    try:
        yield
    finally:
        lib.bfmmm_set_curve_record(0)
        lib.bfmmm_set_exact_instances(1)


def make_sampler(c, T=T_SLOTS):
    import bayesfmmm_amd as bf
    d = F.case_data(c)
    if c.kind == "mv":
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=c.K, n_eigen=c.M, tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, d["Y"], n_chains=c.nch)
    elif c.kind == "spline":
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=c.deg, tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, d["y"], d["t"], d["ik"], d["bk"], n_chains=c.nch)
    else:
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=max(c.degs), tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, d["y"], basis=d["B"], band=c.band, penalty=d["Pmat"], penalty_band=c.pen_band, n_chains=c.nch)
    if c.D:
        smp.set_covariates(R.case_X(c), covariance_adj=True)
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


def slot_state(smp, st, names, slot):
    """st with the arrays `names` replaced by chain slot `slot`"""
    out = dict(st)
    for nm in names:
        ch = smp.get_chain(nm, slot + 1)
        out[nm] = np.array(ch[..., slot] if ch.ndim > 1 else [ch[slot]])
    return out


def state_now(smp, st):
    out = dict(st)
    for nm in ("nu", "Phi", "chi", "Z", "sigma_sq", "pi", "alpha_3"):
        out[nm] = smp.get_state(nm)
    return out


def assert_route(smp, what, c, kind, exact):
    got, exp = smp.curve_route(), R.expected_route(c, kind, exact)
    assert got == exp, f"{what}: the run launched {got}, the case was written for {exp}"
    return got


def note(rec, form, key, res):
    w = rec["worst"].setdefault((form, key), 0.0)
    rec["worst"][(form, key)] = max(w, res["worst"])
    rec["fails"] += res["fails"]


def z_form_name(route):
    z = route["z"]
    return f"z:{z['form']}<{z['BW']},{z['LPC']},{'cov' if z['COV'] else '-'},KT{z['KT']}{',KEX' if z['KEX'] else ''}>"


def chi_form_name(route):
    x = route["chi"]
    inst = f"K{x['KX']}M{x['MX']}" if x["KX"] else ("SMALL" if x["SMALL"] else "general")
    return f"chi<{x['BW']},{x['LPC']},{'cov' if x['COV'] else '-'},{inst}>"


def check_z_run(smp, rec, what, c, q, X, st_in, route, it, beta=1.0, M=None, prepared=True, tt=0):
    """the Z update the record describes, from the state it started from; the chain slot and the working state must agree;
    prepared: whether the update must have taken the proposals k_factor prepared ahead ("z_prepared"); tt: the sweep of a
    tempered-transition block whose keys the update drew with (0: a plain iteration)"""
    rc = smp.debug("rec")
    Z_out = smp.get_state("Z")
    pre = smp.debug("z_prepared")[0]
    if pre != (1.0 if prepared else 0.0):
        rec["fails"].append(f"{what}: the update {'evaluated its proposals in place' if prepared else 'took prepared proposals'} (z_prepared {pre})")
    pr = R.check_proposal(c, st_in["Z"], smp.debug("z_record"), smp.cfg.a_Z_PM, q, it, tt)
    rec["fails"] += [f"{what} [{z_form_name(route)}]: {m}" for m in pr["fails"]]
    print(f"{what}: proposal error / tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in pr["worst"].items()))
    for k, v in pr["worst"].items():
        note(rec, z_form_name(route), "prop_" + k, dict(worst=v, fails=[]))
    res = R.check_z(c, rc, st_in, smp.debug("z_record"), Z_out, beta, X, M=M, logz_part=smp.debug("logz_part"))
    prior = R.check_prior_terms(c, st_in["Z"], smp.debug("z_record"), st_in["pi"], st_in["alpha_3"])
    res["fails"] = [f"{what} [{z_form_name(route)}]: {m}" for m in res["fails"] + prior + R.check_log_uu(c, smp.debug("z_record"), q, it, tt)]
    slot = smp.get_chain("Z", it + 1)[..., it]
    if not np.array_equal(slot, Z_out):
        res["fails"].append(f"{what}: chain slot {it} of Z differs from the working state")
    if not res["vacuous"] <= R.NONVACUOUS:
        res["fails"].append(f"{what}: an acceptance bound is {res['vacuous']:.3g} of the likelihood difference it judges")
    print(f"{what}: {z_form_name(route)}: acceptance error / bound {res['worst']:.3g} (curve {res['where']}), {res['accepted']} of {c.n} accepted, "
          f"{res['forced']} forced")
    note(rec, z_form_name(route), "acc", res)
    if c.D:      # what only k_curve_z writes for the Phi / nu block of a covariate model
        g = R.check_stil(c, rc, st_in, Z_out, X, smp.debug("stil"), smp.debug("yyp_part"))
        g["fails"] = [f"{what} [{z_form_name(route)}]: {m}" for m in g["fails"]]
        print(f"{what}: stil error / bound {g['worst']:.3g}, yyp_part {g['worst_yyp']:.3g}")
        note(rec, z_form_name(route), "stil", g)
        note(rec, z_form_name(route), "yyp", dict(worst=g["worst_yyp"], fails=[]))
    return res


def check_cfull_run(smp, rec, what, c, X, st_in, chi_new, route):
    """covariate models: c_i and G_i c_i as k_curve_chi left them (the mask has no eta / Xi step: nothing rewrote them)"""
    g = R.check_cfull(c, smp.debug("rec"), st_in, chi_new, X, smp.debug("cfull"), smp.debug("gfull"))
    rec["fails"] += [f"{what} [{chi_form_name(route)}]: {m}" for m in g["fails"]]
    print(f"{what}: cfull error / bound {g['worst']:.3g}, gfull {g['worst_g']:.3g}")
    note(rec, chi_form_name(route), "cfull", dict(worst=g["worst"], fails=[]))
    note(rec, chi_form_name(route), "gfull", dict(worst=g["worst_g"], fails=[]))


def check_chi_run(smp, rec, what, c, q, X, st_in, route, it, beta=1.0, tt=0):
    """the chi update of iteration `it` from the state it started from, the residual sums and the log-likelihood"""
    rc = smp.debug("rec")
    chi_new = smp.get_state("chi")
    zn = smp.debug("chi_norm").reshape(c.M, c.n).T
    res = R.check_chi(c, rc, st_in, chi_new, zn, beta, X)
    res["fails"] = [f"{what} [{chi_form_name(route)}]: {m}" for m in res["fails"] + R.check_chi_norm(c, smp.debug("chi_norm"), q, it, tt)]
    if not np.array_equal(smp.get_chain("chi", it + 1)[..., it], chi_new):
        res["fails"].append(f"{what}: chain slot {it} of chi differs from the working state")
    if not res["vacuous"] <= R.NONVACUOUS:
        res["fails"].append(f"{what}: a chi bound is {res['vacuous']:.3g} of the step it judges")
    print(f"{what}: {chi_form_name(route)}: chi step error / bound {res['worst']:.3g} at (curve, m) {res['where']}")
    note(rec, chi_form_name(route), "chi", res)
    if c.D == 0:      # (with covariates the eta / Xi block's residual pass rewrites rss_part: kernels_cov.hip)
        part = smp.debug("rss_part")
        g = R.check_rss(c, rc, st_in, chi_new, part, X)
        s2 = float(smp.get_state("sigma_sq").ravel()[0])
        ll = float(smp.get_state("loglik").ravel()[0])
        g["fails"] += R.check_total_and_loglik(c, part, float(smp.debug("rss")[0]), ll, s2, smp.dims()["n_obs_total"])
        if smp.get_chain("loglik", it + 1)[it] != ll:
            g["fails"].append(f"{c.name}: chain slot {it} of loglik differs from the working state")
        g["fails"] = [f"{what} [{chi_form_name(route)}]: {m}" for m in g["fails"]]
        print(f"{what}: rss_part error / bound {g['worst']:.3g}")
        note(rec, chi_form_name(route), "rss", g)


def run_case(name, exact):
    """every run of one case on one sampler, checked: dict(routes, worst {(form, what): error / bound}, fails); memoised"""
    key = (name, exact)
    if key in _records:
        return _records[key]
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    Sm = bf.sampler
    assert (Sm.U_Z, Sm.U_PI, Sm.U_ALPHA3, Sm.U_NU, Sm.U_TAU, Sm.U_SIGMA, Sm.U_CHI, Sm.U_LOGLIK) == (
        R.U_Z, R.U_PI, R.U_ALPHA3, R.U_NU, R.U_TAU, R.U_SIGMA, R.U_CHI, R.U_LOGLIK)
    _lib.load().bfmmm_set_exact_instances(1 if exact else 0)
    c = R.BY_NAME[name]
    X = R.case_X(c)
    smp = make_sampler(c)
    states = [R.case_state(c, q) for q in range(c.nch)]
    rec = dict(routes={}, worst={}, fails=[], out=[])
    kw = dict(seed=R.SEED, chain=0)
    kinds = ("chi", "z", "logz", "lean", "fused", "prepared") if exact else ("chi", "z", "fused")
    betas = (1.0, 0.37) if name == R.BETA_CASE and exact else (1.0,)
    for beta in betas:
        tag = f"{name}{'' if exact else ':general'}{'' if beta == 1.0 else f':beta{beta}'}"
        if "chi" in kinds:
            push(smp, states)
            run_sampler(smp, f"{tag}:chi", R.MASK_CHI, 1, beta=beta, **kw)
            route = rec["routes"]["chi"] = assert_route(smp, f"{tag}:chi", c, "chi", exact)
            for q, st in enumerate(states):
                smp.select_chain(q)
                check_chi_run(smp, rec, f"{tag}:chi, chain {q}", c, q, X, st, route, 0, beta)
                if c.D:
                    check_cfull_run(smp, rec, f"{tag}:chi, chain {q}", c, X, st, smp.get_state("chi"), route)
                assert np.array_equal(smp.get_state("Z"), st["Z"]), f"{tag}:chi: Z changed without U_Z"
                rec["out"].append(smp.get_state("chi"))
        if "z" in kinds:
            push(smp, states)
            run_sampler(smp, f"{tag}:z", R.U_Z, 1, beta=beta, **kw)
            route = rec["routes"]["z"] = assert_route(smp, f"{tag}:z", c, "z", exact)
            for q, st in enumerate(states):
                smp.select_chain(q)
                check_z_run(smp, rec, f"{tag}:z, chain {q}", c, q, X, st, route, 0, beta, prepared=False)
                if c.D:      # the residual-only pass behind it (mode 1): c_i = c0 at the new Z
                    check_cfull_run(smp, rec, f"{tag}:z, chain {q}", c, X, dict(st, Z=smp.get_state("Z")), st["chi"], route)
                rec["out"].append(smp.get_state("Z"))
    if "logz" in kinds:      # do_update == 0: only the block sums of log Z, Z bit-equal
        push(smp, states)
        run_sampler(smp, f"{name}:logz", R.MASK_LOGZ, 1, **kw)
        rec["routes"]["logz"] = assert_route(smp, f"{name}:logz", c, "logz", exact)
        for q, st in enumerate(states):
            smp.select_chain(q)
            Zs = smp.get_state("Z")
            if not np.array_equal(Zs, st["Z"]):
                rec["fails"].append(f"{name}:logz, chain {q}: Z changed without U_Z")
            if not c.zero:
                rec["fails"] += [f"{name}:logz, chain {q}: {m}" for m in R.check_logz(c, Zs, smp.debug("logz_part"))]
            try:      # a run without a Z update stores no record: the call must say so, not return the previous run's
                smp.debug("z_record")
                rec["fails"].append(f"{name}:logz, chain {q}: z_record answered after a run without a Z update")
            except _lib.BfmmmError as e:
                assert "stored no record" in str(e), e
    if "lean" in kinds:
        push(smp, states)
        run_sampler(smp, f"{name}:lean", R.MASK_LEAN, 2, **kw)
        route = rec["routes"]["lean"] = assert_route(smp, f"{name}:lean", c, "lean", exact)
        for q, st in enumerate(states):
            smp.select_chain(q)
            check_z_run(smp, rec, f"{name}:lean, chain {q}", c, q, X, slot_state(smp, st, ("nu", "Z", "sigma_sq", "pi", "alpha_3"), 0), route, 1)
    if "fused" in kinds:
        push(smp, states)
        run_sampler(smp, f"{tag}:fused", Sm.SWEEP_WARM, 2, **kw)
        route = rec["routes"]["fused"] = assert_route(smp, f"{tag}:fused", c, "fused", exact)
        for q, st in enumerate(states):
            smp.select_chain(q)
            s0 = slot_state(smp, st, ("nu", "Phi", "chi", "Z", "sigma_sq", "pi", "alpha_3"), 0)
            check_z_run(smp, rec, f"{tag}:fused, chain {q}", c, q, X, s0, route, 1)
            s1 = slot_state(smp, st, ("nu", "Phi", "Z", "sigma_sq"), 1)
            s1["chi"] = s0["chi"]
            check_chi_run(smp, rec, f"{tag}:fused, chi of iteration 1, chain {q}", c, q, X, s1, route, 1)
    if "prepared" in kinds:
        before = []
        for q, st in enumerate(states):
            smp.select_chain(q)
            before.append(state_now(smp, st))
        run_sampler(smp, f"{name}:prepared", R.U_Z, 1, first_iter=2, **kw)
        route = rec["routes"]["prepared"] = assert_route(smp, f"{name}:prepared", c, "prepared", exact)
        for q, st in enumerate(before):
            smp.select_chain(q)
            check_z_run(smp, rec, f"{name}:prepared, chain {q}", c, q, X, st, route, 2)
    if name == "cubic_P30-benign" and exact:      # M = 0 through phi_chi_zero: u_k = nu_k
        push(smp, states)
        run_sampler(smp, f"{name}:z:pcz", R.U_Z, 1, phi_chi_zero=True, **kw)
        route = assert_route(smp, f"{name}:z:pcz", c, "z", exact)
        check_z_run(smp, rec, f"{name}:z:pcz", c, 0, X, states[0], route, 0, M=0, prepared=False)
        push(smp, states)
        run_sampler(smp, f"{name}:lean:pcz", R.MASK_LEAN, 2, phi_chi_zero=True, **kw)
        route = assert_route(smp, f"{name}:lean:pcz", c, "lean", exact)
        check_z_run(smp, rec, f"{name}:lean:pcz", c, 0, X, slot_state(smp, states[0], ("nu", "Z", "sigma_sq", "pi", "alpha_3"), 0), route, 1, M=0)
    smp.close()
    if c.nch > 1:       # every chain has its own state: a chain offset would have compared (or written) the wrong one
        per = len(rec["out"]) // c.nch
        for j in range(0, len(rec["out"]), c.nch):
            for q in range(1, c.nch):
                assert not np.array_equal(rec["out"][j], rec["out"][j + q]), f"{name}: chains 0 and {q} hold the same output ({per} outputs per chain)"
    rec.pop("out")
    _records[key] = rec
    return rec


def _params():
    out = [(c.name, True) for c in R.CASES]
    out += [(c.name, False) for c in R.CASES if c.exact_built() and c.K <= 4 and c.M <= 8]
    return out


PARAMS = _params()


@pytest.mark.parametrize("name,exact", PARAMS, ids=[f"{n}{'' if e else ':general'}" for n, e in PARAMS])
def test_every_curve_against_longdouble(name, exact):
    rec = run_case(name, exact)
    assert not rec["fails"], f"{len(rec['fails'])} failures\n" + "\n".join(rec["fails"][:12])


def test_recording_changes_nothing_and_fails_cleanly_when_off():
    """a short SWEEP_WARM trajectory with recording on and off: bit-equal chains; "z_record" is refused while recording is off"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    c = R.BY_NAME["cubic_P30-benign"]
    chains = {}
    for on in (1, 0):
        lib.bfmmm_set_curve_record(on)
        smp = make_sampler(c, T=6)
        smp.set_state(**R.case_state(c))
        run_sampler(smp, f"recording {on}", bf.sampler.SWEEP_WARM, 3, seed=R.SEED)
        run_sampler(smp, f"recording {on}, second run", bf.sampler.SWEEP_WARM, 3, first_iter=3, seed=R.SEED)
        chains[on] = {nm: smp.get_chain(nm) for nm in ("Z", "chi", "nu", "Phi", "sigma_sq", "pi", "alpha_3", "loglik")}
        if on:
            assert smp.debug("z_record").shape == ((6 + c.K) * c.n,)
        else:
            with pytest.raises(_lib.BfmmmError, match="recording is off"):
                smp.debug("z_record")
        smp.close()
    for nm in chains[1]:
        assert np.array_equal(chains[1][nm], chains[0][nm]), f"{nm}: the chains with and without recording differ"
    assert len({float(x) for x in chains[1]["sigma_sq"].ravel()}) == 6


def test_routes_taken_and_largest_errors():
    """the table of the instances the runs took, read from "curve_route", and the largest device error / bound per kernel form"""
    recs = {p: run_case(*p) for p in PARAMS}
    worst, seen_z, seen_chi = {}, set(), set()
    for (name, exact), rec in recs.items():
        for kind, ro in rec["routes"].items():
            z, x = ro["z"], ro["chi"]
            seen_z.add((z["form"], z["BW"], z["LPC"], z["COV"], z["KT"], z["KEX"]))
            if kind in ("chi", "fused"):
                seen_chi.add((x["BW"], x["LPC"], x["COV"], x["SMALL"], x["KX"], x["MX"]))
            print(f"{name + ('' if exact else ':general'):34s} {kind:9s} {z_form_name(ro):40s} {chi_form_name(ro):30s} mode {x['mode']} fuse {int(x['fuse'])}")
        for (form, what), w in rec["worst"].items():
            fam = form.split("<")[0] + ":" + what
            if w > worst.get(fam, (0.0, ""))[0]:
                worst[fam] = (w, f"{name}{'' if exact else ':general'} {form}")
    for fam, (w, where) in sorted(worst.items()):
        print(f"largest device error / bound, {fam}: {w:.3g} ({where})")
    need_z = {("standalone", bw, lpc) for bw in (0, 1, 2, 3, 4, 5, 15, 31) for lpc in (32, 64)}
    need_z |= {("lean", bw, lpc) for bw in (0, 1, 2, 3, 4, 5) for lpc in (32, 64)} | {("fused", bw, lpc) for bw in (0, 1, 2, 3, 4, 5, 15, 31) for lpc in (32, 64)}
    got_z = {(f, bw, lpc) for f, bw, lpc, *_ in seen_z}
    assert need_z <= got_z, f"Z routes not taken: {sorted(need_z - got_z)}"
    assert {(f, kt, kex) for f, _, _, _, kt, kex in seen_z} >= {("standalone", 4, False), ("standalone", 8, False), ("standalone", 3, True), ("lean", 4, False),
                                                                ("lean", 3, True), ("fused", 4, False), ("fused", 8, False), ("fused", 3, True)}
    assert any(cov for _, _, _, cov, _, _ in seen_z)
    need_chi = {(3, 32, False, True, K, M) for K in (2, 3, 4) for M in range(1, 9)} | {(3, 32, False, True, 0, 0), (3, 32, False, False, 0, 0)}
    need_chi |= {(bw, lpc, cov, True, K, M) for bw, lpc, cov in R.CHI_EXACT_COMBOS for K in (2, 3, 4) for M in range(1, 9)}
    need_chi |= {(3, 64, True, True, 0, 0)}
    assert need_chi <= seen_chi, f"chi routes not taken: {sorted(need_chi - seen_chi)}"
    for bw in (0, 1, 2, 3, 4, 5, 15, 31):
        for lpc in (32, 64):
            assert any(x[0] == bw and x[1] == lpc for x in seen_chi), (bw, lpc)
