"""The sweep kernels (k_sweep_chain<0..5>, k_sweep staged / direct / diagonal branch, k_sweep_diag<RPL, mv>) on their own, step
by step: every run of sweep_ref.RUNS pushes a state, runs ONE iteration, asserts the kernel the run launched
(bfmmm_debug_get "sweep_route") against the route the case was written for, reads the sweep's inputs as k_factor left them
("H", "tvec", "Cmat", "Lz", "rvec", "hq"), theta and -- where U_SIGMA is set -- "rss", and holds each of the K M + K dependent
draws to the per-entry longdouble bound of tests/sweep_ref.py (each step judged alone, from the device's own earlier steps) and
the RSS to its bound.  Directions outside the mask must come back bit-equal, the chain slots the sweep writes must equal the
working state bit for bit, every run must end with status 0.  Further: a second run with another mask on the same sampler
(the step tables must follow the mask), the last of 12 iterations replayed from the captured graphs (the hand-off sentinels
and sigma^2 between launches), a 4-chain batch on two streams.  The last test prints the table of routes taken and the largest
device error / bound per kernel.

Masks: subsets of U_NU | U_PHI | U_SIGMA only -- no chi pass, so nothing rewrites Dyn::rss after the sweep (sweep_ref.py)."""
import numpy as np
import pytest

import factor_ref as F
import sweep_ref as S

pytestmark = pytest.mark.gpu

_records = {}


def make_sampler(c, T=2):
    """as tests/test_gpu_factor.py::make_sampler, with T slots and the one-hot ("step") bases"""
    import bayesfmmm_amd as bf
    d = F.case_data(c)
    if c.kind == "mv":
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=c.K, n_eigen=c.M, tot_mcmc_iters=T)
        return bf.Sampler(cfg, d["Y"], n_chains=c.nch)
    if c.kind == "spline":
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=c.deg, tot_mcmc_iters=T)
        return bf.Sampler(cfg, d["y"], d["t"], d["ik"], d["bk"], n_chains=c.nch)
    deg = 1 if c.kind == "step" else max(c.degs)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=deg, tot_mcmc_iters=T)
    return bf.Sampler(cfg, d["y"], basis=d["B"], band=c.band, penalty=d["Pmat"], penalty_band=c.pen_band, n_chains=c.nch)


def run_sampler(smp, what, *a, **kw):
    """bfmmm_run must return 0; a hand-off spin that ran out is a failure of its own"""
    try:
        smp.run(*a, **kw)
    except Exception as e:      # noqa: BLE001 -- the binding raises on every non-zero status
        if "hand-off inside the sweep kernel timed out" in str(e):
            pytest.fail(f"{what}: a hand-off spin of k_sweep_chain ran out (status bit 4): {e}")
        pytest.fail(f"{what}: bfmmm_run did not return 0: {e}")
    for q in range(smp.n_chains):
        smp.select_chain(q)
        status = int(smp.get_state("status")[0])
        assert not status & 6, f"{what}, chain {q}: a hand-off ran out or a fused update had no proposals (status {status})"
        assert status == 0, f"{what}, chain {q}: status word {status}"


def full_rows(c, MD):
    """rows of the device's theta (K (M + 1) x P) of the active directions a = j MD + mt"""
    return [(a // MD) * (c.M + 1) + a % MD for a in range(c.K * MD)]


def read_inputs(smp, c, MD):
    d = smp.dims()
    A, P = c.K * MD, c.P
    assert (d["K"], d["P"], d["M"], d["MD"], d["A"], d["BW"], d["BWP"]) == (c.K, P, c.M, MD, A, c.BW, c.BWP), (c.name, d)
    return dict(H=smp.debug("H").reshape(d["R"], d["LG"]), tvec=smp.debug("tvec").reshape(A, P), Cmat=smp.debug("Cmat").reshape(A, P, P),
                Lz=smp.debug("Lz").reshape(A, P), rvec=smp.debug("rvec").reshape(A, P), hq=smp.debug("hq").reshape(A, P), YY=d["YY"])


def owner_note(route, s):
    if route["kernel"] != "chain":
        return f"k_sweep{'_diag' if route['kernel'] == 'diag' else ''}: one workgroup owns every row"
    if s < 3:
        return f"r of step {s}: every earlier delta applied by the chain wave; mat-vec by the chain wave"
    return (f"r of step {s}: deltas 0 .. {s - 3} applied by a row thread (rank {s}), deltas {s - 2}, {s - 1} and the mat-vec by the "
            f"chain wave")


def check_chain(what, c, mask, MD, route, th0, th1, inp, f, rss):
    """(worst step ratio, rss ratio or None, failure messages) of one chain of one run"""
    fails = []
    r = S.check_steps(c, mask, th0, th1, inp["H"], inp["Cmat"], inp["Lz"], inp["rvec"], inp["hq"], f, MD)
    for x in r["steps"]:
        print(f"{what}: step {x['s']} (j {x['j']}, mt {x['mt']}): error / bound {x['ratio']:.3g} at p {x['p']}")
        # (the bound is small against the step it judges on the device too: a draw left at theta0 cannot pass)
        if not x["bmax"] <= 1e-3 * x["dmax"]:
            fails.append(f"{what}: step {x['s']}: the bound ({x['bmax']:.3g}) is not small against the step ({x['dmax']:.3g})")
        if not x["ratio"] <= 1.0:
            fails.append(f"{what}, kernel {route}: step {x['s']}, direction (j {x['j']}, mt {x['mt']}), row p {x['p']}: value {x['value']!r}, "
                         f"reference {x['ref']!r}, error / bound {x['ratio']:.3g} (bound {x['bound']:.3g}); {owner_note(route, x['s'])}")
    if not r["frozen_ok"] or (not r["ok"] and not fails):
        fails.append(f"{what}, kernel {route}: {r['msg']}")
    g = None
    if mask & S.U_SIGMA:
        g = S.check_rss(c, mask, th0, th1, inp["H"], inp["tvec"], inp["rvec"], inp["hq"], inp["YY"], rss, MD)
        print(f"{what}: {g['msg']}")
        if not g["ok"]:
            fails.append(f"{what}, kernel {route}: {g['msg']}")
    return r["worst"], (g["ratio"] if g else None), fails


def check_sigma(smp, what, q, it, rss, sigma_new):
    """updateSigma of a plain run (UpdateSigma.h:22-58; tt_step = 0 whatever beta is): sigma^2 = 1 / Gamma(a, 1 / b), a = alpha_0 +
    sum_i (n_i / 2) (integer division; multivariate: n P / 2), b = RSS / 2 + beta_0 -- from the device's RSS and the oracle's
    keyed gamma variate.  1e-12 relative: the variate passes through log / pow / sqrt of two math libraries, a few units of
    2^-53 each, against the factor beta = 0.37 (or a = sum_i beta n_i / 2) a tempered form would show."""
    import oracle_lib as O
    d = smp.dims()
    cfg = smp.cfg
    shape = (d["n_obs_total"] // 2 if cfg.model == 1 else d["half_sum"]) + cfg.alpha_0
    g = O.fill(2, 1, seed=F.SEED, chain=q, it=it, upd=14, p1=float(shape), p2=1.0)[0]
    ref = (0.5 * rss + cfg.beta_0) / g
    rel = abs(sigma_new - ref) / ref
    print(f"{what}: sigma^2 {sigma_new!r}, restated {ref!r}, relative difference {rel:.3g}")
    return [] if rel <= 1e-12 else [f"{what}: sigma^2 {sigma_new!r}, UpdateSigma.h from the device's RSS gives {ref!r} (relative {rel:.3g})"]


def slots_equal_state(smp, what, slot):
    """the chain slots the sweep writes (nu, Phi, sigma_sq of `slot`) equal the working state bit for bit"""
    for nm in ("nu", "Phi", "sigma_sq"):
        ch = smp.get_chain(nm, slot + 1)
        got = ch[..., slot] if ch.ndim > 1 else ch[slot]
        cur = smp.get_state(nm)
        assert np.array_equal(np.ravel(got), np.ravel(cur)), f"{what}: chain slot {slot} of {nm} differs from the working state"


def run_checked(rid):
    """one iteration of run `rid`, checked: dict(route, step, rss, fails); memoised (the table test reads every record)"""
    if rid in _records:
        return _records[rid]
    import bayesfmmm_amd as bf
    Sm = bf.sampler
    assert (Sm.U_PHI, Sm.U_NU, Sm.U_SIGMA) == (S.U_PHI, S.U_NU, S.U_SIGMA)
    run = S.RUN_BY_ID[rid]
    c, MD = run.case, run.MD
    smp = make_sampler(c)
    states = [F.case_state(c, q) for q in range(c.nch)]
    for q, st in enumerate(states):
        smp.select_chain(q)
        smp.set_state(**st)
    run_sampler(smp, rid, run.mask, 1, seed=F.SEED, chain=0, phi_chi_zero=run.pcz, beta=run.beta)
    route = smp.sweep_route()
    exp = S.expected_route(c, MD)
    got = (route["kernel"], route["targ"], route["mv"], route["direct"], route["threads"])
    assert got == exp, f"{rid}: the run launched {got}, the case was written for {exp} (kernel, template argument, mv, direct, threads)"
    rec = dict(route=route, step=0.0, rss=None, fails=[], theta1=[])
    rows = full_rows(c, MD)
    for q, st in enumerate(states):
        smp.select_chain(q)
        what = f"{rid}, chain {q}"
        inp = read_inputs(smp, c, MD)
        th_full = smp.debug("theta").reshape(c.K * (c.M + 1), c.P)
        th0_full = S.theta_of(c, st)
        th0, th1 = S.theta_of(c, st, MD), th_full[rows]
        idle = [x for x in range(c.K * (c.M + 1)) if x not in rows]
        assert np.array_equal(th_full[idle], th0_full[idle]), f"{what}: inactive directions (phi_chi_zero) changed"
        assert np.array_equal(S.theta_of(c, dict(nu=smp.get_state("nu"), Phi=smp.get_state("Phi"))), th_full), f"{what}: theta and the state differ"
        f = run.beta / float(st["sigma_sq"][0])
        rss = float(smp.debug("rss")[0]) if run.mask & S.U_SIGMA else None
        w, g, fails = check_chain(what, c, run.mask, MD, route, th0, th1, inp, f, rss)
        if rss is not None:
            fails += check_sigma(smp, what, q, 0, rss, float(smp.get_state("sigma_sq").ravel()[0]))
        rec["step"] = max(rec["step"], w)
        rec["rss"] = g if rec["rss"] is None else max(rec["rss"], g)
        rec["fails"] += fails
        rec["theta1"].append(th1)
        slots_equal_state(smp, what, 0)
        if not run.mask & S.U_SIGMA:
            assert np.array_equal(smp.get_state("sigma_sq").ravel(), st["sigma_sq"]), f"{what}: sigma^2 changed without U_SIGMA"
    smp.close()
    if c.nch > 1:       # every chain has its own state: a chain offset would have compared (or written) the wrong one
        for q in range(1, c.nch):
            assert not np.array_equal(rec["theta1"][0], rec["theta1"][q]), f"{rid}: chains 0 and {q} hold the same theta1"
    rec.pop("theta1")
    _records[rid] = rec
    return rec


@pytest.mark.parametrize("rid", [r.id for r in S.RUNS])
def test_every_step_against_longdouble(rid):
    rec = run_checked(rid)
    assert not rec["fails"], "\n".join(rec["fails"])


def _state_now(smp, c):
    return dict(nu=smp.get_state("nu"), Phi=smp.get_state("Phi")), float(smp.get_state("sigma_sq").ravel()[0])


@pytest.mark.parametrize("name", ["cubic_P30-benign", "quint_P27-stiff"])
def test_step_tables_follow_the_mask(name):
    """U_NU | U_PHI, then U_NU alone on the same sampler: the step tables are built once per run and must be rebuilt"""
    c = S.BY_NAME[name]
    smp = make_sampler(c, T=4)
    smp.set_state(**F.case_state(c))
    full = S.U_NU | S.U_PHI
    run_sampler(smp, name, full, 1, seed=F.SEED)
    route = smp.sweep_route()
    assert route["kernel"] == "chain"
    st1, s2 = _state_now(smp, c)
    th0 = S.theta_of(c, st1)
    run_sampler(smp, name, S.U_NU | S.U_SIGMA, 1, first_iter=1, seed=F.SEED)
    assert smp.sweep_route() == route
    inp = read_inputs(smp, c, c.MD)
    th1 = smp.debug("theta").reshape(c.A, c.P)
    w, g, fails = check_chain(f"{name}: second run (U_NU | U_SIGMA)", c, S.U_NU | S.U_SIGMA, c.MD, route, th0, th1, inp, 1.0 / s2,
                              float(smp.debug("rss")[0]))
    slots_equal_state(smp, name, 1)
    # ... and back: the Phi steps return
    st2, s3 = _state_now(smp, c)
    run_sampler(smp, name, full, 1, first_iter=2, seed=F.SEED)
    inp = read_inputs(smp, c, c.MD)
    w2, _, fails2 = check_chain(f"{name}: third run (U_NU | U_PHI)", c, full, c.MD, route, S.theta_of(c, st2), smp.debug("theta").reshape(c.A, c.P),
                                inp, 1.0 / s3, None)
    smp.close()
    assert not fails + fails2, "\n".join(fails + fails2)


def test_last_iteration_of_a_replayed_run():
    """12 iterations in one run: one replay of the 10-unrolled graph and a remainder graph.  The last iteration alone is checked:
    theta0 = chain slot 10, sigma^2 = slot 10, theta1 = slot 11 (H does not change: Z and chi are not in the mask)."""
    c = S.BY_NAME["cubic_P30-benign"]
    smp = make_sampler(c, T=12)
    smp.set_state(**F.case_state(c))
    mask = S.U_NU | S.U_PHI | S.U_SIGMA
    run_sampler(smp, "replay", mask, 12, seed=F.SEED)
    route = smp.sweep_route()
    assert (route["kernel"], route["targ"]) == ("chain", 3)
    nu, Phi, s2 = smp.get_chain("nu"), smp.get_chain("Phi"), smp.get_chain("sigma_sq").ravel()
    th0 = S.theta_of(c, dict(nu=nu[..., 10], Phi=Phi[..., 10]))
    th1 = S.theta_of(c, dict(nu=nu[..., 11], Phi=Phi[..., 11]))
    assert np.array_equal(th1, smp.debug("theta").reshape(c.A, c.P))
    assert len({float(x) for x in s2}) == 12 and not np.array_equal(th0, th1)
    inp = read_inputs(smp, c, c.MD)
    w, g, fails = check_chain("replay: iteration 11", c, mask, c.MD, route, th0, th1, inp, 1.0 / float(s2[10]), float(smp.debug("rss")[0]))
    slots_equal_state(smp, "replay", 11)
    smp.close()
    assert not fails, "\n".join(fails)


def test_routes_taken_and_largest_errors():
    """the table of the routes the runs took, read from "sweep_route", and the largest device error / bound per kernel"""
    recs = {r.id: run_checked(r.id) for r in S.RUNS}
    seen, worst = set(), {}
    print(f"{'run':58s} {'kernel':8s} {'arg':>3s} {'mv':>5s} {'direct':>6s} {'threads':>7s} {'step err/bound':>14s} {'rss err/bound':>14s}")
    for rid, rec in recs.items():
        ro = rec["route"]
        seen.add((ro["kernel"], ro["targ"], ro["mv"], ro["direct"]))
        if ro["kernel"] == "chain":
            c = S.RUN_BY_ID[rid].case
            A = c.K * S.RUN_BY_ID[rid].MD
            seen.update(("lanes", l) for l in (4, 8, 16) if ro["threads"] == 64 + (A * l + 63) // 64 * 64 and l == (4 if (c.P + 1) // 2 <= 4 else 8 if (c.P + 1) // 2 <= 8 else 16))
        rss = "-" if rec["rss"] is None else f"{rec['rss']:.3g}"
        print(f"{rid:58s} {ro['kernel']:8s} {ro['targ']:3d} {str(ro['mv']):>5s} {str(ro['direct']):>6s} {ro['threads']:7d} {rec['step']:14.3g} {rss:>14s}")
        k = worst.setdefault(ro["kernel"], [0.0, "", 0.0, ""])
        if rec["step"] > k[0]:
            k[0], k[1] = rec["step"], rid
        if rec["rss"] is not None and rec["rss"] > k[2]:
            k[2], k[3] = rec["rss"], rid
    for kern, (a, ra, b, rb) in sorted(worst.items()):
        print(f"largest device error / bound, {kern}: step {a:.3g} ({ra}), RSS {b:.3g} ({rb})")
    need = ({("chain", b, False, False) for b in range(1, 6)} | {("chain", 0, False, False), ("chain", 0, True, False)}
            | {("lanes", l) for l in (4, 8, 16)}
            | {("general", 0, False, False), ("general", 0, False, True), ("general", 0, True, True)}
            | {("diag", 1, True, False), ("diag", 2, True, False), ("diag", 8, True, False), ("diag", 1, False, False)})
    assert need <= seen, f"routes not taken: {sorted(need - seen)}"
    limit = {rid: rec["route"] for rid, rec in recs.items() if rid.startswith(("cubic_P30_K4M5", "cubic_P30_K5M4"))}
    assert [v["kernel"] for _, v in sorted(limit.items())] == ["chain", "general"], limit
