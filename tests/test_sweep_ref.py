"""The reference of tests/test_gpu_sweep.py checked without a device: both float64 emulations of the sweep kernels' orders of
operations against the step bound and the RSS bound on every run of sweep_ref.RUNS (each at most a quarter of its bound), every
mutation of either emulation rejected at ten times the bound on named cases, the bound small against the step it judges (non-
vacuity, from the reference alone) and the step order asserted against the oracle's updatePhi / updateNu loops."""
import numpy as np
import pytest

import factor_ref as F
import sweep_ref as S

pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is no wider than double on this platform")

EMUS = (("general", S.emulate_general), ("chain", S.emulate_chain))


def _emus(c):
    return [(nm, emu) for nm, emu in EMUS if nm == "general" or S.chain_layout_ok(c)]


def _steps(run, inp, th1):
    return S.check_steps(run.case, run.mask, inp["theta0"], th1, inp["H"], inp["Cmat"], inp["Lz"], inp["rvec"], inp["hq"], inp["f"], run.MD)


def _rss(run, inp, th1, rss):
    return S.check_rss(run.case, run.mask, inp["theta0"], th1, inp["H"], inp["tvec"], inp["rvec"], inp["hq"], inp["YY"], rss, run.MD)


def test_emulations_pass_both_bounds():
    """the general emulation on every run, the chain emulation on every run its layout can hold (P <= 32, band <= 5)"""
    worst = {(k, nm): (0.0, "") for k in ("step", "rss") for nm, _ in EMUS}
    for run in S.RUNS:
        for q in range(run.case.nch):
            inp = S.cpu_inputs(run, q)
            for nm, emu in _emus(run.case):
                th1, rss = emu(run.case, run.mask, inp, run.MD)
                r = _steps(run, inp, th1)
                assert r["ok"], f"{nm} emulation, {run.id}: {r['msg']}"
                g = _rss(run, inp, th1, rss)
                assert g["ok"], f"{nm} emulation, {run.id}: {g['msg']}"
                for k, v in (("step", r["worst"]), ("rss", g["ratio"])):
                    if v > worst[k, nm][0]:
                        worst[k, nm] = (v, run.id)
    for key, (v, rid) in sorted(worst.items()):
        print(f"largest error / bound of the {key[1]} emulation, {key[0]} bound: {v:.4g} ({rid})")
    # if an emulation needs more than a quarter of a bound, the derivation is wrong -- not the constant
    assert all(v <= S.EMU_LIMIT for v, _ in worst.values()), worst
    rec = {("step", "general"): S.MEASURED_STEP_GENERAL, ("step", "chain"): S.MEASURED_STEP_CHAIN,
           ("rss", "general"): S.MEASURED_RSS_GENERAL, ("rss", "chain"): S.MEASURED_RSS_CHAIN}
    for key, (v, rid) in worst.items():     # the recorded maxima are what the emulations show (to the digits recorded)
        assert 0.98 * rec[key] <= v <= 1.02 * rec[key], (key, v, rec[key], rid)


# mutation -> the runs on which it must be rejected at >= 10 x the bound (both cubic_P30 regimes in every list)
_C30 = ["cubic_P30-benign:nu+phi+sigma", "cubic_P30-stiff:nu+phi+sigma"]
MUTATION_RUNS = {
    "drop_term": _C30 + ["quint_P27-benign:nu+phi+sigma", "cubic_P40-benign:nu+phi+sigma"],
    "drop_lower": _C30 + ["quad_P29-benign:nu+phi+sigma", "cubic_P13-benign:nu+phi+sigma", "wide_5x6-benign:nu+phi+sigma"],
    "stale_delta": _C30 + ["lin_P6-benign:nu+phi+sigma", "mv_P7-benign:nu+phi+sigma"],
    "no_hq": _C30 + ["mv_P64-stiff:nu+phi+sigma", "cubic_P30-benign:nu"],
    "nu_first": _C30 + ["quart_P32-benign:nu+phi+sigma"],
    "m_outer": _C30 + ["quint_P27-stiff:nu+phi+sigma"],
    "f_no_beta": ["cubic_P30-benign:nu+phi+sigma:beta0.37", "quint_P27-stiff:nu+phi+sigma:beta0.37"],
    "last_row": _C30 + ["quad_P29-benign:nu+phi+sigma", "quint_P27-stiff:nu+phi+sigma", "cubic_P13-benign:nu+phi+sigma", "lin_P33-benign:nu+phi+sigma"],
    "late_delta": _C30 + ["cubic_P30-benign:nu", "cubic_P30_K2M1-benign:phi"],
    "lz_next": _C30 + ["step_P10_pen1-benign:nu+phi+sigma"],
}


def test_mutation_table_is_complete():
    assert sorted(MUTATION_RUNS) == sorted(S.MUTATIONS)
    for m, ids in MUTATION_RUNS.items():
        assert all(i in S.RUN_BY_ID for i in ids), m
        if m != "f_no_beta":        # (needs beta != 1: the two regimes of cubic_P30 / quint_P27 at beta = 0.37)
            assert set(_C30) <= set(ids), m


@pytest.mark.parametrize("mut", S.MUTATIONS)
def test_mutation_of_the_emulations_is_rejected(mut):
    """drop_term: H_{a, a_u} delta_u of (the last step, u = 1) dropped; drop_lower: the below-diagonal band entries of that block;
    stale_delta: delta_1 never applied (theta0 used for an updated direction); no_hq: rhs = f r; nu_first: the nu sweep before
    the Phi sweep; m_outer: m outer, j inner in the Phi sweep; f_no_beta: f = 1 / sigma^2 at beta = 0.37; last_row: row P - 1 left at
    theta0 (the lone row of an odd P; on P = 30 the second row of the last pair); late_delta: every delta applied one step late;
    lz_next: L z of direction a + 1 used for a."""
    for rid in MUTATION_RUNS[mut]:
        run = S.RUN_BY_ID[rid]
        inp = S.cpu_inputs(run)
        for nm, emu in _emus(run.case):
            th1, _ = emu(run.case, run.mask, inp, run.MD, mut=mut, beta=run.beta)
            r = _steps(run, inp, th1)
            w = max(r["steps"], key=lambda x: x["ratio"])
            print(f"{mut}, {nm} emulation, {rid}: error / bound {w['ratio']:.3g} at (step {w['s']}, p {w['p']})")
            assert not r["ok"] and w["ratio"] >= 10.0, f"mutation {mut} of the {nm} emulation passes on {rid}: error / bound {w['ratio']:.3g}"
            if mut == "last_row":
                assert w["p"] == run.case.P - 1
            if mut in ("drop_term", "drop_lower"):      # one term of one step: every other step still passes
                assert all(x["ratio"] <= 1.0 for x in r["steps"] if x["s"] != w["s"]) and w["s"] == len(r["steps"]) - 1


@pytest.mark.parametrize("rss_mut", ["drop_direction", "r0_for_r1"])
def test_rss_mutation_is_rejected(rss_mut):
    for rid in _C30 + ["cubic_P40-benign:nu+phi+sigma", "mv_P7-benign:nu+phi+sigma"]:
        run = S.RUN_BY_ID[rid]
        inp = S.cpu_inputs(run)
        th1, rss = S.emulate_general(run.case, run.mask, inp, run.MD, rss_mut=rss_mut)
        assert _steps(run, inp, th1)["ok"]
        g = _rss(run, inp, th1, rss)
        print(f"{rss_mut}, {rid}: {g['msg']}")
        assert g["ratio"] >= 10.0, g["msg"]


def test_frozen_directions_must_be_bit_equal():
    run = S.RUN_BY_ID["cubic_P30-benign:nu"]
    inp = S.cpu_inputs(run)
    th1, _ = S.emulate_general(run.case, run.mask, inp, run.MD)
    assert _steps(run, inp, th1)["ok"]
    th1[1, 3] = np.nextafter(th1[1, 3], np.inf)        # a Phi direction of a nu-only sweep, one unit in the last place
    r = _steps(run, inp, th1)
    assert not r["ok"] and not r["frozen_ok"]


def test_bound_is_small_against_the_step_it_judges():
    """non-vacuity, from the reference alone: max_p bound_p <= 1e-3 max_p |delta_s[p]| for every run and step"""
    worst = (0.0, "")
    for run in S.RUNS:
        for q in range(run.case.nch):
            for s, a, bmax, dmax in S.nonvacuity(run.case, run.mask, S.cpu_inputs(run, q), run.MD):
                assert bmax <= 1e-3 * dmax, f"{run.id}, chain {q}, step {s} (direction {a}): bound {bmax:.3g}, step {dmax:.3g}"
                if bmax / dmax > worst[0]:
                    worst = (bmax / dmax, f"{run.id} step {s}")
    print(f"largest bound / step: {worst[0]:.3g} ({worst[1]})")


def test_every_route_has_its_cases():
    routes = {S.expected_route(c)[:4] for c in S.ALL_CASES}
    assert {("chain", b, False, False) for b in range(1, 6)} <= routes and ("chain", 0, False, False) in routes and ("chain", 0, True, False) in routes
    assert {S.EXPECTED_ROUTE[c.name.split("-")[0]][4] for c in S.ALL_CASES if S.expected_route(c)[0] == "chain"} == {4, 8, 16}
    assert {("general", 0, False, False), ("general", 0, False, True), ("general", 0, True, True)} <= routes
    assert {("diag", 1, True, False), ("diag", 2, True, False), ("diag", 8, True, False), ("diag", 1, False, False)} <= routes
    by = {c.name: c for c in S.ALL_CASES}
    assert by["cubic_P30_K4M5-benign"].A == 24 and by["cubic_P30_K5M4-benign"].A == 25      # 16 lanes per rank: 384 row threads, 400
    assert S.expected_route(by["cubic_P30_K4M5-benign"])[4] == 448
    assert any(c.P % 2 == 1 and S.expected_route(c)[0] == "chain" for c in S.ALL_CASES)


def test_step_order_against_the_oracle():
    """updatePhi then updateNu of the oracle, with the same keyed normals, against the longdouble sweep in the reference's step
    order -- so that sweep_steps does not merely restate the kernels' step_dir"""
    import oracle_lib as O
    run = S.RUN_BY_ID["lin_P6-benign:nu+phi+sigma"]
    c = run.case
    d, st = F.case_data(c), F.case_state(c)
    model = O.Model(d["y"], d["B"], c.K, c.M, Pmat=d["Pmat"])
    ch = O.Chain(model, 2)
    ch.set_slot0(nu=st["nu"], Phi=st["Phi"], chi=st["chi"], Z=st["Z"], pi=st["pi"], alpha3=st["alpha_3"][0], delta=st["delta"],
                 A=st["A"], sigma=st["sigma_sq"][0], tau=st["tau"], gamma=st["gamma"])
    O.updatePhi(model, ch, 0, np.cumprod(st["delta"], axis=1), seed=F.SEED)
    O.updateNu(model, ch, 0, seed=F.SEED)
    got = S.theta_of(c, dict(nu=ch.nu[:, :, 0], Phi=ch.Phi[:, :, :, 0]))
    inp = S.cpu_inputs(run)
    ref = np.asarray(S.reference_sweep(c, U_FULL, inp["theta0"], inp["H"], inp["Cmat"], inp["Lz"], inp["rvec"], inp["hq"], inp["f"]), dtype=np.float64)
    assert np.abs(got - inp["theta0"]).min(axis=1).max() > 0 and np.abs(got - ref).max() <= 1e-9, np.abs(got - ref).max()
    for order in ("nu_first", "m_outer"):       # ... and the check can tell the orders apart
        th1, _ = S.emulate_general(c, U_FULL, inp, mut=order)
        assert np.abs(th1 - got).max() > 1e-6, order


U_FULL = S.U_NU | S.U_PHI
