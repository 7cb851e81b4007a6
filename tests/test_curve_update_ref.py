"""CPU checks of tests/curve_update_ref.py: both float64 emulations of the per-curve updates pass every bound of every case
within a quarter of it, the measured constants have not grown, every bound is small against the change it judges, each
mutation of the kernel-order emulation is rejected at >= 10 x the bound on a named case, the route table covers what the
issue lists, and the restated chi update agrees with the oracle's updateChi under the same keyed normals."""
import numpy as np
import pytest

import curve_update_ref as R
import factor_ref as F

pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 on this platform")

_memo = {}


def _normals(c, q=0):
    rng = np.random.default_rng(1000 + q + len(c.name))
    return rng.standard_normal((c.n, c.M))


def emulated(name, variant, beta=1.0):
    """both updates of case `name` by emulation `variant`, checked: dict(chi, rss, z) of check results"""
    key = (name, variant, beta)
    if key in _memo:
        return _memo[key]
    c = R.BY_NAME[name]
    rec, st, X = R.host_rec(c), R.case_state(c), R.case_X(c)
    zn = _normals(c)
    chi1, part, cf, gf = R.emulate_chi(c, rec, st, zn, beta, X, variant, full=True)
    out = dict(chi=R.check_chi(c, rec, st, chi1, zn, beta, X), rss=R.check_rss(c, rec, st, chi1, part, X))
    if c.D:
        g = R.check_cfull(c, rec, st, chi1, X, cf, gf)
        out["cf"] = dict(worst=g["worst"], fails=g["fails"])
        out["gf"] = dict(worst=g["worst_g"], fails=[])
    prop = R.synthetic_proposal(c, st)
    acc, Z1, logz = R.emulate_z(c, rec, st, prop, beta, X, variant=variant)
    out["z"] = R.check_z(c, rec, st, R.pack_zrec(c, prop, acc), Z1, beta, X, logz_part=logz)
    if c.D:
        stil, yyp = R.emulate_stil(c, rec, st, Z1, X, variant)
        out["stil"] = R.check_stil(c, rec, st, Z1, X, stil, yyp)
    _memo[key] = out
    return out


def test_emulations_pass_and_constants_hold():
    worst = {k: {"kernel": (0.0, ""), "plain": (0.0, "")} for k in ("chi", "z", "rss", "stil", "yyp", "cf", "gf")}
    vac = {"chi": (0.0, ""), "z": (0.0, "")}
    fails = []
    for c in R.CASES:
        for variant in ("kernel", "plain"):
            for beta in ((1.0, 0.37) if c.name == R.BETA_CASE else (1.0,)):
                out = emulated(c.name, variant, beta)
                if "stil" in out:
                    out = dict(out, yyp=dict(worst=out["stil"]["worst_yyp"], fails=[]))
                for k in out:
                    fails += out[k]["fails"]
                    if out[k]["worst"] > worst[k][variant][0]:
                        worst[k][variant] = (out[k]["worst"], c.name)
                for k in ("chi", "z"):
                    if out[k]["vacuous"] > vac[k][0]:
                        vac[k] = (out[k]["vacuous"], c.name)
    G = {"chi": R.G_CHI, "z": R.G_ACC, "rss": R.G_RSS, "stil": R.G_STIL, "yyp": R.G_YYP, "cf": R.G_CF, "gf": R.G_GF}
    M = {"chi": R.MEASURED_CHI, "z": R.MEASURED_ACC, "rss": R.MEASURED_RSS, "stil": R.MEASURED_STIL, "yyp": R.MEASURED_YYP,
         "cf": R.MEASURED_CF, "gf": R.MEASURED_GF}
    for k in worst:
        for variant, (w, nm) in worst[k].items():
            print(f"{k}: {variant}: largest error / bound {w:.3g} = {w * G[k]:.3g} at G = 1 ({nm})")
            assert w <= R.EMU_LIMIT, (k, variant, w, nm)
            assert w * G[k] <= M[k][variant] * 1.0001, f"{k}, {variant}: measured {w * G[k]:.4g} has grown past {M[k][variant]}"
        assert G[k] >= 4 * max(M[k].values()) * 0.999, k
    assert not fails, "\n".join(fails[:10])
    for k, (v, nm) in vac.items():
        print(f"{k}: largest bound / judged change {v:.3g} ({nm})")
        assert v <= R.NONVACUOUS, f"{k}: a bound is {v:.3g} of the change it judges on {nm}"


CHI_MUT_CASE = {"stale_dl": "cubic_P30_K3M7-benign", "small_at_9": "cubic_P30_K7M9-benign", "sqrtW_as_W": "cubic_P30-benign",
                "rss_no_cross": "cubic_P30-benign", "idle_rss": "cubic_P40-benign"}
Z_MUT_CASE = {"q_transposed": "cubic_P30-benign", "half_dot_dropped": "cubic_P30-benign", "a_vs_resid": "cubic_P30-benign",
              "no_beta": "cubic_P30-benign", "lp_swapped": "cubic_P30-benign", "inv_s2": "cubic_P30-benign",
              "pad_nonzero": "cubic_P30_K3M7-benign"}


@pytest.mark.parametrize("mut", R.CHI_MUTATIONS)
def test_chi_mutations_are_rejected(mut):
    c = R.BY_NAME[CHI_MUT_CASE[mut]]
    rec, st, zn = R.host_rec(c), R.case_state(c), _normals(c)
    chi1, part = R.emulate_chi(c, rec, st, zn, 1.0, None, "kernel", mut=mut)
    got = R.check_rss(c, rec, st, chi1, part)["worst"] if mut in ("rss_no_cross", "idle_rss") else R.check_chi(c, rec, st, chi1, zn, 1.0)["worst"]
    print(f"{mut} on {c.name}: error / bound {got:.3g}")
    assert got >= 10.0, (mut, got)


@pytest.mark.parametrize("mut", R.Z_MUTATIONS)
def test_z_mutations_are_rejected(mut):
    c = R.BY_NAME[Z_MUT_CASE[mut]]
    beta = 0.37 if mut == "no_beta" else 1.0
    rec, st = R.host_rec(c), R.case_state(c)
    prop = R.synthetic_proposal(c, st)
    acc, Z1, logz = R.emulate_z(c, rec, st, prop, beta, mut=mut)
    got = R.check_z(c, rec, st, R.pack_zrec(c, prop, acc), Z1, beta)["worst"]
    print(f"{mut} on {c.name}: error / bound {got:.3g}")
    assert got >= 10.0, (mut, got)


def test_covariate_offset_mutation_is_rejected():
    """the covariate part of u_k left out of o_i (the chi-weighted xi terms): stil and yyp_part both show it"""
    c = R.BY_NAME["cubic_P30_D5-benign"]
    rec, st, X = R.host_rec(c), R.case_state(c), R.case_X(c)
    stil, yyp = R.emulate_stil(c, rec, st, st["Z"], X, mut="cov_left_out")
    got = R.check_stil(c, rec, st, st["Z"], X, stil, yyp)
    print(f"cov_left_out on {c.name}: stil error / bound {got['worst']:.3g}, yyp_part {got['worst_yyp']:.3g}")
    assert got["worst"] >= 10.0 and got["worst_yyp"] >= 10.0


def test_cfull_mutation_is_rejected():
    """the last step's dl left out of c_i and g_i = G_i c_i; and the residual-only pass (chi unchanged) gives c0, G c0"""
    c = R.BY_NAME["cubic_P30_D5-benign"]
    rec, st, X, zn = R.host_rec(c), R.case_state(c), R.case_X(c), _normals(c)
    chi1, _, cf, gf = R.emulate_chi(c, rec, st, zn, 1.0, X, "kernel", mut="cfull_last_step", full=True)
    got = R.check_cfull(c, rec, st, chi1, X, cf, gf)
    print(f"cfull_last_step on {c.name}: cfull error / bound {got['worst']:.3g}, gfull {got['worst_g']:.3g}")
    assert got["worst"] >= 10.0 and got["worst_g"] >= 10.0
    _, _, cf, gf = R.emulate_chi(c, rec, st, zn, 1.0, X, "kernel", full=True)
    assert not R.check_cfull(c, rec, st, st["chi"], X, cf, gf)["ok"]      # the updated c_i is not c0


def test_proposal_tolerances_have_not_grown():
    """MEASURED_PROP: the oracle's float64 arithmetic against the longdouble restatement of the proposal, over every case and chain"""
    worst = dict(Znew=(0.0, ""), lpn=(0.0, ""), lpo=(0.0, ""))
    for c in R.CASES:
        for q in range(c.nch):
            r = R.measure_proposal(c, q)
            for k in worst:
                if r[k] > worst[k][0]:
                    worst[k] = (r[k], c.name)
    for k, (v, nm) in worst.items():
        print(f"{k}: oracle arithmetic against longdouble {v:.3g} u ({nm})")
        assert v <= R.MEASURED_PROP[k] * 1.0001, (k, v, nm)
    # the check itself: a float64 evaluation passes, a neighbouring variate index or a wrong shape does not
    c = R.BY_NAME["cubic_P30-benign"]
    st = R.case_state(c)
    gam = R.oracle_gammas(c, st["Z"], 10000.0, 0, 0)
    prop = R.synthetic_proposal(c, st)
    for i in range(c.n):
        f = R.proposal_fields(st["Z"][i], gam[i], 10000.0, np.float64)
        prop["Znew"][i], prop["lpn"][i], prop["lpo"][i] = f["Znew"], f["lpn"], f["lpo"]
    zrec = R.pack_zrec(c, prop, np.zeros(c.n))
    got = R.check_proposal(c, st["Z"], zrec, 10000.0, 0, 0)
    assert not got["fails"] and max(got["worst"].values()) <= 0.2501, got
    assert R.check_proposal(c, st["Z"], zrec, 10000.0, 0, 1)["fails"] and R.check_proposal(c, st["Z"], zrec, 10000.0, 1, 0)["fails"]
    assert R.check_proposal(c, st["Z"], zrec, 9999.0, 0, 0)["fails"]
    bad = dict(prop, lpn=prop["lpo"], lpo=prop["lpn"])
    assert R.check_proposal(c, st["Z"], R.pack_zrec(c, bad, np.zeros(c.n)), 10000.0, 0, 0)["fails"]


def test_z_restatement_agrees_with_the_oracle():
    """reference_z (Gram form, longdouble, the oracle's keyed gamma variates and uniform) against oracle_lib.updateZ_PM
    (UpdateMixedMembership.h on the observations): the same decisions and Z to 1e-9, also in the state with exact zeros"""
    import oracle_lib as O
    for name in ("cubic_P30-benign", "cubic_P30_K3M7-benign", "cubic_P30_zero-benign"):
        c = R.BY_NAME[name]
        d, st = F.case_data(c), R.case_state(c)
        model = O.Model(d["y"], d["B"], c.K, c.M)
        ch = O.Chain(model, 2)
        ch.set_slot0(nu=st["nu"], Phi=st["Phi"], chi=st["chi"], Z=st["Z"], sigma=float(st["sigma_sq"][0]), pi=st["pi"],
                     alpha3=float(st["alpha_3"][0]))
        O.updateZ_PM(model, ch, 0, 10000.0, beta_i=1.0, seed=R.SEED, chain_id=0)
        ref, acc = R.reference_z(c, R.host_rec(c), st, 1.0, 10000.0, 0, 0)
        got = ch.Z[..., 0]
        moved = (np.abs(got - st["Z"]).max(axis=1) > 0)
        assert moved.any() and (np.abs(ref - st["Z"]).max(axis=1) > 0).tolist() == moved.tolist(), name
        assert np.abs(got - ref).max() <= 1e-9, (name, np.abs(got - ref).max())


def test_decision_rules_are_enforced():
    """a flipped decision, a forced curve that kept Z_old, a wrong block sum of log Z: each is reported"""
    c = R.BY_NAME["cubic_P30_zero-benign"]
    rec, st = R.host_rec(c), R.case_state(c)
    assert ((st["Z"] == 0).sum(axis=1) == 1).sum() == 7
    prop = R.synthetic_proposal(c, st)
    acc, Z1, logz = R.emulate_z(c, rec, st, prop, 1.0)
    ok = R.check_z(c, rec, st, R.pack_zrec(c, prop, acc), Z1, 1.0, logz_part=logz)
    assert ok["ok"] and ok["forced"] == 7, ok["fails"]
    bad = Z1.copy()
    bad[0] = st["Z"][0]                                  # curve 0 has a zero: it must take the proposal
    assert not R.check_z(c, rec, st, R.pack_zrec(c, prop, acc), bad, 1.0)["ok"]
    i = 1
    flipped = Z1.copy()
    flipped[i] = st["Z"][i] if np.array_equal(Z1[i], prop["Znew"][i]) else prop["Znew"][i]
    assert not R.check_z(c, rec, st, R.pack_zrec(c, prop, acc), flipped, 1.0)["ok"]
    lz = logz.copy()
    lz[c.K + 1] *= 1.0 + 1e-12
    assert R.check_logz(c, Z1, lz)
    # the prior terms: right with the state's pi / alpha_3, reported with another iteration's
    zrec = R.pack_zrec(c, prop, acc)
    assert not R.check_prior_terms(c, st["Z"], zrec, st["pi"], st["alpha_3"])
    assert R.check_prior_terms(c, st["Z"], zrec, st["pi"] * (1 + 1e-9), st["alpha_3"])
    assert R.check_prior_terms(c, st["Z"], zrec, st["pi"], st["alpha_3"] + 1e-8)


def test_cases_cover_the_listed_routes():
    seen_z, seen_chi = set(), set()
    for c in R.CASES:
        for exact in (True, False):
            for kind in ("chi", "z", "lean", "fused"):
                r = R.expected_route(c, kind, exact)
                seen_z.add((r["z"]["form"], r["z"]["BW"], r["z"]["LPC"], r["z"]["COV"], r["z"]["KT"], r["z"]["KEX"]))
                seen_chi.add((r["chi"]["BW"], r["chi"]["LPC"], r["chi"]["COV"], r["chi"]["SMALL"], r["chi"]["KX"], r["chi"]["MX"]))
    for bw in (0, 1, 2, 3, 4, 5, 15, 31):
        for lpc in (32, 64):
            assert any(z[1] == bw and z[2] == lpc and z[0] == "standalone" for z in seen_z), (bw, lpc)
            assert any(x[0] == bw and x[1] == lpc for x in seen_chi), (bw, lpc)
    for K in (2, 3, 4):
        for M in range(1, 9):
            assert (3, 32, False, True, K, M) in seen_chi and (3, 32, False, True, 0, 0) in seen_chi
    for bw, lpc, cov in R.CHI_EXACT_COMBOS:
        for K in (2, 3, 4):
            for M in range(1, 9):
                assert (bw, lpc, cov, True, K, M) in seen_chi, (bw, lpc, cov, K, M)
    assert {c.K for c in R.CASES if c.LPC == 32} >= {2, 4, 5, 7, 8} and {c.K for c in R.CASES if c.LPC == 64} >= {6, 7, 8}
    assert {c.M for c in R.CASES} >= {1, 7, 8, 9, 15, 16}
    assert any(c.K * (c.M + 1) * c.P > 1024 for c in R.CASES)
    assert {c.D for c in R.CASES} >= {0, 1, 5, 8}
    assert {f for f, *_ in seen_z} == {None, "standalone", "lean", "fused"}
    assert all(c.n == 21 and c.n % c.GPB for c in R.CASES)


def test_chi_restatement_agrees_with_the_oracle():
    """the Gram-form recursion of reference_chi against oracle_lib.updateChi (UpdateChi.h on the observations) under the same
    keyed normals: 1e-9 relative to the step, the step order (m ascending, later steps see earlier ones) included"""
    import oracle_lib as O
    for name in ("cubic_P30-benign", "cubic_P30_K3M7-benign"):
        c = R.BY_NAME[name]
        d, st = F.case_data(c), R.case_state(c)
        model = O.Model(d["y"], d["B"], c.K, c.M)
        ch = O.Chain(model, 2)
        ch.set_slot0(nu=st["nu"], Phi=st["Phi"], chi=st["chi"], Z=st["Z"], sigma=float(st["sigma_sq"][0]))
        O.updateChi(model, ch, 0, beta_i=1.0, seed=R.SEED, chain_id=0)
        zn = O.fill(1, c.n * c.M, seed=R.SEED, chain=0, it=0, upd=R.UPD_CHI).reshape(c.n, c.M)
        ref = np.asarray(R.reference_chi(c, R.host_rec(c), st, zn, 1.0), dtype=np.float64)
        got = ch.chi[..., 0]
        scale = np.abs(ref - st["chi"]).max()
        assert np.abs(got - ref).max() <= 1e-9 * scale, (name, np.abs(got - ref).max(), scale)
        # a reversed step order is not the oracle's
        rev = dict(st, chi=st["chi"][:, ::-1], Phi=st["Phi"][:, :, ::-1])
        other = np.asarray(R.reference_chi(c, R.host_rec(c), rev, zn[:, ::-1], 1.0), dtype=np.float64)[:, ::-1]
        assert np.abs(got - other).max() > 1e-6 * scale
