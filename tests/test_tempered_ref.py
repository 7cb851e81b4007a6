"""CPU checks of tests/tempered_ref.py: the restatement of the tempered-transition block against the oracle (ladder, logA,
decisions), the two float64 emulations of the host arithmetic under the bound of logA and the constant G_LOGA measured from them,
every mutation rejected, and the conditions on the case list: every sweep kernel and the Xi block named, N_t in {1, 2, 3, 4}, an odd
n_obs_total with odd n_i, both outcomes in every model family, no block the reference leaves undecided."""
import numpy as np
import pytest

import curve_update_ref as R
import factor_ref as F
import oracle_lib as O
import scalar_jobs_ref as J
import tempered_ref as T

U, LD = F.U, F.LD
pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 on this platform")


def synthetic_traces():
    """(tag, N_t, ladder as doubles, sig, rss, N): traces of the size the blocks see, and harder ones (sigma^2 over four decades)"""
    rng = np.random.default_rng(2024)
    out = []
    for N_t in (2, 3, 4, 5, 6):
        for k, (lo, hi) in enumerate(((2.5, 4.5), (1e-3, 10.0), (0.5, 2.0))):
            b = float(rng.uniform(0.02, 0.98))
            lad = O.beta_ladder(N_t, b)
            L = 2 * N_t + 1
            sig = np.exp(rng.uniform(np.log(lo), np.log(hi), size=L))
            N = int(rng.integers(140, 500))
            rss = sig * N * rng.uniform(0.7, 1.4, size=L)
            out.append((f"synthetic:Nt{N_t}:{k}", N_t, lad, sig, rss, N))
    return out


def all_traces():
    out = synthetic_traces()
    for t in T.CASES:
        if t.N_t > 1:
            o = T.oracle_block(t)
            out.append((t.id, t.N_t, O.beta_ladder(t.N_t, t.beta_N_t), o["sig"], o["rss"], o["N"]))
    return out


def test_ladder_and_schedule_match_the_oracle():
    for N_t in (1, 2, 3, 4, 5, 7):
        for b in (0.02, 0.3, 0.5, 0.95, 1.0):
            r = T.check_ladder(N_t, b, O.beta_ladder(N_t, b))
            assert not r["fails"], (N_t, b, r["fails"])
    assert float(T.ladder(1, 0.3)[0]) == 0.3      # the only N_t whose last rung is beta_N_t
    assert abs(float(T.ladder(4, 0.5)[3]) - 0.5 ** 0.75) < 1e-15
    assert T.schedule_index(3) == [0, 1, 2, 2, 1, 0] and T.schedule_index(1) == [0, 0] and T.schedule_index(2) == [0, 1, 1, 0]
    lad = O.beta_ladder(3, 0.6)
    assert not T.check_schedule(3, lad, lad[[0, 1, 2, 2, 1, 0]])
    print(f"largest ladder allowance in the list: {max(T.ladder_tol(t.N_t - 1, t.N_t, t.beta_N_t) for t in T.CASES) / U:.3g} u")


def test_emulations_pass_and_g_loga_holds(monkeypatch):
    """both emulations pass the bound on every trace with G_LOGA as it stands; with G_LOGA = 1 the largest error / bound they show is
    what the constant was set from, and 4 x that is the constant"""
    emus = {"host": T.emulate_host, "grouped": T.emulate_grouped}
    for tag, N_t, lad, sig, rss, N in all_traces():
        for nm, fn in emus.items():
            r = T.check_logA(N_t, lad, sig, rss, N, fn(lad, sig, rss, N))
            assert not r["fails"], (tag, nm, r["fails"])
    G = T.G_LOGA
    monkeypatch.setattr(T, "G_LOGA", 1.0)
    worst = {nm: (0.0, "") for nm in emus}
    for tag, N_t, lad, sig, rss, N in all_traces():
        for nm, fn in emus.items():
            w = T.check_logA(N_t, lad, sig, rss, N, fn(lad, sig, rss, N))["worst"]
            if w > worst[nm][0]:
                worst[nm] = (w, tag)
    for nm, (w, where) in worst.items():
        print(f"largest error / (bound at G = 1), logA, {nm:8s}: {w:.3g} ({where})")
        assert w <= 1.02 * T.MEASURED_LOGA[nm], f"{nm}: the emulation now shows {w:.3g}, the constant was set from {T.MEASURED_LOGA}"
    top = max(T.MEASURED_LOGA.values())
    assert 3.95 * top <= G <= 4.1 * top, f"G_LOGA = {G} is not 4 x {T.MEASURED_LOGA}"
    assert all(str(v) in T.__doc__ for v in (*T.MEASURED_LOGA.values(), G)), "the docstring of tempered_ref no longer states the measured figures"


def test_emulations_differ_in_order_only():
    """the two emulations are different arithmetic (they disagree in the last places on some trace) and the host one is the formula of
    the block as written: PZ summed with four running additions per rung"""
    diff = 0
    for tag, N_t, lad, sig, rss, N in all_traces():
        a, b = T.emulate_host(lad, sig, rss, N), T.emulate_grouped(lad, sig, rss, N)
        diff += a != b
    assert diff > 0


def test_restatement_is_pinned_to_the_oracle():
    """logA of the restatement, from the oracle's own sigma^2 and RSS trace, against the oracle's CalculateTTAcceptance; decisions
    equal.  The oracle sums every PZ observation by observation (N additions): the bound of the host arithmetic, which has
    4 (N_t - 1) terms, gets the oracle's own allowance on top (tempered_ref.oracle_allowance has the count)."""
    worst = (0.0, "")
    for t in T.CASES:
        o = T.oracle_block(t)
        assert o["blocks"] == [t.it], (t.id, o["blocks"])
        lad = O.beta_ladder(t.N_t, t.beta_N_t)
        assert not T.check_ladder(t.N_t, t.beta_N_t, lad)["fails"]
        ref, S = T.logA_ref(T.ladder(t.N_t, t.beta_N_t), o["sig"], o["rss"], o["N"])
        if t.N_t == 1:
            assert o["logA"] == 0.0 and float(ref) == 0.0 and o["accepted"], t.id
            continue
        bound = T.logA_bound(t.N_t, S) + T.oracle_allowance(o["N"], *T.abs_halves(T.ladder(t.N_t, t.beta_N_t), o["sig"], o["rss"], o["N"]))
        r = abs(o["logA"] - float(ref)) / bound
        print(f"{t.id:30s} logA {o['logA']:12.6f} restated {float(ref):12.6f} error / bound {r:.3g} (error / host bound alone "
              f"{abs(o['logA'] - float(ref)) / T.logA_bound(t.N_t, S):.3g}); log u {o['log_u']:.6f}, accepted {o['accepted']}")
        worst = max(worst, (r, t.id))
        assert r <= 1.0, (t.id, o["logA"], float(ref), bound)
        assert o["accepted"] == bool(LD(o["log_u"]) < ref), t.id
        d = T.check_decision(o["log_u"], o["logA"], o["accepted"], t.seed, t.it)
        assert not d["fails"], (t.id, d["fails"])
    print(f"largest oracle error / bound: {worst[0]:.3g} ({worst[1]})")


def test_case_list_conditions():
    """routes named, N_t in {1, 2, 3, 4}, odd n_obs_total with odd n_i, both outcomes per family, nothing undecided, bound small"""
    assert {t.kernel for t in T.CASES} == {"chain", "general", "diag"}
    assert any(t.cov and t.case.D == 2 and t.case.cov_adj for t in T.CASES)
    assert {t.N_t for t in T.CASES} == {1, 2, 3, 4}
    assert any(t.base > 0 for t in T.CASES)
    assert all(t.it - t.base + 1 >= 2 for t in T.CASES), "the plain run before the block has at least two iterations"
    assert {t.name for t in T.CASES} == set(T.ROUTED)
    odd = []
    for t in T.CASES:
        c = t.case
        dm = T.dims_of(c)
        ni = [c.P] * c.n if c.kind == "mv" else [len(y) for y in F.case_data(c)["y"]]
        if dm["n_obs_total"] % 2 and any(k % 2 for k in ni):
            odd.append(t.id)
            assert 2 * dm["half_sum"] != dm["n_obs_total"]
    assert any(T.BY_ID[i].family == "functional" for i in odd) and any(T.BY_ID[i].family == "multivariate" for i in odd), odd
    seen = {}
    for t in T.CASES:
        o = T.oracle_block(t)
        assert o["accepted"] == t.accepted, (t.id, o["logA"], o["log_u"])
        if t.N_t == 1:
            continue
        seen.setdefault(t.family, set()).add(o["accepted"])
        _, S = T.logA_ref(T.ladder(t.N_t, t.beta_N_t), o["sig"], o["rss"], o["N"])
        bound = T.logA_bound(t.N_t, S)
        margin = abs(o["logA"] - o["log_u"])
        print(f"{t.id:30s} |logA - log u| {margin:.3g}, bound {bound:.3g}, bound / S {bound / float(S):.3g}, S {float(S):.6g}")
        assert margin > T.UNDECIDED * bound, f"{t.id}: the reference leaves the block undecided: choose another seed or beta_N_t"
        assert bound <= T.LOGA_NONVACUOUS * float(S)
        # one dropped PZ value is far above the bound
        a, b = T.pz_halves(T.ladder(t.N_t, t.beta_N_t)[1], o["sig"][0], o["rss"][0], o["N"])
        assert abs(a - b) >= 1e6 * bound
    assert seen == {f: {True, False} for f in ("functional", "multivariate", "covariates")}, seen
    assert [T.BY_ID[i].accepted for i in T.AFTER_BLOCK] == [True, False]


# ---------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------
def _trace(tid):
    t = T.BY_ID[tid]
    o = T.oracle_block(t)
    return t, o, O.beta_ladder(t.N_t, t.beta_N_t)


@pytest.mark.parametrize("mut", ["pz_half_sum", "mirror_off_by_one", "sign_swapped"])
@pytest.mark.parametrize("tid", ["cubic_P40-benign:Nt3", "mv_P7-benign:Nt4", "cubic_P30-benign:Nt2"])
def test_loga_mutation_is_rejected(mut, tid):
    t, o, lad = _trace(tid)
    wrong = float(T.logA_ref(lad.astype(LD), o["sig"], o["rss"], o["N"], mut, o["half_sum"])[0])
    r = T.check_logA(t.N_t, lad, o["sig"], o["rss"], o["N"], wrong)
    print(f"{mut} on {tid}: error / bound {r['worst']:.3g}")
    assert r["worst"] >= 10.0 and r["fails"]
    assert not T.check_logA(t.N_t, lad, o["sig"], o["rss"], o["N"], T.emulate_host(lad, o["sig"], o["rss"], o["N"]))["fails"]


def test_ladder_mutation_is_rejected():
    for t in T.CASES:
        if t.N_t == 1:
            continue
        wrong = np.asarray(T.ladder(t.N_t, t.beta_N_t, "last_rung_beta"), dtype=np.float64)
        r = T.check_ladder(t.N_t, t.beta_N_t, wrong)
        print(f"last_rung_beta on {t.id}: error / allowance {r['worst']:.3g}")
        assert r["worst"] >= 10.0 and r["fails"]


def test_schedule_mutation_is_rejected():
    for N_t in (2, 3, 4):
        lad = O.beta_ladder(N_t, 0.4)
        assert T.check_schedule(N_t, lad, lad[T.schedule_index(N_t, "temp_ind_early")])
        assert not T.check_schedule(N_t, lad, lad[T.schedule_index(N_t)])


def _sigma_inputs(name, beta, tt):
    import cov_ref as V
    c = (V.BY_NAME if name in V.BY_NAME else R.BY_NAME)[name]
    dims, hyp = T.dims_of(c), dict(J.HYPER_DEFAULTS)
    g = J.gamma_variate(T.UPD_SIGMA, 0, T.sigma_shape(beta, dims, hyp), F.SEED, 0, 2, tt=tt)[0][0]
    rss = 3.1 * dims["n_obs_total"]
    return c, dims, hyp, g, rss


@pytest.mark.parametrize("name", ["cubic_P40-benign", "mv_P7-benign"])
def test_sigma_mutations_are_rejected(name):
    """the shape with half_sum (seen at the "gstd" entry, at beta = 1 too: odd n_i), the rate without beta (seen at sigma^2, beta = 0.37),
    a tt_step 0 key (seen at the "gstd" entry)"""
    for beta, tt in T.SINGLE_SWEEPS:
        c, dims, hyp, g, rss = _sigma_inputs(name, beta, tt)
        s2 = float(T.sigma_ref(beta, rss, g, hyp))
        ok = T.check_sigma(c, beta, tt, rss, g, s2, dims, hyp, F.SEED, 2)
        assert not ok["fails"] and ok["worst"] <= 1e-3, ok
        g_bad = J.gamma_variate(T.UPD_SIGMA, 0, T.sigma_shape(beta, dims, hyp, "shape_half_sum"), F.SEED, 0, 2, tt=tt)[0][0]
        r = T.check_sigma(c, beta, tt, rss, g_bad, float(T.sigma_ref(beta, rss, g_bad, hyp)), dims, hyp, F.SEED, 2)
        print(f"shape_half_sum on {name}, beta {beta}: \"gstd\" error / allowance {r['worst_g']:.3g}")
        assert r["worst_g"] >= 10.0 and r["fails"]
        g_tt0 = J.gamma_variate(T.UPD_SIGMA, 0, T.sigma_shape(beta, dims, hyp), F.SEED, 0, 2, tt=0)[0][0]
        r = T.check_sigma(c, beta, tt, rss, g_tt0, float(T.sigma_ref(beta, rss, g_tt0, hyp)), dims, hyp, F.SEED, 2)
        print(f"tt0_key_in_sweep on {name}, beta {beta}: \"gstd\" error / allowance {r['worst_g']:.3g}")
        assert r["worst_g"] >= 10.0 and r["fails"]
        if beta != 1.0:
            r = T.check_sigma(c, beta, tt, rss, g, float(T.sigma_ref(beta, rss, g, hyp, "rate_half_rss")), dims, hyp, F.SEED, 2)
            print(f"rate_half_rss on {name}, beta {beta}: sigma^2 error / tolerance {r['worst']:.3g}")
            assert r["worst"] >= 10.0 and r["fails"]


def test_key_mutations_are_rejected():
    """a tt_step l key in the iteration after the block: the chi normals and log_uu of (iter + 1, tt_step l) fail the references at
    (iter + 1, tt_step 0); a tt_step 0 key in a tempered sweep fails them at tt_step l"""
    c = R.BY_NAME["cubic_P30-benign"]
    it, l = 3, 4
    for tt_dev, tt_ref in ((l, 0), (0, l)):
        zn = O.fill(1, c.n * c.M, seed=R.SEED, chain=0, it=it, upd=R.UPD_CHI, tt=tt_dev).reshape(c.n, c.M).T.copy()
        assert R.check_chi_norm(c, zn.ravel(), 0, it, tt=tt_ref)
        assert not R.check_chi_norm(c, zn.ravel(), 0, it, tt=tt_dev)
        zrec = np.zeros((len(R.ZREC_FIELDS) + c.K, c.n))
        zrec[R.ZREC_FIELDS.index("log_uu")] = np.log(O.fill(0, c.n, seed=R.SEED, chain=0, it=it, upd=R.UPD_Z_ACC, tt=tt_dev))
        assert R.check_log_uu(c, zrec, 0, it, tt=tt_ref)
        assert not R.check_log_uu(c, zrec, 0, it, tt=tt_dev)
    assert float(T.log_u_ref(F.SEED, it, tt=l)) != float(T.log_u_ref(F.SEED, it))


@pytest.mark.parametrize("name", ["cubic_P30-benign", "mv_P7-benign"])
def test_factor_normals_with_a_tt0_key_are_rejected(name):
    """L_a z_a formed from the nu / Phi normals of (iteration, tt_step 0) fails factor_ref.check_direction against the normals of
    (iteration, tt_step l) at f = beta / sigma^2, in every direction; formed from those of tt_step l it passes"""
    c = R.BY_NAME[name]
    st = R.case_state(c)
    beta, tt = T.SINGLE_SWEEPS[0]
    it = 2
    precs = F.precisions(c, F.hbands_from_H(c, F.host_H(c, st)), T.tempered_state(st, beta))
    z_ref, z_bad = F.normals(c, 0, it, tt), F.normals(c, 0, it, 0)
    for a in range(c.A):
        if c.diag:
            d = np.diagonal(precs[a])
            Cm, L = np.diag(np.asarray(1 / d, dtype=np.float64)), np.diag(1 / np.sqrt(d))
        else:
            Rf = F.inverse_ld(precs[a])
            Cm, L = np.asarray(Rf.C, dtype=np.float64), Rf.L
            Cm = (Cm + Cm.T) / 2
        good = F.check_direction(c, a, precs[a], Cm, np.asarray(L @ z_ref[a].astype(LD), dtype=np.float64), z_ref[a])
        bad = F.check_direction(c, a, precs[a], Cm, np.asarray(L @ z_bad[a].astype(LD), dtype=np.float64), z_ref[a])
        assert good["ok"], good["msg"]
        assert not bad["ok"] and bad["rL"] >= 10.0 and bad["rC"] <= 1.0, bad["msg"]
    print(f"tt0_key_in_sweep on {name}: Lz error / bound {bad['rL']:.3g} (last direction)")


def test_handover_mutations_are_rejected():
    rng = np.random.default_rng(3)
    names = T.STATE_NAMES + T.SCALAR_NAMES
    snap = {nm: rng.standard_normal(6) for nm in names}
    replay = {nm: rng.standard_normal(6) for nm in names}
    # accepted: the replayed state with the gamma of before the block
    good = dict(replay, gamma=snap["gamma"])
    assert not T.check_handover(True, good, snap, replay, {}, names)
    assert T.check_handover(True, replay, snap, replay, {}, names) == ["gamma after the accepted block is not bit-equal to the snapshot of before the block"]
    # rejected: the snapshot, and the slot rewritten from it
    assert not T.check_handover(False, snap, snap, replay, dict(snap), names)
    bad = T.check_handover(False, snap, snap, replay, dict(replay), names)      # the slot still holds the last tempered sweep
    assert len(bad) == len(names) and all("chain slot" in m for m in bad)
    assert T.check_handover(False, replay, snap, replay, dict(replay), names)


def test_new_fill_arguments_default_to_the_plain_keys():
    c = R.BY_NAME["cubic_P30-benign"]
    assert np.array_equal(F.normals(c), F.normals(c, 0, 0, 0)) and not np.array_equal(F.normals(c), F.normals(c, 0, 0, 1))
    hyp, dims = dict(J.HYPER_DEFAULTS), T.dims_of(c)
    A = R.case_state(c)["A"]
    v0, v1 = J.variates(c, A, hyp, dims), J.variates(c, A, hyp, dims, tt=2)
    lay = J.gstd_layout(c)
    assert np.array_equal(v0["g"], J.variates(c, A, hyp, dims, tt=0)["g"])
    for part in ("gamma", "delta", "tau", "aprop", "aunif", "sigma"):
        assert not np.array_equal(v0["g"][slice(*lay[part])], v1["g"][slice(*lay[part])]), part
