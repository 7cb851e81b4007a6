"""The reference of tests/test_gpu_factor.py checked without a device: inverse_ld against 50-digit arithmetic, the float64
emulation of k_factor's order of operations against both bounds on every case (the constants G_C, G_L, G_J are 4 x what it
shows), every mutation of the emulation rejected on a named case, and the regime guards (kappa_s ranges, the distance of every
direction from the 1e-12 pivot decision) asserted from the reference alone."""
import numpy as np
import pytest

import factor_ref as F

pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is no wider than double on this platform")

_cache = {}


def case_inputs(c):
    """per chain: (state, band rows of H_aa from the host restatement, z, [Prec_a], [reference_a])"""
    if c.name not in _cache:
        out = []
        for q in range(c.nch):
            st = F.case_state(c, q)
            hb = F.hbands_from_H(c, F.host_H(c, st))
            precs = F.precisions(c, hb, st)
            out.append((st, hb, F.normals(c, q), precs, [F.reference(c, a, precs[a]) for a in range(c.A)]))
        _cache[c.name] = out
    return _cache[c.name]


def run_emulation(c, mut=None):
    """check_direction's result for every (chain, direction) of case c under mutation `mut`"""
    res = []
    for st, hb, z, precs, refs in case_inputs(c):
        for a in range(c.A):
            Ch, Lzh = F.emulate_direction(c, hb[a], st, a, z[a], mut=mut)
            res.append(F.check_direction(c, a, precs[a], Ch, Lzh, z[a], R=refs[a]))
    return res


def test_keyed_normals_follow_k_factor_index_layout():
    # element i of the oracle's fill is the variate of counter index i whatever the count, and the two updates' streams differ:
    # z of nu_j is fill(UPD_NU)[j P ...], z of Phi_jm is fill(UPD_PHI)[(j M + m) P ...]  (oracle/updates.c, k_factor)
    import oracle_lib as O
    c = F.BY_NAME["cubic_P30-benign"]
    long = O.fill(1, c.K * c.M * c.P, seed=F.SEED, chain=0, it=0, upd=F.UPD_PHI)
    assert np.array_equal(long[:7], O.fill(1, 7, seed=F.SEED, chain=0, it=0, upd=F.UPD_PHI))
    z = F.normals(c)
    assert np.array_equal(z[1 * c.MD + 2], long[(1 * c.M + 1) * c.P:(1 * c.M + 2) * c.P])
    assert np.array_equal(z[2 * c.MD], O.fill(1, c.K * c.P, seed=F.SEED, chain=0, it=0, upd=F.UPD_NU)[2 * c.P:])
    assert not np.array_equal(z[0], z[1]) and np.isfinite(z).all()


def _to_mp(mp, x):
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - F.LD(hi)))       # a longdouble is the exact sum of two doubles


@pytest.mark.parametrize("name", ["lin_P6-benign", "cubic_P30-stiff", "quint_P27-stiff", "wide_5x6-stiff", "quad_P64-stiff"])
def test_inverse_ld_against_50_digits(name):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    c = F.BY_NAME[name]
    st, hb, z, precs, refs = case_inputs(c)[0]
    a = int(np.argmax([r.kappa_s for r in refs]))         # the stiffest direction of the case
    R, P = refs[a], c.P
    A = mpmath.matrix(P, P)
    for i in range(P):
        for k in range(P):
            A[i, k] = _to_mp(mp, precs[a][i, k])
    C = A ** -1
    L = mpmath.cholesky((C + C.T) / 2)
    sd = [mpmath.sqrt(A[i, i]) for i in range(P)]
    dC = np.array([[float((_to_mp(mp, R.C[i, k]) - C[i, k]) * sd[i] * sd[k]) for k in range(P)] for i in range(P)])
    dL = np.array([[float((_to_mp(mp, R.L[i, k]) - L[i, k]) * sd[i]) for k in range(P)] for i in range(P)])
    nC = np.linalg.norm(np.array([[float(C[i, k] * sd[i] * sd[k]) for k in range(P)] for i in range(P)]), 2)
    nL = np.linalg.norm(np.array([[float(L[i, k] * sd[i]) for k in range(P)] for i in range(P)]), 2)
    eC, eL = np.linalg.norm(dC, 2) / nC, np.linalg.norm(dL, 2) / nL
    print(f"{name} direction {a}: kappa_s {R.kappa_s:.3g}, reference error C {eC:.3g}, L {eL:.3g}")
    # the docstring's claim: about kappa_s 2^-64, i.e. 2^-11 / P of the device's bound (a factor P of slack on the claim)
    lim = P * R.kappa_s * 2.0 ** -64
    assert eC <= lim and eL <= lim, (eC, eL, lim)
    assert lim <= 2.0 ** -9 * F.bound(P, R.kappa_s, min(F.G_C, F.G_L))


def test_emulation_passes_both_bounds_and_sets_the_constants():
    mC = mL = mJ = 0.0
    for c in F.CASES:
        for r in run_emulation(c):
            assert r["ok"], r["msg"]
            if r["route"] == "chol":
                n = c.P * F.U * r["kappa"]
                mC, mL = max(mC, r["raw"][0] / n), max(mL, r["raw"][1] / n)
            elif r["route"] == "pinv":
                n = c.P * F.U * r["kappa"]
                mJ = max(mJ, r["raw"][0] / n, r["raw"][1] / n)
    print(f"largest err / (P 2^-53 kappa): C {mC:.4g}, Lz {mL:.4g}, pseudo-inverse {mJ:.4g}")
    # the recorded maxima are what the emulation shows (to the digits recorded) and the constants are 4 x them, rounded up
    for got, rec, g in ((mC, F.MEASURED_C, F.G_C), (mL, F.MEASURED_L, F.G_L), (mJ, F.MEASURED_J, F.G_J)):
        assert 0.98 * rec <= got <= 1.005 * rec, (got, rec)
        assert 4 * rec <= g <= 4.2 * rec, (rec, g)


# mutation -> (cases on which it must be rejected, cases on which C must still pass)
MUTATIONS = {
    "recip": (["mv_P7-benign", "mv_P64-stiff", "lin_P6-benign", "cubic_P30-benign"], []),
    "drop_prior_edge": (["cubic_P30-benign", "cubic_P30-stiff", "mid_5x5-benign", "wide_7x7-stiff"], []),
    "tilde_tau_short": (["cubic_P30-benign", "quad_P64-stiff", "mv_P7-benign"], []),
    "h_shift": (["lin_P6-benign", "cubic_P30-benign", "quint_P47-stiff", "wide_5x6-benign"], []),
    "uinv_z": (["lin_P6-benign", "cubic_P30-benign", "quart_P32-stiff", "mid_6x6-benign", "wide_7x7-benign"], []),
    "forward": (["lin_P6-benign", "cubic_P30-benign", "quart_P32-stiff", "wide_7x7-benign"],
                ["lin_P6-benign", "cubic_P30-benign", "quart_P32-stiff", "wide_7x7-benign"]),
    "kend": (["lin_P33-benign", "quad_P29-benign", "cubic_P30-benign", "quart_P50-stiff", "quint_P27-benign", "quint_P47-benign",
              "mid_5x5-benign", "wide_5x6-stiff", "wide_7x7-benign"], []),
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_of_the_emulation_is_rejected(mut):
    """recip: a relative error of 1e-13 in every pivot reciprocal (and inverse square root); drop_prior_edge: the prior's
    outermost band entry of one row; tilde_tau_short: one delta too few; h_shift: H's band rows shifted by one; uinv_z: U^-1 z in
    place of U^-T z; forward: first-row-down Cholesky (the same C, another factor); kend: the X'X sum truncated to P & ~3 (only
    P % 4 != 0 can notice)."""
    must_fail, c_must_pass = MUTATIONS[mut]
    for name in must_fail:
        res = run_emulation(F.BY_NAME[name], mut)
        assert any(not r["ok"] for r in res), f"mutation {mut} passes every bound on case {name}"
    for name in c_must_pass:
        assert all(r["rC"] <= 1.0 for r in run_emulation(F.BY_NAME[name], mut)), f"{mut}: C changed on {name}"
    if mut == "kend":     # ... and P % 4 == 0 cannot
        for name in ["quad_P64-benign", "quart_P32-benign", "cubic_P40-stiff"]:
            assert all(r["ok"] for r in run_emulation(F.BY_NAME[name], mut)), name
    if mut == "forward":  # ... where it is Lz that fails
        assert any(r["rL"] > 1.0 for r in run_emulation(F.BY_NAME["cubic_P30-benign"], mut))


def test_every_instantiation_has_its_cases():
    inst = {(c.PP, c.BW) for c in F.CASES}
    for PP in (32, 64):
        assert {(PP, b) for b in (0, 1, 2, 3, 4, 5, F.BWMID, F.BWWIDE)} <= inst
        for reg in ("benign", "stiff"):
            assert {c.BW for c in F.CASES if c.PP == PP and c.regime == reg and c.special is None} >= {0, 1, 2, 3, 4, 5, F.BWMID, F.BWWIDE}
    Ps = {c.P for c in F.CASES if c.kind == "spline"}
    assert {32, 33, 64, 6} <= Ps and any(p % 4 == 1 for p in Ps) and any(p % 4 == 2 for p in Ps)
    assert all(c.n == 24 and c.K <= 3 and c.M <= 2 and c.A <= 9 for c in F.CASES)
    assert {c.P for c in F.CASES if c.kind == "mv"} == {7, 64}


def test_regime_guards():
    lo_b = lo_s = np.inf
    hi_b = hi_s = 0.0
    for c in F.CASES:
        for st, hb, z, precs, refs in case_inputs(c):
            if c.diag:
                continue
            pinv = [a for a in range(c.A) if F.is_pinv_direction(c, a)]
            chol = [a for a in range(c.A) if a not in pinv]
            for a in chol:
                assert refs[a].ok and refs[a].rho >= 1e-9, (c.name, a, refs[a].rho)       # a factor 1000 from the 1e-12 decision
            for a in pinv:
                assert (st["Z"][:, a // c.MD] == 0.0).all() and (hb[a] == 0.0).all(), (c.name, a)    # structurally singular
                assert refs[a].n_null == 1
            ks = [refs[a].kappa_s for a in chol]
            if c.special is None and c.regime == "benign":
                assert max(ks) <= 1e4, (c.name, max(ks))
                lo_b, hi_b = min(lo_b, min(ks)), max(hi_b, max(ks))
            if c.regime == "stiff":
                assert 1e6 <= max(ks) <= 1e10, (c.name, max(ks))                          # the bound stays below 1e-4
                lo_s, hi_s = min(lo_s, max(ks)), max(hi_s, max(ks))
            if c.special == "empty":
                assert len(pinv) == 1
            if c.special == "prior":      # H_aa of the weak cluster is ~1e-8 of the others
                w, o = c.weak * c.MD, (1 - c.weak) * c.MD
                assert np.abs(hb[w]).max() < 1e-6 * np.abs(hb[o]).max()
    print(f"benign kappa_s in [{lo_b:.3g}, {hi_b:.3g}]; largest kappa_s of the stiff cases in [{lo_s:.3g}, {hi_s:.3g}]")
