"""CPU tests of tests/stats_ref.py: the longdouble basis agrees with scipy's design matrix and with the oracle's basis, the
partition of unity holds, both float64 emulations of the record builder pass every exact check and every bound on every case (and
the constants G_B, G_SUM are still 4 x what they show), every mutation of the emulation is rejected by the check written for it,
and the case list stays small."""
import numpy as np
import pytest

import factor_ref as F
import stats_ref as S

pytestmark = pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 here")

SPLINES = [c for c in S.CASES if c.kind == "spline"]
EPS_LD = float(np.finfo(np.longdouble).eps)


@pytest.mark.parametrize("name", [c.name for c in SPLINES if c.knots != "dup" and not c.n])
def test_longdouble_basis_against_scipy_and_the_oracle(name):
    """to float64 rounding: 8 deg u relative (both are float64 triangles of their own order) + u absolute"""
    si = pytest.importorskip("scipy.interpolate")
    import oracle_lib as O
    c, d = S.BY_NAME[name], S.case_data(S.BY_NAME[name])
    ref = S.reference(c)
    for x, Br in zip(d["t"], ref["B"]):
        Br = np.asarray(Br, dtype=np.float64)
        tol = 8 * c.deg * S.U * np.abs(Br) + S.U
        Bs = si.BSpline.design_matrix(x, d["knots"], c.deg).toarray()
        assert np.all(np.abs(Bs - Br) <= tol), (name, "scipy", np.abs(Bs - Br).max())
        Bo = O.bspline_basis(x, d["ik"], c.deg, d["bk"])
        assert np.all(np.abs(Bo - Br) <= tol), (name, "oracle", np.abs(Bo - Br).max())


def test_partition_of_unity():
    worst = 0.0
    for c in SPLINES:
        for Br in S.reference(c)["B"]:
            worst = max(worst, float(np.abs(Br.sum(axis=1) - 1).max()))
            assert np.all(Br >= 0)
    print(f"largest |sum_p B_p - 1| of the longdouble basis: {worst / EPS_LD:.3g} longdouble epsilons")
    assert worst <= 8 * EPS_LD      # deg <= 5 levels of a convex combination


def test_emulations_pass_and_constants_hold(monkeypatch):
    """both emulations pass every check on every case with the constants as they stand; with G_B = G_SUM = 1 the largest error /
    bound they show is what the constants were set from (and 4 x that is the constant)"""
    for c in S.CASES:
        for variant in ("fma", "plain"):
            res = S.check(c, S.emulate(c, variant))
            assert not res["fails"], f"{c.name}, {variant} emulation:\n" + "\n".join(res["fails"][:8])
    G = dict(B=S.G_B, SUM=S.G_SUM)
    monkeypatch.setattr(S, "G_B", 1.0)
    monkeypatch.setattr(S, "G_SUM", 1.0)
    worst = {v: dict(B=(0.0, ""), SUM=(0.0, "")) for v in ("fma", "plain")}
    for c in S.CASES:
        for variant in ("fma", "plain"):
            w = S.check(c, S.emulate(c, variant))["worst"]
            for k, v in (("B", w["basis"]), ("SUM", max(w["band"], w["s"], w["yy"], w["YY"]))):
                if v > worst[variant][k][0]:
                    worst[variant][k] = (v, c.name)
    for variant in worst:
        for k, (w, where) in worst[variant].items():
            print(f"largest error / (bound at G = 1), {k:3s} {variant:5s}: {w:.3g} ({where})")
    for k, meas in (("B", S.MEASURED_B), ("SUM", S.MEASURED_SUM)):
        for variant in worst:
            assert abs(worst[variant][k][0] - meas[variant]) <= 0.006 * meas[variant], f"{k}, {variant}: the emulation now shows {worst[variant][k][0]:.4g}, stored {meas}"
        assert 3.95 * max(meas.values()) <= G[k] <= 4.1 * max(meas.values()), f"G_{k} = {G[k]} is not 4 x {meas}"


@pytest.mark.parametrize("mut", sorted(S.MUTATIONS))
def test_mutation_is_rejected(mut):
    name, which = S.MUTATIONS[mut]
    c = S.BY_NAME[name]
    clean = S.check(c, S.emulate(c, "fma"))
    assert not clean["fails"], clean["fails"][:4]
    res = S.check(c, S.emulate(c, "fma", mut=mut))
    if which.startswith("exact:"):
        hit = [m for m in res["fails"] if which[6:] in m]
        print(f"{mut} on {name}: {hit[:1]}")
        assert hit, f"{mut} on {name}: no exact check named '{which[6:]}' failed: {res['fails'][:4]}"
    else:
        print(f"{mut} on {name}: {which} error / bound {res['worst'][which]:.3g}")
        assert res["worst"][which] >= 10.0, f"{mut} on {name}: the {which} check sees only {res['worst'][which]:.3g} x its bound"
        assert res["fails"]


def test_case_list_stays_small():
    total = sum(S.n_obs(c) for c in S.CASES)
    print(f"{len(S.CASES)} cases, {total} observations (cap {S.OBS_CAP})")
    assert total < S.OBS_CAP
    assert len(S.CASES) <= 48
    for c in S.CASES:
        n = len(S.reference(c)["ni"])
        assert n <= 20 or c.name.startswith("totals_") or c.name == "mv_n257_P2", (c.name, n)


def test_case_list_covers_the_edges():
    """what the issue's list names is in the case list: every degree with and without knots, PMAX, both lane rounds, padding of
    both parities, every curve length, knots hit, both boundaries and their neighbours, every knot kind, the totals and
    multivariate shapes, both wide bands"""
    shapes = {(c.deg, c.P) for c in SPLINES}
    assert {(g, g + 1) for g in range(1, 6)} | {(g, 64) for g in range(1, 6)} | {(3, 12), (3, 13)} <= shapes
    for g in range(1, 6):
        par = {((g + 2) * c.P + 1) % 2 for c in SPLINES if c.deg == g}
        assert par == ({0, 1} if g % 2 else {1}), (g, par)
    assert {c.knots for c in SPLINES} >= {"uniform", "random", "pair", "dup"} and any(c.bk[0] == 1e6 for c in SPLINES)
    for name in ("cubic_P12", "quint_P64"):
        c, d = S.BY_NAME[name], S.case_data(S.BY_NAME[name])
        assert {len(y) for y in d["y"]} >= {1, 2, c.deg, 63, 64, 65, 255, 256, 257, 512, 513, 700}
    for c in SPLINES:
        if c.n:
            continue
        d = S.case_data(c)
        x = d["t"][d["tags"].index("knots")]
        b0, b1 = d["bk"]
        want = {b0, b1, np.nextafter(b0, b1), np.nextafter(b1, b0)}
        for k in d["ik"]:
            want |= {k, np.nextafter(k, b0), np.nextafter(k, b1)}
        assert want <= set(x), c.name
        assert np.all(d["t"][d["tags"].index("all_b1")] == b1)
        j = S.spans(d["knots"], d["t"][d["tags"].index("one_span")], c.deg, c.P)
        assert np.all(j == j[0]), c.name
        yo = d["y"][d["tags"].index("offset")]
        assert yo.min() > 9e5 and any((y < 0).any() and (y > 0).any() for y in d["y"])
    pair = S.case_data(S.BY_NAME["cubic_P13"])["ik"]
    assert 0 < np.diff(pair).min() < 2e-9
    assert np.diff(S.case_data(S.BY_NAME["lin_P5_dup"])["ik"]).min() == 0
    assert {len(S.reference(c)["ni"]) for c in S.CASES if c.name.startswith("totals_")} == {1, 255, 256, 257, 513, 1000}
    for c in S.CASES:
        if c.name.startswith("totals_"):
            ni = S.reference(c)["ni"]
            assert (c.deg, c.P) == (1, 2) and 1 <= ni.min() and ni.max() <= 3
            if len(ni) > 1:
                assert (ni % 2).sum() >= 2 and (ni % 2 == 0).any()      # floor(sum / 2) differs from the sum of floors
    assert {(c.n, c.P) for c in S.CASES if c.kind == "mv"} == {(1, 1), (5, 50), (3, 63), (3, 64), (257, 2)}
    assert {c.BW for c in S.CASES if c.kind == "basis"} >= {3, 5, S.BWMID, S.BWWIDE}
