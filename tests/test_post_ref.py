"""CPU checks of tests/post_ref.py (no device): both float64 emulations of the post-processing pass stay within the bounds on every
case and on 2400 random curves, and the constants were set from what they show; the rank-M form of the CPO log-density equals the
reference's dense form in long double; every named mutation of the kernel-order emulation breaks its bound on a named case; the case
list visits every class of the launch geometry."""
import numpy as np
import pytest

import post_ref as J

QUANT = ("llik", "mean_pdf", "mean_fit", "joint", "cpo_ll", "paths")


def _ratios(c, variant, mut=None):
    """{quantity: largest error / (bound at G = 1)} of one emulation of one case (paths: the worse of mean and mean_only)"""
    ref = J.ld_pointwise(c)
    out = {}
    if "pw" in c.passes:
        out.update(J.judge_pointwise(c, J.kern_pointwise(c, mut=mut) if variant == "kern" else J.plain_pointwise(c), ref))
    if "paths" in c.passes:
        r = J.judge_paths(c, *(J.kern_paths(c, mut=mut) if variant == "kern" else J.plain_paths(c)), ref)
        out["paths"] = max(r.values())
    if "cpo" in c.passes:
        lr = J.ld_cpo(c)
        mat = J.kern_cpo(c, mut=mut) if variant == "kern" else J.plain_cpo(c)
        out["cpo_ll"] = J.judge_cpo(c, mat, lr)["cpo_ll"]
        fk = c.first_kept
        # the reduction: the matrix's bound carried through, and the few-ulp bound against the emulation's own matrix
        carried = J.G_CPO * lr["b_cpo_carry"] + lr["b_cpo_own"]
        out["cpo"] = J.ratio(J.kern_harmonic(mat[:, fk:]), lr["cpo"], carried)
        own, _, b_own = J.ld_harmonic(mat[:, fk:])
        out["cpo_own"] = J.ratio(J.kern_harmonic(mat[:, fk:]), own, b_own)
    return out


def test_emulations_pass_and_constants_hold():
    worst = {v: {k: (0.0, "") for k in QUANT} for v in ("kern", "plain")}
    for c in J.CASES + J.random_cases():
        for variant in worst:
            r = _ratios(c, variant)
            for k in QUANT:
                if k in r and r[k] > worst[variant][k][0]:
                    worst[variant][k] = (r[k], c.name)
            for k in ("cpo", "cpo_own"):
                assert r.get(k, 0.0) <= 1.0, f"{c.name} ({variant}): log CPO misses its bound, ratio {r[k]:.3g} ({k})"
    for variant in worst:
        for k, (w, where) in worst[variant].items():
            print(f"largest error / (bound at G = 1), {k:9s} {variant:6s}: {w:.3g} ({where})")
    for k in QUANT:
        meas = J.MEASURED[k]
        top = max(worst["kern"][k][0], worst["plain"][k][0])
        assert top <= 1.02 * max(meas.values()), f"{k}: the emulations now show {top:.3g}, the constant was set from {meas}"
        assert 3.95 * max(meas.values()) <= J.G[k] <= 4.1 * max(meas.values()), f"{k}: G = {J.G[k]} is not {J.MARGIN} x {meas}"
        # conditioning: the kernel-order emulation has room on every case
        assert worst["kern"][k][0] <= J.G[k] / 2


def test_rank_m_form_equals_dense_form():
    """calcLikelihoodCPO forms the n_i x n_i covariance; the device (and ld_cpo) the M x M system.  In long double the two agree to a
    small fraction (2^-9) of the float64 bound on every curve of up to 64 observations."""
    seen = 0
    for c in J.CASES:
        if "cpo" not in c.passes or max(c.lens) > 64:
            continue
        a, b = J.ld_cpo(c), J.ld_cpo(c, dense=True)
        r = J.ratio(b["ll"], a["ll"], a["b_ll"])
        assert r <= 2.0 ** -9, f"{c.name}: dense and rank-M forms differ by {r:.3g} of the bound"
        seen += sum(c.lens) > 0
    small = J.Case("dense_small", [1, 2, 3, 4, 5, 63, 64], K=3, M=2, P=9, T=4)
    d = J.make_data(small)
    a, b = J.ld_cpo(small, d), J.ld_cpo(small, d, dense=True)
    assert J.ratio(b["ll"], a["ll"], a["b_ll"]) <= 2.0 ** -9
    assert seen >= 3


# the case that catches each mutation, and the quantity that misses its bound there
CAUGHT_BY = {
    "zskip": ("zskip", "llik"),                       # the NaN rows of the skipped cluster reach every draw's sum
    "ni_for_ni_minus_M": ("mix_cubic", "cpo_ll"),
    "segment": ("mix_cubic", "cpo_ll"),
    "pad": ("mix_cubic", "cpo_ll"),                   # curves of 1, 2, 3, 5, 13, 27, 63, 65, 129 observations have pad rows
    "first_kept": ("mix_cubic", "mean_fit"),
    "tile_last": ("mix_cubic", "llik"),               # T = 33, G = 32: draw 31 is a tile's last
    "clamp": ("mix_cubic", "llik"),                   # rows at x = 1 start at column P - 1 > P - W
    "chol_sigma": ("m9", "cpo_ll"),
    "chunk0": ("t65", "mean_pdf"),                    # three chunks, first_kept = 3 inside chunk 0
    "logsd": ("t1", "llik"),
}


@pytest.mark.parametrize("mut", J.MUTATIONS)
def test_mutations_are_caught(mut):
    name, quantity = CAUGHT_BY[mut]
    c = J.CASE[name]
    clean, broken = _ratios(c, "kern"), _ratios(c, "kern", mut=mut)
    assert clean[quantity] <= J.G[quantity], f"{name}: the unmutated emulation misses the {quantity} bound"
    assert not broken[quantity] <= J.G[quantity], f"mutation {mut} passes the {quantity} bound of case {name} (ratio {broken[quantity]:.3g})"
    print(f"mutation {mut}: caught by {name} ({quantity}: error / bound {broken[quantity] / J.G[quantity]:.3g})")


def test_case_list_covers_every_geometry_class():
    seen = {"pw": set(), "cpo": set()}
    for c in J.CASES:
        for p, s in J.classes(c).items():
            seen[p] |= s
    for p, need in J.REQUIRED_CLASSES.items():
        assert need <= seen[p], f"{p}: classes not visited: {sorted(need - seen[p])}"
    lens = {ni for c in J.CASES for ni in c.lens}
    assert {1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 256, 257, 1024, 307, 308, 936} <= lens
    g = {c.name: J.case_geometry(c) for c in J.CASES}
    assert g["gc1"]["cpo"]["Gc"] == 1 and g["long"]["cpo"]["gc_class"] == "budget" and g["long"]["cpo"]["NIPX"] == 1024
    assert g["t65"]["NCH"] == 3 and g["t1"]["NCH"] == 1
    assert {g[nm]["R"] for nm in ("r12_d8", "r13_m0", "r24")} == {12, 13, 24} and g["k8m16"]["batches"] == 12
    assert any((c.T - c.first_kept) % g[c.name]["cpo"]["Gc"] for c in J.CASES if "cpo" in c.passes)
    assert {c.M for c in J.CASES if "cpo" in c.passes} >= {1, 8, 9, 16}
    assert {(c.D, c.cov) for c in J.CASES} >= {(0, "none"), (1, "eta"), (1, "etaxi"), (8, "eta"), (8, "etaxi")}
    assert {c.P for c in J.CASES if c.basis == "identity"} == {1, 7, 64}
    assert {(c.T, c.first_kept) for c in J.CASES} >= {(1, 0), (33, 0), (33, 5), (33, 32), (33, 17), (65, 3)}
    # staging on either side of n_i (W | 1) = 1536 in one cubic case; the tensor-product case is never staged
    st = {q["ni"]: q["staged"] for q in g["long"]["pw"]}
    assert st[307] and not st[308] and not any(q["staged"] for q in g["tensor"]["pw"])
    # the refused tile: padded length 940 at M = 16, P = 8
    gc0 = next(q[0] for q in J.REFUSED if q[0].name == "gc0")
    assert J.case_geometry(gc0)["cpo"]["Gc"] == 0 and J.case_geometry(gc0)["cpo"]["NIPX"] == 940
