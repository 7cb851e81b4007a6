"""The pair-Gram restatement (pair_gram_ref.py) and its derived bound, without a device: the bound has to be loose enough for
the device's summation order (a float64 emulation of it passes) and tight enough to see one wrong term (every mutation of the
emulation fails)."""
import numpy as np
import pytest

import pair_gram_ref as R

SIZES = [(70, 32), (4096 + 37, 144), (32768, 256)]      # (n, KS): 3, 29 and 128 k-slices
K, M, P, BW = 2, 1, 6, 2
MD = M + 1


def make_data(n, seed=5):
    rng = np.random.default_rng(seed)
    Z = rng.dirichlet(np.full(K, 2.0), size=n)
    chi = rng.standard_normal((n, M)) * rng.choice([0.05, 1.0, 7.0], size=(n, 1))
    Gc = rng.standard_normal((n, (BW + 1) * P))
    for d in range(BW + 1):
        Gc[:, d * P + P - d:(d + 1) * P] = 0.0            # beyond the band's end
    s = rng.standard_normal((n, P)) * 3.0
    return Gc, s, Z, chi


_cache = {}


def case(n):
    if n not in _cache:
        Gc, s, Z, chi = make_data(n)
        _cache[n] = (Gc, s, Z, chi, R.pair_gram_ref(Gc, s, Z, chi, MD))
    return _cache[n]


def test_longdouble_is_wide_or_exact_fallback_agrees():
    # the reference runs in longdouble where that is wider than double, exactly otherwise; both agree on a small case
    Gc, s, Z, chi = make_data(9, seed=2)
    ref = R.pair_gram_ref(Gc, s, Z, chi, MD)
    old = R.LONGDOUBLE_OK
    try:
        R.LONGDOUBLE_OK = False
        ex = R.pair_gram_ref(Gc, s, Z, chi, MD)
    finally:
        R.LONGDOUBLE_OK = old
    if old:
        assert np.finfo(np.longdouble).eps < 1e-18
    assert np.all(np.abs(np.asarray(ref.H, dtype=np.float64) - ex.H) <= 2.0 ** -52 * ex.H_abs)
    assert np.all(np.abs(np.asarray(ref.t, dtype=np.float64) - ex.t) <= 2.0 ** -52 * ex.t_abs)


def test_row_order_and_dense_restatement():
    # rows and columns against the dense definition H_ab = sum_i w_ai w_bi G_i, t_a = sum_i w_ai s_i
    n = 23
    Gc, s, Z, chi, ref = case(n)
    ct = R.chit_of(chi, MD)
    W = np.einsum("ij,im->ijm", Z, ct).reshape(n, K * MD)
    ncc = MD * (MD + 1) // 2
    assert ref.H.shape == (K * (K + 1) // 2 * ncc, (BW + 1) * P) and ref.t.shape == (K * MD, P)
    for a in range(K * MD):
        for b in range(K * MD):
            ja, ma, jb, mb = a // MD, a % MD, b // MD, b % MD
            row = R.tri(K, ja, jb) * ncc + R.tri(MD, ma, mb)
            dense = (W[:, a] * W[:, b]) @ Gc
            np.testing.assert_allclose(np.asarray(ref.H[row], dtype=np.float64), dense, rtol=0, atol=1e-12 * ref.H_abs[row].max())
    np.testing.assert_allclose(np.asarray(ref.t, dtype=np.float64), W.T @ s, rtol=0, atol=1e-12 * ref.t_abs.max())
    assert np.all(ref.H_abs >= np.abs(np.asarray(ref.H, dtype=np.float64)) * (1 - 1e-12))
    # columns beyond a band end: no terms
    for d in range(1, BW + 1):
        assert np.all(ref.H_abs[:, d * P + P - d:(d + 1) * P] == 0.0)


@pytest.mark.parametrize("nks", [1, 3, 4, 5, 7, 8, 32, 33, 36])
def test_reduce_slices_is_a_sum(nks):
    rng = np.random.default_rng(nks)
    part = rng.standard_normal((nks, 5))
    got = R.reduce_slices(part)
    np.testing.assert_allclose(got, part.sum(axis=0), rtol=0, atol=1e-13)
    if nks == 8:      # the order itself: (p0 + p4 + p1 + p5) + (p2 + p6 + p3 + p7), interleaved
        want = (((part[0] + part[4]) + (part[1] + part[5])) + ((part[2] + part[6]) + (part[3] + part[7])))
        assert np.array_equal(got, want)
    if nks == 7:      # the three left-over slices join sum 0
        want = ((((part[0] + part[4]) + part[5]) + part[6]) + part[1]) + (part[2] + part[3])
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n,KS", SIZES)
def test_canonical_order_passes_the_bound(n, KS):
    Gc, s, Z, chi, ref = case(n)
    H, t = R.emulate(Gc, s, Z, chi, MD, KS)
    r, where, rH, rt = R.worst(H, t, ref)
    print(f"n={n} KS={KS}: worst error / bound = {r:.3g} at {where}")
    assert R.assert_pair_gram("emulation", H, t, ref) <= 1.0
    assert np.all(H[ref.H_abs == 0.0] == 0.0)
    # the bound is not loose by orders of magnitude for nothing: a plain float64 sum in any order sits inside it as well
    pf, sf = R.pair_weights(Z, chi, MD)
    Hn = ((pf[0] * pf[1]) * (pf[2] * pf[3])).T @ Gc
    assert R.ratios(Hn, ref.H, ref.H_abs, n).max() <= 1.0


def _mid(st):
    return st["n"] // 2 + 1


def mut_drop_curve(st):
    i = _mid(st)
    st["A"][i] = 0.0
    st["As"][i] = 0.0


def mut_curve_twice(st):
    i = _mid(st)
    st["A"][i] *= 2.0
    st["As"][i] *= 2.0


def mut_swap_weights(st):
    i, k = _mid(st), _mid(st) + 1
    st["A"][[i, k]] = st["A"][[k, i]]
    st["As"][[i, k]] = st["As"][[k, i]]


def mut_swap_columns(st):
    st["G"][:, [1, 2]] = st["G"][:, [2, 1]]
    st["s"][:, [1, 2]] = st["s"][:, [2, 1]]


def mut_drop_slice(st):
    return {(st["n"] - 1) // st["KS"] // 2}


def mut_stale_tail(st):
    # the last, partial 16-curve chunk read as if full: its dead positions hold what the chunk before left there
    n = st["n"]
    end = (n + 15) // 16 * 16
    for key in ("A", "As", "G", "s"):
        st[key][n:end] = st[key][n - 16:end - 16]


def mut_chit0_zero(st):
    # chit_0 = 0 instead of 1: pair row (j 0, j' 1, m 0, m' 1) and single row (j 1, m 0)
    rows = R.pair_rows(st["K"], st["MD"])
    row = int(np.where((rows == (0, 1, 0, 1)).all(axis=1))[0][0])
    st["A"][:, row] = 0.0
    st["As"][:, 1 * st["MD"] + 0] = 0.0


MUTATIONS = {"drop_curve": mut_drop_curve, "curve_twice": mut_curve_twice, "swap_weights": mut_swap_weights,
             "swap_columns": mut_swap_columns, "drop_slice": mut_drop_slice, "stale_tail": mut_stale_tail,
             "chit0_zero": mut_chit0_zero}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
@pytest.mark.parametrize("n,KS", SIZES + [(32768 - 3, 256)])
def test_mutations_fail_the_bound(n, KS, name):
    Gc, s, Z, chi, ref = case(n)
    H, t = R.emulate(Gc, s, Z, chi, MD, KS, mutate=MUTATIONS[name])
    if name == "stale_tail" and n % 16 == 0:
        # no partial chunk at this size: the mutation has nothing to read (n = 32768 - 3 stands in for it)
        H0, t0 = R.emulate(Gc, s, Z, chi, MD, KS)
        assert np.array_equal(H, H0) and np.array_equal(t, t0)
        return
    rH = R.ratios(H, ref.H, ref.H_abs, n)
    rt = R.ratios(t, ref.t, ref.t_abs, n)
    print(f"{name} n={n}: H error / bound = {rH.max():.3g}, t error / bound = {rt.max():.3g}")
    assert rH.max() > 1.0 and rt.max() > 1.0
    with pytest.raises(AssertionError, match="route emulation"):
        R.assert_pair_gram("emulation", H, t, ref)


def test_zero_terms_must_give_exact_zero_and_message_decodes():
    n = 70
    Gc, s, Z, chi, ref = case(n)
    H, t = R.emulate(Gc, s, Z, chi, MD, 32)
    col = 2 * P + P - 1                  # band offset 2, p = P - 1: beyond the band's end
    assert ref.H_abs[4, col] == 0.0
    H[4, col] = 1e-300
    with pytest.raises(AssertionError) as e:
        R.assert_pair_gram("solo", H, t, ref)
    msg = str(e.value)
    j, j2, m, m2 = R.pair_rows(K, MD)[4]
    assert "route solo" in msg and f"(j {j}, j' {j2}, m {m}, m' {m2})" in msg and f"band offset 2, p {P - 1}" in msg
    assert "row tile 0" in msg and f"column tile {col // 16}" in msg and "error / bound = inf" in msg
    H, t = R.emulate(Gc, s, Z, chi, MD, 32)
    t[3, 5] *= 1 + 1e-9
    with pytest.raises(AssertionError, match=r"t\[a 3 = \(j 1, m 1\), p 5\]"):
        R.assert_pair_gram("general", H, t, ref)


def test_multivariate_and_covariate_restatements():
    rng = np.random.default_rng(11)
    n, D = 41, 2
    Gc, s, Z, chi = make_data(n, seed=4)
    # multivariate: G_i = I -> every column of H is the plain sum of the pair weights
    ref = R.pair_gram_ref(None, s, Z, chi, MD, mv=True)
    pf, _ = R.pair_weights(Z, chi, MD)
    w = (pf[0] * pf[1] * pf[2] * pf[3]).sum(axis=0)
    assert ref.H.shape == (9, P)
    np.testing.assert_allclose(np.asarray(ref.H, dtype=np.float64), np.repeat(w[:, None], P, axis=1), rtol=1e-13)
    # covariates: s~_i = s_i - G_i o_i against the dense definition
    X = rng.standard_normal((n, D))
    eta = rng.standard_normal((P, D, K))
    xi = rng.standard_normal((P, D, M, K))
    o, oa = R.cov_offset(Z, chi, X, eta, xi, MD)
    od = np.zeros((n, P))
    for i in range(n):
        for k in range(K):
            u = eta[:, :, k] @ X[i]
            for m in range(M):
                u = u + chi[i, m] * (xi[:, :, m, k] @ X[i])
            od[i] += Z[i, k] * u
    np.testing.assert_allclose(np.asarray(o, dtype=np.float64), od, rtol=0, atol=1e-13 * np.abs(od).max())
    assert np.all(np.asarray(oa, dtype=np.float64) >= np.abs(od) * (1 - 1e-12))
    st, sa = R.stil_ref(Gc, s, o, oa, P, BW)
    Gd = np.zeros((n, P, P))
    for d in range(BW + 1):
        for p in range(P - d):
            Gd[:, p, p + d] = Gd[:, p + d, p] = Gc[:, d * P + p]
    sd = s - np.einsum("ipq,iq->ip", Gd, od)
    np.testing.assert_allclose(np.asarray(st, dtype=np.float64), sd, rtol=0, atol=1e-12 * np.abs(sd).max())
    assert np.all(np.asarray(sa, dtype=np.float64) >= np.abs(sd) * (1 - 1e-12))
    assert np.array_equal(R.band_columns(Gd, BW), Gc)
