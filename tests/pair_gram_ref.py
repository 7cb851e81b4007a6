"""High-precision restatement of the pair-Gram contraction and its entry-by-entry tolerance.  (Test infrastructure.)

What the device computes (kernels_pair_gram.hip: k_pair_gram + k_pg_reduce, k_pair_gram_pack + k_pg_reduce_pack):

    H[row, d P + p] = sum_i (Z_ij Z_ij') (chit_im chit_im') G_i[p, p + d]      row = tri(K, j, j') NCC + tri(MD, m, m')
    t[j MD + m, p]  = sum_i  Z_ij chit_im  s_i[p]                              chit_i0 = 1, chit_i,m+1 = chi_im

over the per-curve records rec_i = [G_i band-packed, diagonal-major | s_i | yy_i] (model.hpp).  Multivariate model: G_i = I,
the band has one diagonal and H[row, p] is the same sum of weights for every p.  Covariate-adjusted models contract the s part
against s~_i = s_i - G_i o_i, o_i = sum_k Z_ik sum_d X_id (eta_k[:, d] + sum_m chi_im xi_km[:, d]) (k_curve_z).

Reference: the same sums in np.longdouble (64-bit significand; every product of two doubles and every partial sum carries a
relative error of 2^-64, so the reference is off by at most about 4 (n + 3) 2^-64 S_abs -- under 1 % of the bound below), or,
where longdouble is no wider than double, exactly (rational arithmetic, small shapes only).

Tolerance, DERIVED and not tuned.  Write u = 2^-53 and S_abs[entry] = sum_i |term_i| (the sum of the absolute values of the
terms of that entry).  A term is a product of at most four stored (already rounded) factors and a record entry:
  * the weight (Z_j Z_j') (chit_m chit_m') costs three roundings (two inner products, one outer): relative error <= 3 u;
  * the MFMA multiplies the weight by the record entry and adds it to the accumulator fused, one rounding per addition; a
    k-slice of KS curves is one accumulation chain, at most KS additions, of which at most min(KS, n) see a non-zero term;
  * the NKS slice sums are combined as four interleaved sums, the <= 3 left-over slices and (s0 + s1) + (s2 + s3): at most
    NKS / 4 + 5 further additions on the path of any one term.
A term therefore passes through at most 3 + min(KS, n) + NKS / 4 + 5 roundings (padding curves add exact zeros, which do not
round).  With one slice NKS / 4 = 0; with NKS >= 2 slices of KS >= 16 curves n > KS (NKS - 1) >= KS + 16 (NKS - 2), which
exceeds KS + NKS / 4: in every geometry min(KS, n) + NKS / 4 <= n, so first-order
    |H - H_ref| <= (n + 8) u S_abs         entry by entry, the same form for t,
whatever the order of the additions (the standard bound |fl(sum) - sum| <= gamma_k sum |x_i| holds for any order with k the
longest chain).  No scaling by a global maximum anywhere.  An entry with S_abs == 0 (a band column beyond the band's end, where
every record holds 0.0) must be exactly 0.0.
Covariates: s~_i is itself computed on the device: o_i is a sum of K D MD products of up to four factors, G_i o_i a band
product of 2 BW + 1 terms, then one subtraction, so |s~_i - exact| <= (K D MD + 2 BW + 8) u (|s_i| + |G_i| o_abs_i), which
enters t as `extra` = K D MD + 2 BW + 8 more roundings on S_abs = sum_i |w_ai| (|s_i| + |G_i| o_abs_i).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)
LD = np.longdouble


def tri(n, a, b):
    """index of (a, b) in the packed upper triangle of an n x n symmetric table (tri_index, model.hpp)"""
    a, b = min(a, b), max(a, b)
    return a * n - a * (a - 1) // 2 + (b - a)


def pair_rows(K, MD):
    """(R, 4) table: row -> (j, j', m, m'), j <= j', m <= m', in the device's row order"""
    zz = [(a, b) for a in range(K) for b in range(a, K)]
    cc = [(a, b) for a in range(MD) for b in range(a, MD)]
    return np.array([(j, j2, m, m2) for (j, j2) in zz for (m, m2) in cc], dtype=np.int64)


def chit_of(chi, MD):
    n = chi.shape[0]
    return np.concatenate([np.ones((n, 1)), np.asarray(chi, dtype=np.float64)], axis=1)[:, :MD]


def band_columns(G, BW):
    """n x P x P symmetric blocks -> n x (BW + 1) P band-packed, diagonal-major columns (col = d P + p = G[p, p + d])"""
    n, P, _ = G.shape
    out = np.zeros((n, (BW + 1) * P), dtype=G.dtype)
    for d in range(BW + 1):
        for p in range(P - d):
            out[:, d * P + p] = G[:, p, p + d]
    return out


def records_from_basis(B, y, BW):
    """the record columns from basis matrices and observations: G part (n x LG) and s part (n x P), in float64 as the device
    stores them (the device's own values, `smp.debug("rec")`, are the factors the bound speaks about: prefer those)"""
    G = np.stack([b.T @ b for b in B])
    s = np.stack([b.T @ v for b, v in zip(B, y)])
    return band_columns(G, BW), s


def split_records(rec, LG, P):
    return rec[:, :LG], rec[:, LG:LG + P]


def _wsum(factors, cols):
    """sum_i prod_f factors[f][i, r] * cols[i, c] -> (R, C), in longdouble (or exactly)"""
    if LONGDOUBLE_OK:
        W = np.ones(factors[0].shape, dtype=LD)
        for f in factors:
            W = W * f.astype(LD)
        return W.T @ cols.astype(LD)
    n, R = factors[0].shape
    C = cols.shape[1]
    out = np.zeros((R, C), dtype=np.float64)
    for r in range(R):
        w = [Fraction(1)] * n
        for f in factors:
            w = [a * Fraction(float(b)) for a, b in zip(w, f[:, r])]
        for c in range(C):
            out[r, c] = float(sum((a * Fraction(float(b)) for a, b in zip(w, cols[:, c])), Fraction(0)))
    return out


def pair_weights(Z, chi, MD):
    """the factor tables of the pair rows and of the single rows: lists of n x R (n x A) float64 arrays whose product is the weight"""
    Z = np.asarray(Z, dtype=np.float64)
    K = Z.shape[1]
    ct = chit_of(chi, MD)
    rows = pair_rows(K, MD)
    pf = [Z[:, rows[:, 0]], Z[:, rows[:, 1]], ct[:, rows[:, 2]], ct[:, rows[:, 3]]]
    ja = np.repeat(np.arange(K), MD)
    ma = np.tile(np.arange(MD), K)
    sf = [Z[:, ja], ct[:, ma]]
    return pf, sf


def cov_offset(Z, chi, X, eta, xi, MD):
    """o_i (n x P, longdouble) and the sum of the absolute values of its terms; eta: (P, D, K), xi: (P, D, M, K)"""
    Z, X = np.asarray(Z, dtype=LD), np.asarray(X, dtype=LD)
    ct = chit_of(chi, MD).astype(LD)
    th = [np.asarray(eta, dtype=LD)] + [np.asarray(xi[:, :, m, :], dtype=LD) for m in range(MD - 1)]    # mt -> (P, D, K)
    n, P = Z.shape[0], eta.shape[0]
    o = np.zeros((n, P), dtype=LD)
    oa = np.zeros((n, P), dtype=LD)
    for mt, t in enumerate(th):
        for k in range(Z.shape[1]):
            w = (Z[:, k] * ct[:, mt])[:, None] * X            # n x D
            o += w @ t[:, :, k].T
            oa += np.abs(w) @ np.abs(t[:, :, k]).T
    return o, oa


def stil_ref(Gc, s, o, oa, P, BW):
    """s~_i = s_i - G_i o_i from the band-packed columns, and |s_i| + |G_i| o_abs_i"""
    Gc, s = np.asarray(Gc, dtype=LD), np.asarray(s, dtype=LD)
    st, sa = s.copy(), np.abs(s)
    for d in range(BW + 1):
        for p in range(P - d):
            g = Gc[:, d * P + p]
            st[:, p] -= g * o[:, p + d]
            sa[:, p] += np.abs(g) * oa[:, p + d]
            if d > 0:
                st[:, p + d] -= g * o[:, p]
                sa[:, p + d] += np.abs(g) * oa[:, p]
    return st, sa


class Ref:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def pair_gram_ref(Gc, s, Z, chi, MD, mv=False, s_abs=None):
    """H_ref (R x LG), t_ref (A x P) and the per-entry sums of absolute terms.  Gc: n x LG band-packed G columns (ignored for
    the multivariate model: G_i = I, one diagonal of ones), s: n x P (s_i, or s~_i with s_abs = |s_i| + |G_i| o_abs_i)."""
    Z = np.asarray(Z, dtype=np.float64)
    n, K = Z.shape
    P = s.shape[1]
    if mv:
        Gc = np.ones((n, P))
    pf, sf = pair_weights(Z, chi, MD)
    H = _wsum(pf, np.asarray(Gc))
    t = _wsum(sf, np.asarray(s))
    apf, asf = [np.abs(f) for f in pf], [np.abs(f) for f in sf]
    H_abs = np.asarray(_wsum(apf, np.abs(np.asarray(Gc))), dtype=np.float64)
    t_abs = np.asarray(_wsum(asf, np.abs(np.asarray(s)) if s_abs is None else np.asarray(s_abs)), dtype=np.float64)
    return Ref(H=H, t=t, H_abs=H_abs, t_abs=t_abs, n=n, K=K, MD=MD, P=P, LG=np.asarray(Gc).shape[1], mv=mv)


def bound(n, S_abs, extra=0):
    return (n + 8 + extra) * U * S_abs


def ratios(got, ref, S_abs, n, extra=0):
    """|got - ref| / bound entry by entry; entries with S_abs == 0 give 0 if got is exactly 0.0 and inf otherwise"""
    got = np.asarray(got, dtype=np.float64)
    err = np.asarray(np.abs(got.astype(LD) - ref), dtype=np.float64) if LONGDOUBLE_OK else np.abs(got - ref)
    b = bound(n, S_abs, extra)
    out = np.where(got == 0.0, 0.0, np.inf)
    nz = S_abs > 0
    out[nz] = err[nz] / b[nz]
    out[~np.isfinite(got)] = np.inf
    return out


def decode_H(ref, row, col):
    j, j2, m, m2 = pair_rows(ref.K, ref.MD)[row]
    d, p = divmod(col, ref.P)
    return (f"H[row {row} = (j {j}, j' {j2}, m {m}, m' {m2}), col {col} = (band offset {d}, p {p})] "
            f"row tile {row // 16} (row {row % 16} of it), column tile {col // 16} (column {col % 16}; 32-column pair {col // 32})")


def decode_t(ref, a, p):
    return (f"t[a {a} = (j {a // ref.MD}, m {a % ref.MD}), p {p}] row tile {a // 16} (row {a % 16} of it), "
            f"column tile {p // 16} (column {p % 16})")


def worst(got_H, got_t, ref, extra_t=0):
    """(ratio, message) of the worst entry of H and of t"""
    rH = ratios(np.asarray(got_H).reshape(ref.H.shape), ref.H, ref.H_abs, ref.n)
    rt = ratios(np.asarray(got_t).reshape(ref.t.shape), ref.t, ref.t_abs, ref.n, extra_t)
    iH = np.unravel_index(np.argmax(rH), rH.shape)
    it = np.unravel_index(np.argmax(rt), rt.shape)
    if rH[iH] >= rt[it]:
        return rH[iH], decode_H(ref, int(iH[0]), int(iH[1])), rH, rt
    return rt[it], decode_t(ref, int(it[0]), int(it[1])), rH, rt


def assert_pair_gram(route, got_H, got_t, ref, extra_t=0):
    """entry-by-entry check of H and t against the reference; the message decodes the worst entry"""
    got_H = np.asarray(got_H, dtype=np.float64).reshape(ref.H.shape)
    got_t = np.asarray(got_t, dtype=np.float64).reshape(ref.t.shape)
    r, where, rH, rt = worst(got_H, got_t, ref, extra_t)
    nbad = int((rH > 1).sum() + (rt > 1).sum())
    if ref.mv:
        assert np.array_equal(got_H, np.repeat(got_H[:, :1], ref.P, axis=1)), f"{route}: multivariate H differs across p"
    assert r <= 1.0, (f"route {route}: {where}: error / bound = {r:.3g} (bound (n + 8) 2^-53 S_abs, n = {ref.n}); "
                      f"{nbad} of {rH.size + rt.size} entries beyond their bound")
    return r


# ---- float64 emulation of the canonical summation order (tests of the bound itself, no device) ----
def reduce_slices(part):
    """k_pg_reduce: part (NKS, ...) -> four interleaved sums over NKS & ~3 slices, left-over slices on sum 0, (s0+s1)+(s2+s3)"""
    NKS = part.shape[0]
    nfull = NKS & ~3
    sg = [np.zeros(part.shape[1:]) for _ in range(4)]
    for g in range(4):
        for k in range(g, nfull, 4):
            sg[g] = sg[g] + part[k]
    for k in range(nfull, NKS):
        sg[0] = sg[0] + part[k]
    return (sg[0] + sg[1]) + (sg[2] + sg[3])


def emulate(Gc, s, Z, chi, MD, KS, mutate=None):
    """H, t in float64 in the device's order: slices of KS curves, one accumulation chain per slice over steps of four
    consecutive curves, slices combined by reduce_slices.  mutate(dict) may alter the staged operands: it receives
    A (n_pad x R pair weights), As (n_pad x A single weights), G (n_pad x LG), s (n_pad x P), n, KS and may return a set of
    slice indices whose partial sums are dropped."""
    Z = np.asarray(Z, dtype=np.float64)
    n = Z.shape[0]
    NKS = (n + KS - 1) // KS
    npad = NKS * KS
    pf, sf = pair_weights(Z, chi, MD)
    A = (pf[0] * pf[1]) * (pf[2] * pf[3])          # the device's association
    As = sf[0] * sf[1]
    pad = lambda x: np.concatenate([x, np.zeros((npad - n,) + x.shape[1:])], axis=0)
    st = dict(A=pad(A), As=pad(As), G=pad(np.asarray(Gc, dtype=np.float64)), s=pad(np.asarray(s, dtype=np.float64)), n=n, KS=KS,
              pf=pf, MD=MD, K=Z.shape[1])
    dropped = mutate(st) if mutate else None
    out = []
    for W, B in ((st["A"], st["G"]), (st["As"], st["s"])):
        Wk = W.reshape(NKS, KS, -1)
        Bk = B.reshape(NKS, KS, -1)
        acc = np.zeros((NKS, Wk.shape[2], Bk.shape[2]))
        for il in range(KS):                      # (curve il of every slice at once: the chains of different slices are independent)
            acc = acc + Wk[:, il, :, None] * Bk[:, il, None, :]
        if dropped:
            acc[sorted(dropped)] = 0.0
        out.append(reduce_slices(acc))
    return out[0], out[1]
