"""High-precision restatement of the record builder (csrc/kernels_stats.hip: eval_basis, k_stats_functional<1..5>,
k_stats_multivariate, k_stats_totals; the host loop of bfmmm_create_from_basis in csrc/bfmmm_capi.hip), its exact checks, its
bounds, two float64 emulations and the case list shared by tests/test_stats_ref.py (CPU) and tests/test_gpu_stats.py (device).
(Test infrastructure.)  u = 2^-53; every reference value is np.longdouble.

What the builder leaves, per curve i with n_i observations (t_l, y_l) and basis rows B_i (n_i x P):

    rec_i = [ G(p, p + d) at d P + p, d <= BW | s_p = sum_l B_lp y_l at LG + p | yy = sum_l y_l^2 at LG + P | 0 up to LREC ]
    LG = (BW + 1) P,   LREC = LG + P + 1 rounded up to even,   ni[i] = n_i
    YY = sum_i yy_i,   n_obs_total = sum_i n_i,   half_sum = sum_i floor(n_i / 2)

BW = min(degree, P - 1) for the spline model, 0 for the multivariate one (B_i = I: rec_i = [1 .. 1 | y_i | yy_i | 0], ni = P), and
for a supplied basis of half-bandwidth `band`: min(band, P - 1) up to 5, 15 (BWMID) up to 15, 31 (BWWIDE) above, zero padded.

Reference (reference()).  The clamped knot vector; the span of x is the largest j in [deg, P - 1] with knots[j] <= x (right-continuous,
the right boundary in the last span); the Cox-de Boor triangle with 0 / 0 = 0 (scipy's convention at a repeated knot) in
longdouble; dense rows, and from them (or from the supplied rows, taken as exact) every record entry as a longdouble sum.

Bounds (check()).  The triangle adds only non-negative terms, so a basis value carries a RELATIVE error
    eps_B = G_B deg u                                                          (0 for a supplied basis and the multivariate model)
and with T_e = sum_l |term_l| of entry e (= the entry itself for the band of a spline basis and for yy):
    band   (G_SUM (n_i + 1) u + 2 eps_B) T_e         a sum, in observation order, of n_i products of two basis values
    s      (G_SUM (n_i + 1) u + eps_B) T_e           T_e = sum_l |B_lp| |y_l|
    yy     G_SUM (n_i + 1) u yy
    YY     G_SUM (ceil(n / 256) + 256 + max n_i + 1) u sum_i yy_i
(n_i additions and one product rounding per term; YY: the entries' own errors, a thread's piece of ceil(n / 256) entries and the
sequential sum of 256 pieces.)  Where the reference is exactly 0 the bound is 0: the entry must be 0.0.

Exact checks (check()).  The first non-zero index of every basis row is the reference's; zeros outside the deg + 1 window
[span - deg, span]; B[x = b0][0] == 1.0 and B[x = b1][P - 1] == 1.0; band slots with p + d >= P and the padding e > LG + P are 0.0;
ni, n_obs_total, half_sum as integers; multivariate: the first P entries exactly 1.0, the next P exactly y.

Constants.  G_B and G_SUM are 4 x the largest error / (bound with G_B = G_SUM = 1) of two float64 emulations of the kernel's order
over CASES (chunks of 256 observations, one accumulator per entry e summed in observation order, the totals as 256 contiguous
per-thread pieces and a sequential sum of 256; `fma`: every a + b c of the triangle and of the accumulations fused, as the device
build contracts them -- the fused operation is restated as a longdouble product and sum, exact to 2^-11 ulp --; `plain`: every
product rounded), measured by tests/test_stats_ref.py::test_emulations_pass_and_constants_hold, never from a device run:

    basis:  fma 1.73 (lin_P5_dup),       plain 1.73 (lin_P5_dup)                 ->  G_B = 6.9
    sums:   fma 0.697 (lin_P64),         plain 0.697 (lin_P64)                   ->  G_SUM = 2.79
(both figures come from degree 1, where the triangle has no sum to fuse and a one-point curve's band entry is one product: the two
emulations agree there; the sums' figure is the largest over band, s, yy and YY.)

Underflow.  x = nextafter(0, 1) is subnormal, and a product of two tiny basis values falls below 2^-1022 = eta, where float64
rounds absolutely: every non-zero basis value's bound carries + eta, every non-zero band entry's + n_i eta, every non-zero s
entry's + eta sum_l |y_l|.

The triangle's form.  eval_basis computes temp = N[q] / denom, N'[q] = saved + right temp, saved' = left temp.  Where one of the two
knot differences is 0 the other's weight is denom / denom = 1, but right (N[q] / right) can return N[q] (1 - u): the parent of
this test returned B[b1][P - 1] = 1 - u on quart_P64 and quart_P11 and B[b0][0] = 1 - u on cubic_P12.  eval_basis therefore hands N[q]
on as it is where left == 0 (right != 0) or right == 0 (left != 0), which leaves every other value bit for bit as it was and makes
the boundary values exactly 1.0; the textbook form is kept as the `recip` emulation (MUTATIONS["recip_form"]).

Cases.  The smallest shapes at which the builder can still go wrong: every degree with no internal knot and with P = 64 (PMAX; at
degree 5 yy sits at e = 448, lane 0's q = 7), cubic P = 12 / 13 ((BW + 2) P + 1 = 61 / 66, either side of one lane round), LG + P + 1 odd
(padding) for every degree and even for the odd degrees ((deg + 2) P is even whenever deg is: no such shape exists for degrees 2
and 4).  Every spline case holds a curve of all internal knots, their neighbours (nextafter) on both sides, both boundaries
and their inner neighbours; a curve inside one span; a curve of b1 alone; a curve offset by 1e6; lengths 1, 2, deg, 63, 64, 65 and,
in cubic_P12 and quint_P64, 255, 256, 257, 512, 513, 700.  Knots: uniform, random, a pair 1e-9 apart, one duplicated, boundaries at
[1e6, 1e6 + 1].  The totals cases are degree 1, P = 2, curves of 1..3 points.  OBS_CAP caps the observations of the whole list.
"""
import zlib

import numpy as np

import factor_ref as F

U, LD = F.U, F.LD
CHUNK, PMAX, BWMAX, BWMID, BWWIDE = 256, 64, 5, 15, 31
ETA = LD(2.0) ** -1022      # the smallest normal float64
OBS_CAP = 30000     # observations over all cases (tests/test_stats_ref.py::test_case_list_stays_small)

# measured by tests/test_stats_ref.py::test_emulations_pass_and_constants_hold (largest error / bound at G_B = G_SUM = 1 over CASES)
MEASURED_B = {"fma": 1.73, "plain": 1.73}
MEASURED_SUM = {"fma": 0.697, "plain": 0.697}
G_B, G_SUM = 6.9, 2.79

SHORT = (1, 2, "deg", 63, 64, 65)
FULL = SHORT + (255, 256, 257, 512, 513, 700)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """kind "spline" (t, y, knots), "mv" (Y), "basis" (supplied rows: src names the spline case whose rows are passed back, or
    band > 5 a dense-in-band matrix)"""
    def __init__(self, name, kind, deg=0, P=0, knots="uniform", bk=(0.0, 1.0), lengths=SHORT, n=0, band=0, src=None):
        self.name, self.kind, self.deg, self.P, self.knots, self.bk, self.lengths, self.n, self.band, self.src = name, kind, deg, P, knots, bk, lengths, n, band, src
        if kind == "spline":
            self.BW = min(deg, P - 1)
        elif kind == "mv":
            self.BW = 0
        else:
            self.BW = min(band, P - 1) if band <= BWMAX else BWMID if band <= BWMID else BWWIDE
        self.LG = (self.BW + 1) * P
        self.LREC = (self.LG + P + 2) // 2 * 2


FAR = (1e6, 1e6 + 1.0)
DEGNAME = {1: "lin", 2: "quad", 3: "cubic", 4: "quart", 5: "quint"}


def _cases():
    cs = [Case(f"{DEGNAME[g]}_P{g + 1}", "spline", deg=g, P=g + 1) for g in range(1, 6)]      # no internal knot; LG + P + 1 odd
    cs += [Case("lin_P64", "spline", deg=1, P=64), Case("quad_P64", "spline", deg=2, P=64, knots="random"),
           Case("cubic_P64", "spline", deg=3, P=64, knots="pair"), Case("quart_P64", "spline", deg=4, P=64, knots="random"),
           Case("quint_P64", "spline", deg=5, P=64, lengths=FULL)]                                 # yy at e = 448: lane 0, q = 7
    cs += [Case("cubic_P12", "spline", deg=3, P=12, knots="random", lengths=FULL),                # 61 outputs: one lane round
           Case("cubic_P13", "spline", deg=3, P=13, knots="pair"),                                # 66: two; even, no padding
           Case("lin_P5_dup", "spline", deg=1, P=5, knots="dup"),                                 # a discontinuous basis; 16, even
           Case("cubic_P9_dup", "spline", deg=3, P=9, knots="dup"),
           Case("quad_P10_far", "spline", deg=2, P=10, knots="random", bk=FAR),
           Case("quart_P11", "spline", deg=4, P=11, knots="pair"),
           Case("quint_P9_far", "spline", deg=5, P=9, bk=FAR)]                                    # 64 outputs: even, exactly one round
    cs += [Case(f"totals_n{n}", "spline", deg=1, P=2, n=n, lengths=()) for n in (1, 255, 256, 257, 513, 1000)]
    cs += [Case(f"mv_n{n}_P{P}", "mv", P=P, n=n) for n, P in ((1, 1), (5, 50), (3, 63), (3, 64), (257, 2))]
    cs += [Case("basis_cubic_P12", "basis", P=12, band=3, src="cubic_P12"), Case("basis_quint_P9_far", "basis", P=9, band=5, src="quint_P9_far"),
           Case("basis_band6_P20", "basis", P=20, band=6, n=6), Case("basis_band16_P40", "basis", P=40, band=16, n=6)]
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_data, _ref = {}, {}


def knot_vector(ik, bk, deg):
    return np.concatenate([[bk[0]] * (deg + 1), np.asarray(ik, dtype=np.float64), [bk[1]] * (deg + 1)])


def _internal_knots(c, rng):
    m, (b0, b1) = c.P - c.deg - 1, c.bk
    if m == 0:
        return np.zeros(0)
    if c.knots == "uniform":
        return np.linspace(b0, b1, m + 2)[1:-1]
    ik = np.sort(rng.uniform(b0 + 0.02 * (b1 - b0), b1 - 0.02 * (b1 - b0), size=m))
    if c.knots == "pair" and m >= 2:
        ik[m // 2] = ik[m // 2 - 1] + 1e-9
    if c.knots == "dup" and m >= 2:
        ik[m // 2] = ik[m // 2 - 1]
    return ik


def rw1(P):
    """the RW1 penalty of the nu prior (BFMMM.h:1027-1037), half-bandwidth 1"""
    Pm = 2.0 * np.eye(P) - np.eye(P, k=1) - np.eye(P, k=-1)
    Pm[0, 0] = Pm[P - 1, P - 1] = 1.0
    return Pm


def case_data(c):
    """spline: dict(t, y (lists), ik, bk, knots, tags); mv: dict(Y); basis: dict(B, y (lists), Pmat, pen_band)"""
    if c.name in _data:
        return _data[c.name]
    rng = np.random.default_rng(zlib.crc32(("stats" + c.name).encode()))
    if c.kind == "mv":
        d = dict(Y=rng.standard_normal((c.n, c.P)) * 2.0)
        if c.n > 1:
            d["Y"][1] += 1e6
    elif c.kind == "basis" and c.src:
        s = case_data(BY_NAME[c.src])
        d = dict(B=[basis_f64(s["knots"], x, BY_NAME[c.src].deg, c.P) for x in s["t"]], y=s["y"], Pmat=rw1(c.P), pen_band=1)
    elif c.kind == "basis":      # dense in band: every row has band + 1 non-zero entries from a random column on, of mixed sign
        ni = [1, 2, 65, 257, 40, 31][:c.n]
        B = []
        for k in ni:
            b = np.zeros((k, c.P))
            for l, f in enumerate(rng.integers(0, c.P - c.band, size=k)):
                b[l, f:f + c.band + 1] = rng.uniform(-1.0, 1.0, size=c.band + 1)
            B.append(b)
        d = dict(B=B, y=[rng.standard_normal(k) * 2.0 for k in ni], Pmat=rw1(c.P), pen_band=1)
    else:
        ik = _internal_knots(c, rng)
        b0, b1 = c.bk
        knots = knot_vector(ik, c.bk, c.deg)
        t, tags = [], []
        if c.n:      # totals: n curves of 1..3 points
            ln = rng.integers(1, 4, size=c.n)
            t = [rng.uniform(b0, b1, size=k) for k in ln]
            tags = ["totals"] * c.n
        else:
            edge = [b0, b1, np.nextafter(b0, b1), np.nextafter(b1, b0)]
            for k in np.unique(ik):
                edge += [k, np.nextafter(k, b0), np.nextafter(k, b1)]
            t.append(rng.permutation(np.array(edge)))
            tags.append("knots")
            uk = np.unique(knots)
            j = int(rng.integers(0, len(uk) - 1))
            t.append(rng.uniform(np.nextafter(uk[j], b1), uk[j + 1], size=7) if uk[j + 1] - uk[j] > 1e-6 else np.full(7, np.nextafter(uk[j], b1)))
            tags.append("one_span")
            t.append(np.full(5, b1))
            tags.append("all_b1")
            t.append(rng.uniform(b0, b1, size=33))
            tags.append("offset")
            for k in c.lengths:
                t.append(rng.uniform(b0, b1, size=c.deg if k == "deg" else k))
                tags.append("ragged")
        y = [rng.standard_normal(len(x)) * 2.0 for x in t]
        if "offset" in tags:
            y[tags.index("offset")] = 1e6 + rng.standard_normal(33)
        d = dict(t=t, y=y, ik=ik, bk=np.array(c.bk), knots=knots, tags=tags)
    _data[c.name] = d
    return d


def n_obs(c):
    d = case_data(c)
    return c.n * c.P if c.kind == "mv" else int(sum(len(y) for y in d["y"]))


# ---------------------------------------------------------------------------------------------------------------------
# the basis
# ---------------------------------------------------------------------------------------------------------------------
def spans(knots, x, deg, P, left=False):
    """the largest j in [deg, P - 1] with knots[j] <= x (left: < x, the left-continuous rule)"""
    return np.clip(np.searchsorted(knots, x, side="left" if left else "right") - 1, deg, P - 1)


def _fma(a, b, c):
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


def triangle(knots, x, j, deg, dtype=LD, fma=False, recip=False):
    """the deg + 1 non-zero basis values of every x in span j (Cox-de Boor, 0 / 0 = 0), in eval_basis's order of operations
    (recip: the textbook form, N / denom first)"""
    kn, xv = np.asarray(knots, dtype=np.float64).astype(dtype), np.asarray(x, dtype=np.float64).astype(dtype)
    N = np.zeros((len(xv), deg + 1), dtype=dtype)
    N[:, 0] = 1
    for d in range(1, deg + 1):
        saved = np.zeros(len(xv), dtype=dtype)
        for q in range(d):
            right, left = kn[j + q + 1] - xv, xv - kn[j + 1 - d + q]
            denom = right + left
            ok = denom != 0
            safe = np.where(ok, denom, 1)
            nq = N[:, q].copy()
            temp = np.where(ok, nq / np.where(ok, denom, 1), 0)
            new = _fma(right, temp, saved) if fma else saved + right * temp
            nxt = left * temp
            if not recip:      # a zero difference hands N[q] on as it is
                new = np.where((left == 0) & (right != 0), saved + nq, new)
                nxt = np.where((right == 0) & (left != 0), nq, nxt)
            N[:, q], saved = new, nxt
        N[:, d] = saved
    return N


def dense(N, first, P):
    B = np.zeros((N.shape[0], P), dtype=N.dtype)
    for q in range(N.shape[1]):
        B[np.arange(N.shape[0]), first + q] = N[:, q]
    return B


def basis_ld(knots, x, deg, P):
    j = spans(knots, x, deg, P)
    return dense(triangle(knots, x, j, deg), j - deg, P)


def basis_f64(knots, x, deg, P, fma=True, mut=None):
    """eval_basis in float64: dense rows"""
    x = np.asarray(x, dtype=np.float64)
    j = spans(knots, x, deg, P, left=mut == "span_left")
    B = dense(triangle(knots, x, j, deg, np.float64, fma, recip=mut == "recip_form"), j - deg, P)
    if mut == "b1_zero_row":
        B[x == knots[-1]] = 0.0
    return B


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------
def factors(c, B, y, mut=None):
    """(F1, F2), n_i x (LG + P + 1): entry e of the record is sum_l F1[l, e] F2[l, e]"""
    B, y = np.asarray(B), np.asarray(y)
    k, P, LG = B.shape[0], c.P, c.LG
    F1, F2 = np.zeros((k, LG + P + 1), dtype=B.dtype), np.zeros((k, LG + P + 1), dtype=B.dtype)
    for d in range(min(c.BW, P - 1) + 1):
        F1[:, d * P:d * P + P - d], F2[:, d * P:d * P + P - d] = B[:, :P - d], B[:, d:]
        if mut == "band_wrap" and d:      # the diagonal runs on past p + d = P - 1, into column (p + d) - P
            F1[:, d * P + P - d:(d + 1) * P], F2[:, d * P + P - d:(d + 1) * P] = B[:, P - d:], B[:, :d]
    F1[:, LG:LG + P], F2[:, LG:LG + P] = B, (np.roll(y, 1) if mut == "s_neighbour_y" else y)[:, None]
    F1[:, LG + P] = F2[:, LG + P] = y
    return F1, F2


def record_ld(c, B, y):
    """(record, sum of absolute terms) of one curve in longdouble, LREC entries"""
    F1, F2 = factors(c, np.asarray(B).astype(LD), np.asarray(y, dtype=np.float64).astype(LD))
    rec, ab = np.zeros(c.LREC, dtype=LD), np.zeros(c.LREC, dtype=LD)
    rec[:F1.shape[1]], ab[:F1.shape[1]] = (F1 * F2).sum(axis=0), np.abs(F1 * F2).sum(axis=0)
    return rec, ab


def record_f64(c, B, y, fma=True, mut=None):
    """one workgroup of k_stats_functional (or one curve of the host loop of bfmmm_create_from_basis) in float64: chunks of 256
    observations, one accumulator per entry, summed in observation order"""
    F1, F2 = factors(c, np.asarray(B, dtype=np.float64), np.asarray(y, dtype=np.float64), mut)
    k, E = F1.shape
    acc = np.zeros(E)
    f32 = mut == "band_f32"
    for c0 in range(0, k, CHUNK):
        obs = list(range(c0, min(k, c0 + CHUNK)))
        if c0 == CHUNK and mut == "drop_256":
            obs = obs[1:]
        if c0 == CHUNK and mut == "dup_256":
            obs = [obs[0]] + obs
        if fma:
            prod = F1[obs].astype(LD) * F2[obs].astype(LD)
            for l in range(len(obs)):
                acc = (prod[l] + acc.astype(LD)).astype(np.float64)
        elif obs:
            acc = np.add.accumulate(np.vstack([acc[None, :], F1[obs] * F2[obs]]), axis=0)[-1]
        if f32:
            acc[:c.LG] = acc[:c.LG].astype(np.float32)
    rec = np.zeros(c.LREC)
    rec[:E] = acc
    if mut == "q7_lost":
        rec[448:] = 0.0
    if mut == "padding" and c.LREC > E:
        rec[E:] = 5e-324
    return rec


def totals_f64(yy, ni, mut=None):
    """k_stats_totals: 256 contiguous per-thread pieces of per = ceil(n / 256) entries, then a sequential sum of 256"""
    n = len(ni)
    per = -(-n // 256)
    sy, sn, sh = np.zeros(256), [0] * 256, [0] * 256
    for tid in range(256):
        hi = min(n, (tid + 1) * per)
        if mut == "totals_skip_partial" and (tid + 1) * per > n:
            continue
        a = 0.0
        for i in range(tid * per, hi):
            a += float(yy[i])
            sn[tid] += int(ni[i])
            sh[tid] += int(ni[i]) // 2
        sy[tid] = a
    s = 0.0
    for q in range(256):
        s += sy[q]
    return dict(YY=s, n_obs_total=sum(sn), half_sum=sum(sn) // 2 if mut == "half_sum_of_total" else sum(sh))


def reference(c):
    """dict(B: list of longdouble dense rows (None: no basis is evaluated), first: list of span - deg, rec, abs (n x LREC), ni,
    n_obs_total, half_sum, sum_yy)"""
    if c.name in _ref:
        return _ref[c.name]
    d = case_data(c)
    r = dict(B=None, first=None)
    if c.kind == "mv":
        Y = d["Y"].astype(LD)
        rec = np.zeros((c.n, c.LREC), dtype=LD)
        rec[:, :c.P], rec[:, c.P:2 * c.P], rec[:, 2 * c.P] = 1, Y, (Y * Y).sum(axis=1)
        r.update(rec=rec, abs=np.abs(rec), ni=np.full(c.n, c.P))
    else:
        if c.kind == "spline":
            r["B"] = [basis_ld(d["knots"], x, c.deg, c.P) for x in d["t"]]
            r["first"] = [spans(d["knots"], x, c.deg, c.P) - c.deg for x in d["t"]]
            rows = r["B"]
        else:
            rows = d["B"]
        both = [record_ld(c, b, y) for b, y in zip(rows, d["y"])]
        r.update(rec=np.array([b[0] for b in both]), abs=np.array([b[1] for b in both]), ni=np.array([len(y) for y in d["y"]]))
    r["n_obs_total"], r["half_sum"] = int(r["ni"].sum()), int((r["ni"] // 2).sum())
    r["sum_yy"] = r["rec"][:, c.LG + c.P].sum()
    _ref[c.name] = r
    return r


def emulate(c, variant="fma", mut=None):
    """what the device would hand to check(): dict(B (spline: list of float64 rows), rec (n x LREC), ni, dims)"""
    d = case_data(c)
    fma = variant == "fma"
    out = dict(B=None)
    if c.kind == "mv":
        Y = d["Y"]
        rec = np.zeros((c.n, c.LREC))
        rec[:, :c.P], rec[:, c.P:2 * c.P] = 1.0, Y
        for i in range(c.n):      # lane 0's loop over p
            a = 0.0
            for p in range(c.P - 1 if (mut == "mv_63" and c.P == 64) else c.P):
                a = float(_fma(Y[i, p:p + 1], Y[i, p:p + 1], np.array([a]))[0]) if fma else a + Y[i, p] * Y[i, p]
            rec[i, 2 * c.P] = a
        ni = np.full(c.n, c.P)
    else:
        if c.kind == "spline":
            out["B"] = rows = [basis_f64(d["knots"], x, c.deg, c.P, fma, mut) for x in d["t"]]
        else:
            rows = d["B"]
        rec = np.array([record_f64(c, b, y, fma, mut) for b, y in zip(rows, d["y"])])
        ni = np.array([len(y) for y in d["y"]])
    tot = totals_f64(rec[:, c.LG + c.P], ni, mut)
    out.update(rec=rec, ni=ni, dims=dict(P=c.P, BW=c.BW, LG=c.LG, LREC=c.LREC, **tot))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def _ratios(err, bound):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)


def check(c, out):
    """every exact check and every bound (module docstring) on what the device (or an emulation) left: out = dict(B: list of n_i x P
    rows or None, rec (n x LREC), ni (n), dims: Sampler.dims()).  Returns dict(worst: {basis, band, s, yy, YY}, fails, judged)"""
    d, ref = case_data(c), reference(c)
    P, LG, LREC, n = c.P, c.LG, c.LREC, len(ref["ni"])
    res = dict(worst=dict(basis=0.0, band=0.0, s=0.0, yy=0.0, YY=0.0), fails=[], judged=set())
    fails, dm = res["fails"], out["dims"]

    def fail(msg):
        if len(fails) < 24:
            fails.append(f"{c.name}: {msg}")

    for nm, want in (("P", P), ("BW", c.BW), ("LG", LG), ("LREC", LREC), ("n_obs_total", ref["n_obs_total"]), ("half_sum", ref["half_sum"])):
        if int(dm[nm]) != want:
            fail(f"dims()['{nm}'] is {dm[nm]}, the reference has {want}")
    rec = np.asarray(out["rec"], dtype=np.float64)
    if rec.shape != (n, LREC):
        fail(f"the record has shape {rec.shape}, not {(n, LREC)}")
        return res
    ni = np.asarray(out["ni"])
    if ni.shape != (n,) or not np.array_equal(ni, ref["ni"]):
        fail(f"ni is {ni[:8]} .., the curves have {ref['ni'][:8]} ..")
    epsB = G_B * c.deg * U if c.kind == "spline" else 0.0
    # ---- the basis rows ----
    if c.kind == "spline":
        b0, b1 = d["bk"]
        cols = np.arange(P)
        for i, (Bd, Br, f, x) in enumerate(zip(out["B"], ref["B"], ref["first"], d["t"])):
            Bd = np.asarray(Bd, dtype=np.float64)
            outside = (cols[None, :] < f[:, None]) | (cols[None, :] > f[:, None] + c.deg)
            if np.any(Bd[outside] != 0.0):
                fail(f"curve {i}: a basis row is non-zero outside its window of {c.deg + 1}")
            nz_d, nz_r = Bd != 0, Br != 0
            fd = np.where(nz_d.any(axis=1), nz_d.argmax(axis=1), -1)
            fr = np.where(nz_r.any(axis=1), nz_r.argmax(axis=1), -1)
            if not np.array_equal(fd, fr):
                l = int(np.argmax(fd != fr))
                fail(f"curve {i}, point {l} (x = {x[l]!r}): the first non-zero basis function is {fd[l]}, the reference's {fr[l]}")
            for xv, col, tag in ((b0, 0, "b0"), (b1, P - 1, "b1")):
                at = x == xv
                if at.any():
                    res["judged"].add(tag)
                    if np.any(Bd[at, col] != 1.0):
                        fail(f"curve {i}: B[x = {tag}][{col}] is {Bd[at, col][0]!r}, not 1.0")
            if np.isin(x, d["ik"]).any():
                res["judged"].add("knot_hit")
            rat = _ratios(np.abs(Bd.astype(LD) - Br), epsB * np.abs(Br) + ETA * (Br != 0))
            res["worst"]["basis"] = max(res["worst"]["basis"], float(rat.max()))
            if not rat.max() <= 1.0:
                l, p = np.unravel_index(int(np.argmax(rat)), rat.shape)
                fail(f"curve {i}, point {l} (x = {x[l]!r}): B[{p}] = {Bd[l, p]!r}, longdouble {float(Br[l, p])!r}, error / bound {rat[l, p]:.3g}")
        res["judged"].add(f"deg{c.deg}")
    # ---- the records ----
    if c.kind == "mv":
        if np.any(rec[:, :P] != 1.0):
            fail("multivariate: one of the first P entries of a record is not 1.0")
        if not np.array_equal(rec[:, P:2 * P], d["Y"]):
            fail("multivariate: entries P .. 2 P - 1 of a record are not y bit for bit")
        if P == 64:
            res["judged"].add("mv_P64")
    for dd in range(c.BW + 1):
        if np.any(rec[:, dd * P + max(P - dd, 0):(dd + 1) * P] != 0.0):
            fail(f"band diagonal {dd}: a slot with p + d >= P is not 0.0")
    if np.any(rec[:, LG + P + 1:] != 0.0):
        fail("the padding behind yy is not 0.0")
    nn = (ref["ni"] + 1)[:, None]
    bound = G_SUM * nn * U * ref["abs"]
    bound[:, :LG] += 2 * epsB * ref["abs"][:, :LG]
    bound[:, LG:LG + P] += epsB * ref["abs"][:, LG:LG + P]
    if c.kind == "spline":      # gradual underflow of the terms (module docstring)
        live = ref["abs"][:, :LG + P] != 0
        bound[:, :LG] += ETA * ref["ni"][:, None] * live[:, :LG]
        bound[:, LG:LG + P] += ETA * np.array([np.abs(y).sum() for y in d["y"]], dtype=LD)[:, None] * live[:, LG:]
    rat = _ratios(np.abs(rec.astype(LD) - ref["rec"]), bound)
    for nm, sl in (("band", slice(0, LG)), ("s", slice(LG, LG + P)), ("yy", slice(LG + P, LG + P + 1))):
        part = rat[:, sl]
        res["worst"][nm] = float(part.max())
        if not part.max() <= 1.0:
            i, e = np.unravel_index(int(np.argmax(part)), part.shape)
            e += sl.start
            fail(f"curve {i} (n_i = {ref['ni'][i]}), {nm} entry e = {e}: {rec[i, e]!r}, longdouble {float(ref['rec'][i, e])!r}, error / bound {part.max():.3g}")
    if c.kind == "spline" and LG + P >= 448:
        res["judged"].add("q7")
    if c.kind == "spline" and ref["ni"].max() > CHUNK:
        res["judged"].add("multi_chunk")
    if c.kind == "basis":
        res["judged"].add(f"basis_BW{c.BW}")
    res["judged"].add(f"totals_n{n}")
    by = G_SUM * (-(-n // 256) + 256 + int(ref["ni"].max()) + 1) * U * ref["sum_yy"]
    r = float(_ratios(abs(LD(float(dm["YY"])) - ref["sum_yy"]), by))
    res["worst"]["YY"] = r
    if not r <= 1.0:
        fail(f"YY is {dm['YY']!r}, longdouble {float(ref['sum_yy'])!r}, error / bound {r:.3g}")
    return res


# name: (case, what must reject it: a key of check()'s worst (error / bound above 1) or "exact" (a message with the word given))
MUTATIONS = {
    "span_left": ("lin_P5_dup", "basis"),
    "b1_zero_row": ("cubic_P12", "exact:B[x = b1]"),
    "recip_form": ("quart_P64", "exact:B[x = b1]"),
    "drop_256": ("cubic_P12", "yy"),
    "dup_256": ("cubic_P12", "yy"),
    "band_wrap": ("cubic_P4", "exact:p + d >= P"),
    "s_neighbour_y": ("cubic_P13", "s"),
    "q7_lost": ("quint_P64", "yy"),
    "padding": ("quart_P11", "exact:padding"),
    "band_f32": ("quad_P10_far", "band"),
    "totals_skip_partial": ("totals_n257", "exact:n_obs_total"),
    "half_sum_of_total": ("totals_n255", "exact:half_sum"),
    "mv_63": ("mv_n3_P64", "yy"),
}
