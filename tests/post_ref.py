"""High-precision restatement of the likelihood-based post-processing pass (csrc/kernels_post.hip: k_post_pointwise, k_post_reduce,
k_post_cpo, k_post_cpo_reduce, k_post_paths), its bounds, two float64 emulations, the host's launch rules and the case list shared by
tests/test_post_ref.py (CPU) and tests/test_gpu_post_steps.py (device).  (Test infrastructure.)  u = 2^-53; every reference value is
np.longdouble, restated from the formulas of the reference (CalculateLikelihood.h:29-70, :172-194, :344-389; PostProcessing.cpp:6797-6810),
not from the kernels' order of operations.  Inputs are in the reference's shapes, those of api._post_input: nu (K, P, T), Phi (K, P, M, T),
Z (n, K, T), chi (n, M, T), sigma (T,) [the variance], X (n, D), eta (P, D, K, T), xi (P, D, M, K, T); covariates none / eta only / eta
and xi; basis rows B_i (n_i, P), the identity among them.

Notation.  Row r = k (M + 1) + mt of draw t is theta_r = nu_k (mt = 0) or phi_k,mt-1, plus sum_d x_id (eta_k or xi_k,mt-1)_d.  With the
basis row B_ij,
    F[t, k, mt, j] = B_ij' theta_r(t),                  Fa = the same with every factor replaced by its absolute value,
    fitted  f_ij(t) = sum_{k: Z_ik != 0} Z_ik ( F[k, 0] + sum_m chi_im F[k, m] ),      Af = its absolute sum (|Z|, |chi|, Fa)
(the reference's Z_ik == 0 skip: a non-finite row of a cluster nobody belongs to does not reach f),
    lt_ij(t) = -( log sqrt(2 pi) + z^2 / 2 + log(sigma^2) / 2 ),  z = (y_ij - f) / sd,  sd = sqrt(sigma^2),      dens = exp(lt),
    ll_i(t) = sum_j lt_ij(t),   llik(t) = sum_i ll_i(t),   mean_pdf_ij / mean_fit_ij = means of dens / f over the kept draws t >= first_kept,
    joint_i = mean over the kept draws of exp(ll_i(t))                                   (bfmmm_post_pointwise_joint).

Bounds, pointwise pass (each G u (sum of absolute terms); G measured below).  depth_f = R + D + W + 3 counts the roundings an
absolute term of f can meet: D covariate products folded into a row, the R-term accumulation of the coefficient vector (a product
with Z, one with chi, an addition), the W-term window dot.
    fitted:    |df| <= depth_f u Af
    lt:        z carries df / sd and three roundings of its own (difference, 1 / sd, product), so z^2 / 2 moves by |z| depth_f u Af / sd
               + 3 u z^2; log sd is two roundings of a value, the sum three additions:
               S_lt = |z| depth_f Af / sd + 4 z^2 + 2 |log sd| + 0.92 + |lt|
    ll_i(t):   sum_j S_lt + ds sum_j |lt|,   ds = ceil(n_i / JW) + log2 min(JW, 64) + JW / 64   (lane-serial, butterfly, wave partials)
    llik(t):   sum_i [ that ] + n sum_i |ll_i(t)|                                          (k_post_reduce: curves in order)
    mean_pdf:  RELATIVE in each term: exp turns the absolute error of lt -- u S_lt, which carries |lt| u -- into a relative one, + 2 u for
               exp itself:  sum_kept dens (S_lt + 2) / kept + dt mean_pdf + 2^-1022 / u,
               dt = min(kept, (tchunk / G) NG) + GT + NCH + 1 the additions a kept draw's term meets (its draw lane's register sum, the
               lanes, the chunks, the division); 2^-1022 the underflow threshold (a density below it may be flushed)
    mean_fit:  (depth_f + dt) sum_kept Af / kept
    joint:     sum_kept exp(ll) (bound of ll / u + 2) / kept + (kept + 1) joint + 2^-1022 / u       (k_post_reduce: draws in order)

CPO pass (no Z == 0 skip: calcLikelihoodCPO has none).  c = sum_k Z_ik theta_k,0, v_m = sum_k Z_ik theta_k,m, r = y_i - B_i c, U = B_i [v_m]:
    ll_i(t) = -(n_i / 2) log 2 pi - ld / 2 - quad / 2,   ld = (n_i - M) log sigma^2 + 2 sum_m log L_mm,   quad = (r'r - w'w) / sigma^2,
    A = sigma^2 I + U'U = L L',  w = L^-1 U'r.
With x = A^-1 U'r, first-order perturbation gives d(w'w) = -x' dA x + 2 x' d(U'r) and d log det A = tr(A^-1 dA); every entry of r, U, U'r, U'U
is a sum whose absolute terms are ra = |y| + |B| |c|, AU = |B| |v|, so with Aa = AU'AU + sigma^2 I
    S_quad = ( ra'ra + |x|' Aa |x| + 2 |x|' AU'ra ) / sigma^2 + sum_ab |A^-1|_ab Aa_ab
bounds r'r AND w'w by their absolute terms (the cancellation in r'r - w'w is bounded, not ignored) and the log-determinant's movement;
    S_fix = |(n_i - M) log sigma^2| + sum_m |2 log L_mm| + (n_i / 2) log 2 pi + |ll|,
    bound = G_CPO u (depth_c S_quad + 4 S_fix),   depth_c = K (D + 1) + W + NIP / 4 + M + 8
(coefficient sums, window dot, a segment's serial sum and sum4, the Cholesky's M-term eliminations, the closing arithmetic).
log CPO_i = log L + min_t ll - log sum_t exp(min - ll_t) over the L kept draws (k_post_cpo_reduce): a softmin, so a matrix error b_t moves
it by at most sum_t w_t b_t, w_t = exp(min - ll_t) / sum; against the device's OWN matrix it is judged to a few ulp,
    u ( 4 (|log L| + |min| + |log sum|) + sum_t w_t (2 |min - ll_t| + 4) + L ).

Sample paths (k_post_paths).  mean_only = sum_{k: Z != 0} Z_ik F[k, 0], mean = f; depth_p = R + D + W + 3:  G_PATH depth_p u (Af0 | Af).  The
noise is sqrt(sigma^2(t)) times the oracle's keyed normal, orc_rnorm with UPD_SAMPLE_PATH = 41, iteration = draw index, index = global
observation index, under the AS241 allowance of curve_update_ref.check_chi_norm: sd (32 |z| + 4) u, + 2 u |noise| for the square root
and the product, + u |path| for the closing addition.  paths - noise is held to the mean's bound plus that allowance; at M = 0 the
device's mean_only is the path's own mean, so paths - mean_only is the noise alone and is held to the allowance alone.

Constants.  Largest error / (bound at G = 1) of two float64 emulations over CASES and 2400 random curves (random_cases()) -- `kern`: the
kernels' order of operations (window dot over W, 1 / sd and log sd, lane-serial sums, the butterfly over observation lanes and the wave
partials, per-draw-lane accumulators, chunk sums in chunk order, four segments and sum4, the Cholesky's elimination order); `plain`: the
obvious numpy form (einsum, matrix products, pairwise sums, numpy's Cholesky) -- measured on the CPU by
    pytest -s tests/test_post_ref.py::test_emulations_pass_and_constants_hold
never from a device run:

    llik:      kern 0.24  (id1),       plain 0.153 (id1)        ->  G_LLIK  = 0.96
    mean_pdf:  kern 0.2   (rand_44),   plain 0.194 (t1)         ->  G_PDF   = 0.8
    mean_fit:  kern 0.125 (rand_100),  plain 0.125 (rand_100)   ->  G_FIT   = 0.5
    joint:     kern 0.126 (rand_177),  plain 0.243 (t1)         ->  G_JOINT = 0.972
    cpo ll:    kern 0.109 (id1),       plain 0.11  (id1)        ->  G_CPO   = 0.44
    paths:     kern 0.377 (long),      plain 0.31  (rand_135)   ->  G_PATH  = 1.51

Margin: the device gets 4 x the larger measured ratio, the factor scalar_jobs_ref uses.  Reasons: the compiler contracts
a * b + c into one rounding where the emulations take two (at most the emulations' own error again, a factor 2); ocml's exp, log and
sqrt are good to 1-2 ulp where numpy's libm is 0.5-1 (the S_lt, S_fix and `+ 2` terms double at worst); a different but equally deep
summation tree changes which terms meet, not how many (covered by the same factor 2).  4 covers 2 x 2 without opening room for a wrong
term: every mutation of test_post_ref.py misses its bound by orders of magnitude at this margin.

geometry() is a COPY of the launch rules of post_impl and the kernels' first lines (kernels_post.hip) and must be kept in step with
them; nothing on the device reports these numbers.
"""
import functools
import math
import zlib

import numpy as np

U, LD = 2.0 ** -53, np.longdouble
TINY = 2.0 ** -1022
LOG_SQRT_2PI = LD("0.918938533204672741780329736405617639861")
LOG_2PI = 2 * LOG_SQRT_2PI
UPD_SAMPLE_PATH = 41
# launch constants of kernels_post.hip
NJ, GMAX, BL_MAX, WMAX, NG, KMAXP, NB = 4, 32, 1536, 26, 8, 16, 12
CPO_MREG, CPO_MMAX, CPO_GMAX, CPO_LDS_BUDGET = 8, 16, 16, 17000

# measured by tests/test_post_ref.py::test_emulations_pass_and_constants_hold (largest error / bound at G = 1)
MEASURED = {"llik": {"kern": 0.24, "plain": 0.153}, "mean_pdf": {"kern": 0.2, "plain": 0.194}, "mean_fit": {"kern": 0.125, "plain": 0.125},
            "joint": {"kern": 0.126, "plain": 0.243}, "cpo_ll": {"kern": 0.109, "plain": 0.11}, "paths": {"kern": 0.377, "plain": 0.31}}
MARGIN = 4.0
G_LLIK, G_PDF, G_FIT, G_JOINT, G_CPO, G_PATH = 0.96, 0.8, 0.5, 0.972, 0.44, 1.51
G = {"llik": G_LLIK, "mean_pdf": G_PDF, "mean_fit": G_FIT, "joint": G_JOINT, "cpo_ll": G_CPO, "paths": G_PATH, "mean_only": G_PATH}


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """lens: observations per curve; cov: "none" | "eta" | "etaxi"; basis: "cubic" (P - 4 internal knots on [0, 1], every curve of two
    or more observations touches both ends), "tensor" (quadratic x cubic Bernstein rows, P = 12, all columns non-zero), "identity"
    (every curve has P observations); zskip: one cluster has exact zero membership for every curve at the odd draws, where its rows
    (and covariate rows) are NaN / inf; passes: which kernels take the case"""
    def __init__(self, name, lens, K, M, P, T, first_kept=0, D=0, cov="none", basis="cubic", zskip=False, passes=("pw", "cpo", "paths")):
        self.name, self.lens, self.K, self.M, self.P, self.T, self.first_kept = name, list(lens), K, M, P, T, first_kept
        self.D, self.cov, self.basis, self.zskip, self.passes = D, cov, basis, zskip, tuple(passes)
        self.n, self.R = len(self.lens), K * (M + 1)

    def __repr__(self):
        return self.name


CASES = [
    # every JW 1 .. 256, G 8 / 16 / 32, long and short curves in one call, first_kept inside a tile, kept = 28 not a multiple of Gc = 16;
    # P = 9 is odd, so the coefficient tile has no pad column between two draws (the unclamped-window mutation reads the next draw)
    Case("mix_cubic", [1, 2, 3, 4, 5, 13, 27, 63, 64, 65, 128, 129], K=3, M=2, P=9, T=33, first_kept=5),
    # 1024 observations, both sides of the staging limit n_i (W | 1) = 1536, Gc = 8 from the budget at small M, eta alone
    Case("long", [256, 257, 1024, 1, 307, 308], K=2, M=1, P=8, T=33, first_kept=17, D=1, cov="eta"),
    # K + M = 24 on a curve longer than 256, R = 136 (twelve row batches, the last of four rows), the LDS system at M = 16
    Case("k8m16", [300, 5, 64], K=8, M=16, P=8, T=5, first_kept=1),
    # Gc = 1: M = 16, P = 8, longest curve 936; K = 1
    Case("gc1", [936, 3], K=1, M=16, P=8, T=3),
    # R = 12: exactly one row batch; D = 8 with eta and xi; first_kept = T - 1
    Case("r12_d8", [6, 70, 2], K=4, M=2, P=8, T=33, first_kept=32, D=8, cov="etaxi"),
    # R = 13: one row into the second batch; M = 0 (pointwise and paths only)
    Case("r13_m0", [5, 33], K=13, M=0, P=8, T=4, passes=("pw", "paths")),
    # R = 24: two full batches; M = 1; D = 1 with eta and xi
    Case("r24", [7, 129], K=12, M=1, P=8, T=6, first_kept=2, D=1, cov="etaxi"),
    # K = 16 with M = 8: the largest register system of the CPO pass, and K + M = 24 again
    Case("k16m8", [65, 4, 1], K=16, M=8, P=8, T=4),
    # M = 9: the smallest LDS system
    Case("m9", [64, 7, 129], K=2, M=9, P=8, T=17, D=1, cov="etaxi"),
    Case("t1", [2, 33], K=2, M=1, P=8, T=1),
    # T = 65: three chunks of 32, a ragged last tile; kept = 62; D = 8 with eta alone
    Case("t65", [5, 70, 1], K=2, M=2, P=8, T=65, first_kept=3, D=8, cov="eta"),
    Case("t33_fk0", [9, 17], K=2, M=2, P=8, T=33),
    # the wide window of a tensor-product basis: W = 12, never staged at these lengths
    Case("tensor", [129, 257], K=2, M=2, P=12, T=9, first_kept=1, basis="tensor"),
    Case("id1", [1] * 5, K=2, M=1, P=1, T=33, basis="identity"),
    Case("id7", [7] * 4, K=3, M=2, P=7, T=12, first_kept=4, basis="identity"),
    Case("id64", [64] * 4, K=2, M=3, P=64, T=6, D=1, cov="eta", basis="identity"),
    # exact zeros in Z with non-finite rows in the skipped cluster (no CPO: that pass has no skip)
    Case("zskip", [5, 64, 130], K=3, M=2, P=8, T=10, first_kept=2, D=1, cov="etaxi", zskip=True, passes=("pw", "paths")),
]
CASE = {c.name: c for c in CASES}
# refused by message: name -> (case, pass, message)
REFUSED = [
    (Case("obs1025", [1025, 2], K=2, M=1, P=8, T=2), "pw", "at most 1024 observations per curve"),
    (Case("kplusm25", [5, 9], K=9, M=16, P=8, T=2), "pw", "K \\+ M <= 24"),
    (Case("p65", [65, 65], K=2, M=1, P=65, T=2, basis="identity"), "pw", "P <= 64"),
    (Case("d9", [5, 9], K=2, M=1, P=8, T=2, D=9, cov="eta"), "pw", "D <= 8"),
    (Case("cpo_m0", [5, 9], K=2, M=0, P=8, T=2), "cpo", "1 <= M <= 16"),
    (Case("cpo_m17", [5, 9], K=2, M=17, P=8, T=2), "cpo", "1 <= M <= 16"),
    (Case("gc0", [937, 3], K=1, M=16, P=8, T=2), "cpo", "exceed the on-chip tile"),       # padded length 940
]


def random_cases(count=300, n=8):
    """count x n random curves: the population the constants are measured over besides CASES"""
    rng = np.random.default_rng(20240229)
    out = []
    for s in range(count):
        D = int(rng.integers(0, 3))
        out.append(Case(f"rand_{s}", rng.integers(1, 81, size=n).tolist(), K=int(rng.integers(1, 5)), M=int(rng.integers(1, 5)), P=8,
                        T=6, first_kept=int(rng.integers(0, 3)), D=D, cov=("none" if D == 0 else ("eta", "etaxi")[s % 2])))
    return out


def bspline_rows(x, P, deg=3):
    """B-spline basis rows on [0, 1] with P - deg - 1 equally spaced internal knots (Cox-de Boor; exact zeros outside a row's support)"""
    x = np.asarray(x, dtype=np.float64)
    ik = np.linspace(0.0, 1.0, P - deg + 1)[1:-1]
    t = np.concatenate([np.zeros(deg + 1), ik, np.ones(deg + 1)])
    nb = len(t) - 1
    N = np.zeros((len(x), nb))
    for j in range(nb):
        if t[j] < t[j + 1]:
            N[:, j] = (x >= t[j]) & ((x < t[j + 1]) | ((x == 1.0) & (t[j + 1] == 1.0)))
    for d in range(1, deg + 1):
        Nn = np.zeros((len(x), nb - d))
        for j in range(nb - d):
            a = (x - t[j]) / (t[j + d] - t[j]) * N[:, j] if t[j + d] > t[j] else 0.0
            b = (t[j + d + 1] - x) / (t[j + d + 1] - t[j + 1]) * N[:, j + 1] if t[j + d + 1] > t[j + 1] else 0.0
            Nn[:, j] = a + b
        N = Nn
    return N


@functools.lru_cache(maxsize=None)
def _case_data(name):
    c = CASE.get(name) or {q[0].name: q[0] for q in REFUSED}.get(name) or {q.name: q for q in random_cases()}[name]
    return make_data(c)


def case_data(c):
    """the case's inputs (cached, never modified): Y, B lists, arrays in the reference's shapes"""
    return _case_data(c.name)


def make_data(c):
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    n, K, M, P, T, D = c.n, c.K, c.M, c.P, c.T, c.D
    B = []
    for i, ni in enumerate(c.lens):
        if c.basis == "identity":
            B.append(np.eye(P))
        elif c.basis == "tensor":
            x1, x2 = rng.uniform(0.05, 0.95, size=ni), rng.uniform(0.05, 0.95, size=ni)
            b1, b2 = bspline_rows(x1, 3, 2), bspline_rows(x2, 4, 3)
            B.append(np.ascontiguousarray((b1[:, :, None] * b2[:, None, :]).reshape(ni, 12)))
        else:
            x = np.sort(rng.uniform(0, 1, size=ni))
            if ni >= 2:
                x[0], x[-1] = 0.0, 1.0
            else:
                x[0] = float(i % 2)
            B.append(bspline_rows(x, P))
    nu = rng.standard_normal((K, P, 1)) + 0.1 * rng.standard_normal((K, P, T))
    Phi = 0.3 * rng.standard_normal((K, P, M, T))
    Z = rng.dirichlet(np.full(K, 0.7), size=(n, T)).transpose(0, 2, 1) if K > 1 else np.ones((n, 1, T))
    if K > 1 and n > 3:
        Z[3] = 0.0
        Z[3, 0] = 1.0                                   # all weight on one cluster: exact zeros, finite rows
    chi = rng.standard_normal((n, M, T))
    sigma = rng.uniform(0.3, 0.9, size=T)               # away from 1: log sigma^2 must count
    sigma[::2] = rng.uniform(1.2, 1.8, size=len(sigma[::2]))
    d = dict(B=B, nu=nu, Phi=Phi, Z=Z, chi=chi, sigma=sigma, X=None, eta=None, xi=None)
    if D:
        d["X"] = rng.standard_normal((n, D))
        d["eta"] = 0.3 * rng.standard_normal((P, D, K, T))
        if c.cov == "etaxi":
            d["xi"] = 0.1 * rng.standard_normal((P, D, M, K, T))
    if c.zskip:
        Z[:, 1, 1::2] = 0.0
        Z[:, 0, 1::2] = 1.0 - Z[:, 2, 1::2]
    # observations: the first draw's mean function plus noise, so that residuals stay of the order of sd under every draw
    d["Y"] = [B[i] @ (Z[i, :, 0] @ nu[:, :, 0]) + 0.7 * rng.standard_normal(c.lens[i]) for i in range(n)]
    if c.zskip:                                         # after Y: the skipped cluster's rows are not numbers at the odd draws
        nu[1, :, 1::2], Phi[1, :, :, 1::2] = np.nan, np.inf
        d["eta"][:, :, 1, 1::2], d["xi"][:, :, :, 1, 1::2] = -np.inf, np.nan
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def rows(d):
    """th (T, K, M + 1, P) and thx (T, K, M + 1, D, P): the draw's parameter rows and their covariate rows, as post_impl lays them out"""
    nu, Phi = d["nu"], d["Phi"]
    K, P, T = nu.shape
    M = Phi.shape[2]
    th = np.empty((T, K, M + 1, P))
    th[:, :, 0, :] = nu.transpose(2, 0, 1)
    th[:, :, 1:, :] = Phi.transpose(3, 0, 2, 1)
    D = 0 if d["X"] is None else d["X"].shape[1]
    thx = np.zeros((T, K, M + 1, D, P))
    if D and d["eta"] is not None:
        thx[:, :, 0] = d["eta"].transpose(3, 2, 1, 0)
    if D and d["xi"] is not None:
        thx[:, :, 1:] = d["xi"].transpose(4, 3, 2, 1, 0)
    return th, thx


def windows(B, P, clamp=True):
    """post_impl's window rule: W = the widest span of non-zero columns of any row, every row's first column clamped to P - W; returns
    W, first (n_obs,), Bc (n_obs, W).  clamp=False is the mutation: the raw first column, the window read on into the next row."""
    Bm = np.concatenate(B, axis=0)
    nz = Bm != 0.0
    any_ = nz.any(axis=1)
    f = np.where(any_, nz.argmax(axis=1), 0)
    l = np.where(any_, P - 1 - nz[:, ::-1].argmax(axis=1), 0)
    W = max(1, int((l - f + 1)[any_].max()) if any_.any() else 1)
    st = np.minimum(f, P - W) if clamp else f
    flat = np.concatenate([Bm.reshape(-1), np.zeros(W)])
    Bc = flat[(np.arange(len(Bm)) * P + st)[:, None] + np.arange(W)[None, :]]
    return W, st.astype(np.int64), Bc


# ---------------------------------------------------------------------------------------------------------------------
# the host's launch rules (a copy of post_impl / the kernels' first lines: keep in step)
# ---------------------------------------------------------------------------------------------------------------------
def geometry(lens, K, M, P, D, T, first_kept, W):
    n, R = len(lens), K * (M + 1)
    pw = []
    for ni in lens:
        JW = 1
        while JW < min(ni, 256):
            JW <<= 1
        GT = min(256 // JW, GMAX // NG)
        pw.append(dict(ni=ni, JW=JW, GT=GT, G=GT * NG, staged=ni * (W | 1) <= BL_MAX))
    tchunk = T
    while n * (-(-T // tchunk)) < 2048 and tchunk > GMAX:
        tchunk = (tchunk + 1) // 2
    tchunk = -(-tchunk // GMAX) * GMAX
    out = dict(pw=pw, tchunk=tchunk, NCH=-(-T // tchunk), batches=-(-R // NB), R=R, kept=T - first_kept)
    if 1 <= M <= CPO_MMAX and K <= KMAXP:
        NIPX = (max(lens) + 3) & ~3
        M1, NQ = M + 1, M * (M + 1) // 2 + M + 1
        per_draw = M1 * (P | 1) + M1 * NIPX + NQ * 4 + (M * M + M if M > CPO_MREG else 0)
        Gc = min(CPO_GMAX, CPO_LDS_BUDGET // per_draw)
        out["cpo"] = dict(NIPX=NIPX, per_draw=per_draw, Gc=Gc, gc_class="cap" if CPO_LDS_BUDGET // per_draw >= CPO_GMAX else ("1" if Gc == 1 else ("refused" if Gc < 1 else "budget")),
                          NIP=[(ni + 3) & ~3 for ni in lens], staged=[ni * (W | 1) <= BL_MAX for ni in lens], home="reg" if M <= CPO_MREG else "lds")
    return out


def case_geometry(c):
    W, _, _ = windows(case_data(c)["B"], c.P)
    return geometry(c.lens, c.K, c.M, c.P, c.D, c.T, c.first_kept, W)


def classes(c):
    """the geometry classes a case visits, per pass: {pass: set of labels}"""
    g = case_geometry(c)
    out = {}
    if "pw" in c.passes:
        s = set()
        for q in g["pw"]:
            s |= {f"JW={q['JW']}", f"G={q['G']}", "staged" if q["staged"] else "unstaged"}
        s.add("NCH=1" if g["NCH"] == 1 else "NCH>1")
        out["pw"] = s
    if "cpo" in c.passes:
        q = g["cpo"]
        s = {f"home={q['home']}", f"Gc={q['gc_class']}"} | {"staged" if v else "unstaged" for v in q["staged"]}
        if min(q["NIP"]) < q["NIPX"]:
            s.add("NIP<NIPX")
        out["cpo"] = s
    return out


REQUIRED_CLASSES = {"pw": {f"JW={1 << b}" for b in range(9)} | {"G=8", "G=16", "G=32", "staged", "unstaged", "NCH=1", "NCH>1"},
                    "cpo": {"home=reg", "home=lds", "Gc=1", "Gc=budget", "Gc=cap", "NIP<NIPX", "staged", "unstaged"}}


# ---------------------------------------------------------------------------------------------------------------------
# long-double restatement
# ---------------------------------------------------------------------------------------------------------------------
def _F(d, i, th, thx):
    """F and Fa (T, K, M + 1, n_i) of curve i in long double; a row that is not finite stays so in F only"""
    Bi = d["B"][i].astype(LD)
    co = th.astype(LD)
    ca = np.abs(co)
    if thx.shape[3]:
        x = d["X"][i].astype(LD)
        with np.errstate(invalid="ignore"):
            co = co + np.einsum("tkmdp,d->tkmp", thx.astype(LD), x)
            ca = ca + np.einsum("tkmdp,d->tkmp", np.abs(thx.astype(LD)), np.abs(x))
    with np.errstate(invalid="ignore"):
        return np.matmul(co, Bi.T), np.matmul(ca, np.abs(Bi).T)


def _fitted(d, i, F, Fa):
    """f, Af (all rows), mo, Af0 (mt = 0 rows only), each (T, n_i), with the Z == 0 skip"""
    z = d["Z"][i].T.astype(LD)                                    # (T, K)
    w = np.concatenate([np.ones((z.shape[0], 1), dtype=LD), d["chi"][i].T.astype(LD)], axis=1)      # (T, M + 1)
    on = (z != 0)[:, :, None, None]
    Fz, Faz = np.where(on, F, LD(0)), np.where(on, Fa, LD(0))
    f = np.einsum("tk,tm,tkmj->tj", z, w, Fz)
    Af = np.einsum("tk,tm,tkmj->tj", np.abs(z), np.abs(w), Faz)
    mo = np.einsum("tk,tkj->tj", z, Fz[:, :, 0])
    Af0 = np.einsum("tk,tkj->tj", np.abs(z), Faz[:, :, 0])
    return f, Af, mo, Af0


_LD_CACHE = {}


def ld_pointwise(c, d=None):
    """the pointwise pass and the sample paths' means in long double with their bounds at G = 1 (u is inside, G_* is not); the result of
    a case's own data is kept and must not be modified"""
    if d is None:
        if ("pw", c.name) not in _LD_CACHE:
            _LD_CACHE[("pw", c.name)] = ld_pointwise(c, case_data(c))
        return _LD_CACHE[("pw", c.name)]
    th, thx = rows(d)
    W, _, _ = windows(d["B"], c.P)
    g = geometry(c.lens, c.K, c.M, c.P, c.D, c.T, c.first_kept, W)
    fk, T, kept = c.first_kept, c.T, c.T - c.first_kept
    depth_f = c.R + c.D + W + 3
    sig = d["sigma"].astype(LD)
    sd, lsd = np.sqrt(sig)[:, None], (np.log(sig) / 2)[:, None]
    out = dict(fit=[], mo=[], b_fit_e=[], b_mo_e=[], lt=[], mean_pdf=[], mean_fit=[], b_pdf=[], b_fit=[], ll=np.zeros((c.n, T), dtype=LD),
               b_ll=np.zeros((c.n, T), dtype=LD), joint=np.zeros(c.n, dtype=LD), b_joint=np.zeros(c.n, dtype=LD))
    for i in range(c.n):
        q = g["pw"][i]
        F, Fa = _F(d, i, th, thx)
        f, Af, mo, Af0 = _fitted(d, i, F, Fa)
        y = d["Y"][i].astype(LD)[None, :]
        z = (y - f) / sd
        lt = -(LOG_SQRT_2PI + z * z / 2 + lsd)
        S = np.abs(z) * depth_f * Af / sd + 4 * z * z + 2 * np.abs(lsd) + LD(0.92) + np.abs(lt)
        ds = -(-q["ni"] // q["JW"]) + math.log2(min(q["JW"], 64)) + q["JW"] / 64
        out["ll"][i] = lt.sum(axis=1)
        out["b_ll"][i] = U * (S.sum(axis=1) + ds * np.abs(lt).sum(axis=1))
        dens = np.exp(lt)
        dt = min(kept, (g["tchunk"] // q["G"]) * NG) + q["GT"] + g["NCH"] + 1
        mp = dens[fk:].sum(axis=0) / kept
        out["mean_pdf"].append(mp)
        out["b_pdf"].append(U * ((dens[fk:] * (S[fk:] + 2)).sum(axis=0) / kept + dt * mp) + TINY)
        out["mean_fit"].append(f[fk:].sum(axis=0) / kept)
        out["b_fit"].append(U * (depth_f + dt) * Af[fk:].sum(axis=0) / kept)
        e = np.exp(out["ll"][i][fk:])
        out["joint"][i] = e.sum() / kept
        out["b_joint"][i] = (e * (out["b_ll"][i][fk:] + 2 * U)).sum() / kept + U * (kept + 1) * out["joint"][i] + TINY
        out["fit"].append(f); out["mo"].append(mo); out["lt"].append(lt)
        out["b_fit_e"].append(U * depth_f * Af); out["b_mo_e"].append(U * depth_f * Af0)
    out["llik"] = out["ll"].sum(axis=0)
    out["b_llik"] = out["b_ll"].sum(axis=0) + U * c.n * np.abs(out["ll"]).sum(axis=0)
    return out


def _chol_ld(A):
    """Cholesky of a stack of SPD matrices (T, m, m) in the array's own precision, column by column"""
    m = A.shape[-1]
    L = np.zeros_like(A)
    for c_ in range(m):
        s = A[:, c_, c_] - (L[:, c_, :c_] ** 2).sum(axis=1)
        L[:, c_, c_] = np.sqrt(s)
        if c_ + 1 < m:
            L[:, c_ + 1:, c_] = (A[:, c_ + 1:, c_] - np.einsum("trk,tk->tr", L[:, c_ + 1:, :c_], L[:, c_, :c_])) / L[:, c_, c_][:, None]
    return L


def _fsolve_ld(L, b):
    """L x = b for stacks: L (T, m, m) lower, b (T, m, q)"""
    x = np.zeros_like(b)
    for r in range(L.shape[-1]):
        x[:, r] = (b[:, r] - np.einsum("tk,tkq->tq", L[:, r, :r], x[:, :r])) / L[:, r, r][:, None]
    return x


def _cpo_parts(c, d, i, th, thx):
    """r (T, n_i), Um (T, n_i, M) and their absolute sums ra, AU in long double (no Z == 0 skip)"""
    F, Fa = _F(d, i, th, thx)
    z = d["Z"][i].T.astype(LD)
    cv, ca = np.einsum("tk,tkmj->tmj", z, F), np.einsum("tk,tkmj->tmj", np.abs(z), Fa)
    y = d["Y"][i].astype(LD)[None, :]
    return y - cv[:, 0], cv[:, 1:].transpose(0, 2, 1), np.abs(y) + ca[:, 0], ca[:, 1:].transpose(0, 2, 1)


def ld_cpo(c, d=None, dense=False):
    """the matrix ll (n, T) of marginal log-densities (rank-M form, or the reference's dense n_i x n_i form), its bound b_ll at G = 1,
    log CPO and the bound the matrix's bound carries into it"""
    if d is None:
        if ("cpo", dense, c.name) not in _LD_CACHE:
            _LD_CACHE[("cpo", dense, c.name)] = ld_cpo(c, case_data(c), dense)
        return _LD_CACHE[("cpo", dense, c.name)]
    th, thx = rows(d)
    W, _, _ = windows(d["B"], c.P)
    M, T, fk = c.M, c.T, c.first_kept
    sig = d["sigma"].astype(LD)
    ll, b = np.zeros((c.n, T), dtype=LD), np.zeros((c.n, T), dtype=LD)
    for i, ni in enumerate(c.lens):
        r, Um, ra, AU = _cpo_parts(c, d, i, th, thx)
        if dense:
            Cov = np.einsum("tjm,tlm->tjl", Um, Um) + sig[:, None, None] * np.eye(ni, dtype=LD)[None]
            L = _chol_ld(Cov)
            w = _fsolve_ld(L, r[:, :, None])[:, :, 0]
            ll[i] = -(LD(ni) / 2) * LOG_2PI - np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1) - (w * w).sum(axis=1) / 2
            continue
        I = np.eye(M, dtype=LD)[None]
        A = np.einsum("tjm,tjl->tml", Um, Um) + sig[:, None, None] * I
        bb = np.einsum("tjm,tj->tm", Um, r)
        L = _chol_ld(A)
        w = _fsolve_ld(L, bb[:, :, None])[:, :, 0]
        Li = _fsolve_ld(L, np.broadcast_to(I, A.shape).copy())
        Ainv = np.einsum("tkm,tkl->tml", Li, Li)
        xa = np.abs(np.einsum("tml,tl->tm", Ainv, bb))
        Aa = np.einsum("tjm,tjl->tml", AU, AU) + sig[:, None, None] * I
        rr, ww = (r * r).sum(axis=1), (w * w).sum(axis=1)
        logL = np.log(np.diagonal(L, axis1=1, axis2=2))
        ld_ = (ni - M) * np.log(sig) + 2 * logL.sum(axis=1)
        ll[i] = -(LD(ni) / 2) * LOG_2PI - ld_ / 2 - (rr - ww) / sig / 2
        S_quad = ((ra * ra).sum(axis=1) + np.einsum("tm,tml,tl->t", xa, Aa, xa) + 2 * np.einsum("tm,tjm,tj->t", xa, AU, ra)) / sig + (np.abs(Ainv) * Aa).sum(axis=(1, 2))
        S_fix = np.abs((ni - M) * np.log(sig)) + 2 * np.abs(logL).sum(axis=1) + (LD(ni) / 2) * LOG_2PI + np.abs(ll[i])
        depth_c = c.K * (c.D + 1) + W + ((ni + 3) & ~3) // 4 + M + 8
        b[i] = U * (depth_c * S_quad + 4 * S_fix)
    out = dict(ll=ll, b_ll=b)
    out["cpo"], out["b_cpo_carry"], out["b_cpo_own"] = ld_harmonic(ll[:, fk:], b[:, fk:])
    return out


def ld_harmonic(rows_, b=None):
    """log CPO of every row of a matrix (n, kept) of log-densities in long double: the value, the bound carried from the matrix's bound
    b (at G = 1; zero without one) and the few-ulp bound of the reduction's own arithmetic"""
    rows_ = np.asarray(rows_).astype(LD)
    kept = rows_.shape[1]
    mn = rows_.min(axis=1)
    e = np.exp(mn[:, None] - rows_)
    ph = e.sum(axis=1)
    cpo = np.log(LD(kept)) + mn - np.log(ph)
    wgt = e / ph[:, None]
    carry = (wgt * b).sum(axis=1) if b is not None else np.zeros_like(cpo)
    own = U * (4 * (abs(math.log(kept)) + np.abs(mn) + np.abs(np.log(ph))) + (wgt * (2 * np.abs(mn[:, None] - rows_) + 4)).sum(axis=1) + kept)
    return cpo, carry, own


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulations.  mut: a named mutation of `kern` (tests/test_post_ref.py::test_mutations_are_caught)
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("zskip", "ni_for_ni_minus_M", "segment", "pad", "first_kept", "tile_last", "clamp", "chol_sigma", "chunk0", "logsd")


def _window_dot(Bc, st, cvec, W, stale=None):
    """sum_w Bc[j, w] cvec[..., st_j + w] in the order of w; cvec (..., P), read on past P into `stale` (the unclamped mutation)"""
    if stale is not None:
        cvec = np.concatenate([cvec, stale], axis=-1)
    f = np.zeros(cvec.shape[:-1] + (len(st),))
    for w in range(W):
        f = f + Bc[:, w] * cvec[..., st + w]
    return f


def _lane_sum(lt, ni, JW):
    """a curve's log-likelihood per draw as k_post_pointwise adds it: lane jl takes j = jl, jl + JW, ... in order, the lanes of a wave
    meet by the xor butterfly (lane 0's tree: halves folded), waves of a draw lane in order"""
    nrow = -(-ni // JW)
    a = np.zeros((lt.shape[0], nrow * JW))
    a[:, :ni] = lt
    a = a.reshape(-1, nrow, JW)
    lane = np.zeros((lt.shape[0], JW))
    for r in range(nrow):
        lane = lane + a[:, r]
    wl = min(JW, 64)
    wv = lane.reshape(-1, JW // wl, wl)
    while wl > 1:
        wl //= 2
        wv = wv[:, :, :wl] + wv[:, :, wl:2 * wl]
    s = np.zeros(lt.shape[0])
    if JW <= 64:
        return wv[:, 0, 0]
    for v in range(wv.shape[1]):
        s = s + wv[:, v, 0]
    return s


def kern_pointwise(c, d=None, mut=None):
    d = d or case_data(c)
    th, thx = rows(d)
    T, K, M, P, D, R, M1, fk = c.T, c.K, c.M, c.P, c.D, c.R, c.M + 1, c.first_kept
    th, thx = th.reshape(T, R, P), thx.reshape(T, R, D, P)
    W, st_all, Bc_all = windows(d["B"], P, clamp=mut != "clamp")
    g = geometry(c.lens, K, M, P, D, T, fk, W)
    tchunk, NCH, kept = g["tchunk"], g["NCH"], T - fk
    off = np.concatenate([[0], np.cumsum(c.lens)])
    llpart = np.zeros((c.n, T))
    mean_pdf, mean_fit = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for i, ni in enumerate(c.lens):
            q = g["pw"][i]
            v = th.copy()
            for dd in range(D):
                v = v + d["X"][i, dd] * thx[:, :, dd, :]
            zt, ct = d["Z"][i].T, d["chi"][i].T
            cv = np.zeros((T, P))
            for r in range(R):
                k, mt = divmod(r, M1)
                zk = zt[:, k][:, None]
                x = v[:, r, :] if mut == "zskip" else np.where(zk != 0.0, v[:, r, :], 0.0)
                cv = cv + zk * (x if mt == 0 else ct[:, mt - 1][:, None] * x)
            sig = d["sigma"].copy()
            if mut == "tile_last":      # the last slot of a full tile takes the draw before it
                for t in range(T):
                    t_lo = (t // tchunk) * tchunk
                    if (t - t_lo) % q["G"] == q["G"] - 1:
                        cv[t], sig[t] = cv[t - 1], sig[t - 1]
            stale = None
            if mut == "clamp":          # past column P: the tile's pad column (unwritten; zero here) when P is even, then the next draw
                nxt = np.concatenate([cv[1:], np.zeros((1, P))], axis=0)
                stale = nxt if (P | 1) == P else np.concatenate([np.zeros((T, 1)), nxt], axis=1)
            st, Bc = st_all[off[i]:off[i + 1]], Bc_all[off[i]:off[i + 1]]
            f = _window_dot(Bc, st, cv, W, stale)
            sdv = np.sqrt(sig)
            isd, lsd = (1.0 / sdv)[:, None], (np.log(sig) if mut == "logsd" else np.log(sdv))[:, None]
            z = (d["Y"][i][None, :] - f) * isd
            lt = -(0.91893853320467274178 + 0.5 * z * z + lsd)
            llpart[i] = _lane_sum(lt, ni, q["JW"])
            dens = np.exp(lt)
            accP, accF = np.zeros((NCH, q["GT"], ni)), np.zeros((NCH, q["GT"], ni))
            for t in range(fk + (mut == "first_kept"), T):
                ch = t // tchunk
                gl = ((t - ch * tchunk) % q["G"]) // NG
                accP[ch, gl] += dens[t]
                accF[ch, gl] += f[t]
            res = []
            for acc in (accP, accF):
                part = np.zeros((NCH, ni))
                for gl in range(q["GT"]):
                    part = part + acc[:, gl]
                s = np.zeros(ni)
                for ch in range(NCH):
                    s = s + part[ch]
                    if mut == "chunk0" and ch == 0:
                        s = s + part[0]
                res.append(s / float(kept))
            mean_pdf.append(res[0]); mean_fit.append(res[1])
        llik = np.zeros(T)
        for i in range(c.n):
            llik = llik + llpart[i]
        joint = np.zeros(c.n)
        for t in range(fk, T):
            joint = joint + np.exp(llpart[:, t])
        joint = joint / float(kept)
    return dict(llik=llik, mean_pdf=mean_pdf, mean_fit=mean_fit, joint=joint, ll=llpart)


def plain_pointwise(c, d=None):
    d = d or case_data(c)
    th, thx = rows(d)
    fk = c.first_kept
    sig = d["sigma"]
    ll, mean_pdf, mean_fit = np.zeros((c.n, c.T)), [], []
    with np.errstate(invalid="ignore"):
        for i in range(c.n):
            co = th + (np.einsum("tkmdp,d->tkmp", thx, d["X"][i]) if c.D else 0.0)
            z = d["Z"][i].T
            w = np.concatenate([np.ones((c.T, 1)), d["chi"][i].T], axis=1)
            co = np.where((z != 0)[:, :, None, None], co, 0.0)
            f = np.einsum("tk,tm,tkmp->tp", z, w, co) @ d["B"][i].T
            lt = -0.5 * np.log(2 * np.pi * sig)[:, None] - 0.5 * (d["Y"][i][None, :] - f) ** 2 / sig[:, None]
            ll[i] = lt.sum(axis=1)
            mean_pdf.append(np.exp(lt[fk:]).mean(axis=0))
            mean_fit.append(f[fk:].mean(axis=0))
    return dict(llik=ll.sum(axis=0), mean_pdf=mean_pdf, mean_fit=mean_fit, joint=np.exp(ll[:, fk:]).mean(axis=1), ll=ll)


def kern_cpo(c, d=None, mut=None):
    """k_post_cpo's matrix (n, T); columns before first_kept are NaN (the kernel never writes them)"""
    d = d or case_data(c)
    th, thx = rows(d)
    T, K, M, P, D, M1, fk = c.T, c.K, c.M, c.P, c.D, c.M + 1, c.first_kept
    W, st_all, Bc_all = windows(d["B"], P)
    off = np.concatenate([[0], np.cumsum(c.lens)])
    out = np.full((c.n, T), np.nan)
    sig = d["sigma"][fk:]
    Tk = T - fk
    pairs = [(0, 0)] + [(m, 0) for m in range(1, M1)] + [(a, b) for a in range(1, M1) for b in range(a, M1)]
    ia, ib = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    for i, ni in enumerate(c.lens):
        sV = np.zeros((Tk, M1, P))
        for k in range(K):
            x = th[fk:, k].copy()
            for dd in range(D):
                x = x + d["X"][i, dd] * thx[fk:, k, :, dd, :]
            sV = sV + d["Z"][i, k, fk:][:, None, None] * x
        st, Bc = st_all[off[i]:off[i + 1]], Bc_all[off[i]:off[i + 1]]
        f = _window_dot(Bc, st, sV, W)                                  # (Tk, M1, ni)
        NIP = (ni + 3) & ~3
        Ut = np.zeros((Tk, M1, NIP))
        Ut[:, 0, :ni] = d["Y"][i][None, :] - f[:, 0]
        Ut[:, 1:, :ni] = f[:, 1:]
        if mut == "pad":                                                # pad rows left as they were: here the row's last entry
            Ut[:, :, ni:] = Ut[:, :, ni - 1:ni]
        Ls = NIP // 4
        prod = (Ut[:, ia] * Ut[:, ib]).reshape(Tk, len(pairs), 4, Ls)
        p4 = np.zeros((Tk, len(pairs), 4))
        for j in range(Ls):
            p4 = p4 + prod[..., j]
        s4 = (p4[..., 0] + p4[..., 1]) + (p4[..., 2] if mut == "segment" else (p4[..., 2] + p4[..., 3]))
        rr, b = s4[:, 0], s4[:, 1:M1].copy()
        A = np.zeros((Tk, M, M))
        q = M1
        for m1 in range(M):
            for m2 in range(m1, M):
                A[:, m1, m2] = s4[:, q] + (sig if (m1 == m2 and mut != "chol_sigma") else 0.0)
                q += 1
        logdet, ww = np.zeros(Tk), np.zeros(Tk)
        for cc in range(M):
            dg = A[:, cc, cc].copy()
            for k2 in range(cc):
                dg = dg - A[:, cc, k2] * A[:, cc, k2]
            with np.errstate(invalid="ignore"):      # (a mutation may leave the pivot negative)
                l = np.sqrt(dg)
            A[:, cc, cc] = l
            wv = b[:, cc].copy()
            for k2 in range(cc):
                wv = wv - A[:, cc, k2] * b[:, k2]
            wv = wv / l
            b[:, cc] = wv
            logdet = logdet + 2.0 * np.log(l)
            ww = ww + wv * wv
            for r3 in range(cc + 1, M):
                vv = A[:, cc, r3].copy()
                for k2 in range(cc):
                    vv = vv - A[:, r3, k2] * A[:, cc, k2]
                A[:, r3, cc] = vv / l
        ld_ = float(ni if mut == "ni_for_ni_minus_M" else ni - M) * np.log(sig) + logdet
        quad = (rr - ww) / sig
        out[i, fk:] = -(0.5 * ni) * 1.83787706640934548356 - 0.5 * ld_ - 0.5 * quad
    return out


def kern_harmonic(rows_):
    """k_post_cpo_reduce on a matrix (n, kept): fmin and the sum of exponentials in draw order"""
    rows_ = np.asarray(rows_, dtype=np.float64)
    mn = rows_[:, 0].copy()
    for t in range(1, rows_.shape[1]):
        mn = np.fmin(mn, rows_[:, t])
    ph = np.zeros(len(rows_))
    for t in range(rows_.shape[1]):
        ph = ph + np.exp(mn - rows_[:, t])
    return np.log(float(rows_.shape[1])) + mn - np.log(ph)


def plain_cpo(c, d=None):
    d = d or case_data(c)
    th, thx = rows(d)
    M, fk = c.M, c.first_kept
    out = np.full((c.n, c.T), np.nan)
    sig = d["sigma"]
    for i, ni in enumerate(c.lens):
        co = th + (np.einsum("tkmdp,d->tkmp", thx, d["X"][i]) if c.D else 0.0)
        cv = np.einsum("tk,tkmp->tmp", d["Z"][i].T, co) @ d["B"][i].T            # (T, M1, ni)
        r, Um = d["Y"][i][None, :] - cv[:, 0], cv[:, 1:].transpose(0, 2, 1)
        A = Um.transpose(0, 2, 1) @ Um + sig[:, None, None] * np.eye(M)[None]
        L = np.linalg.cholesky(A)
        w = np.linalg.solve(L, (Um.transpose(0, 2, 1) @ r[:, :, None]))[:, :, 0]
        ld_ = (ni - M) * np.log(sig) + 2 * np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
        out[i] = -0.5 * ni * np.log(2 * np.pi) - 0.5 * ld_ - 0.5 * ((r * r).sum(axis=1) - (w * w).sum(axis=1)) / sig
    out[:, :fk] = np.nan
    return out


def kern_paths(c, d=None, mut=None):
    """k_post_paths without the noise: mean, mean_only lists of (kept, n_i)"""
    d = d or case_data(c)
    th, thx = rows(d)
    T, K, M, P, D, M1, fk = c.T, c.K, c.M, c.P, c.D, c.M + 1, c.first_kept
    W, st_all, Bc_all = windows(d["B"], P)
    off = np.concatenate([[0], np.cumsum(c.lens)])
    means, mos = [], []
    with np.errstate(invalid="ignore"):
        for i, ni in enumerate(c.lens):
            st, Bc = st_all[off[i]:off[i + 1]], Bc_all[off[i]:off[i + 1]]
            mean, mo = np.zeros((T - fk, ni)), np.zeros((T - fk, ni))
            for k in range(K):
                z = d["Z"][i, k, fk:][:, None]
                on = (z != 0) | (mut == "zskip")
                for mt in range(M1):
                    dot = np.zeros((T - fk, ni))
                    for w in range(W):
                        cf = th[fk:, k, mt][:, st + w]
                        for dd in range(D):
                            cf = cf + thx[fk:, k, mt, dd][:, st + w] * d["X"][i, dd]
                        dot = dot + cf * Bc[:, w]
                    if mt == 0:
                        mean, mo = np.where(on, mean + z * dot, mean), np.where(on, mo + z * dot, mo)
                    else:
                        mean = np.where(on, mean + z * d["chi"][i, mt - 1, fk:][:, None] * dot, mean)
            means.append(mean); mos.append(mo)
    return means, mos


def plain_paths(c, d=None):
    d = d or case_data(c)
    th, thx = rows(d)
    fk = c.first_kept
    means, mos = [], []
    with np.errstate(invalid="ignore"):
        for i in range(c.n):
            co = th + (np.einsum("tkmdp,d->tkmp", thx, d["X"][i]) if c.D else 0.0)
            z = d["Z"][i].T
            co = np.where((z != 0)[:, :, None, None], co, 0.0)
            w = np.concatenate([np.ones((c.T, 1)), d["chi"][i].T], axis=1)
            means.append((np.einsum("tk,tm,tkmp->tp", z, w, co) @ d["B"][i].T)[fk:])
            mos.append((np.einsum("tk,tkp->tp", z, co[:, :, 0]) @ d["B"][i].T)[fk:])
    return means, mos


def keyed_noise(c, d, seed):
    """sqrt(sigma^2(t)) z in long double and z itself (kept, n_obs): the oracle's keyed normal, UPD_SAMPLE_PATH, iteration = draw index,
    index = global observation index"""
    import oracle_lib as O
    n_obs = int(np.sum(c.lens))
    z = np.stack([O.fill(1, n_obs, seed=seed, chain=0, it=t, upd=UPD_SAMPLE_PATH) for t in range(c.first_kept, c.T)])
    return np.sqrt(d["sigma"][c.first_kept:].astype(LD))[:, None] * z.astype(LD), z


# ---------------------------------------------------------------------------------------------------------------------
# judging: every entry, non-finite values only where the restatement has the same
# ---------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    """the largest |got - ref| / bound over every entry; inf where an entry is not finite and the restatement's is not the same
    non-finite value, or where a bound is not positive"""
    got, ref, bound = np.asarray(got, dtype=LD).reshape(-1), np.asarray(ref, dtype=LD).reshape(-1), np.asarray(bound, dtype=LD).reshape(-1)
    if got.shape != ref.shape or got.shape != bound.shape:
        return float("inf")
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        same = (np.isnan(got) & np.isnan(ref)) | (np.isinf(got) & (got == ref))
        r = np.abs(got - ref) / bound
    r = np.where(same, LD(0), np.where(np.isfinite(got) & np.isfinite(ref) & (bound > 0), r, LD(np.inf)))
    r = np.where(np.isnan(r), LD(np.inf), r)
    return float(r.max())


def judge_pointwise(c, got, ref=None):
    """{quantity: largest error / (bound at G = 1)} of a result dict (llik, mean_pdf, mean_fit, joint; any may be missing)"""
    ref = ref or ld_pointwise(c)
    out = {}
    if got.get("llik") is not None:
        out["llik"] = ratio(got["llik"], ref["llik"], ref["b_llik"])
    for nm, b in (("mean_pdf", "b_pdf"), ("mean_fit", "b_fit")):
        if got.get(nm) is not None:
            out[nm] = ratio(np.concatenate(got[nm]), np.concatenate(ref[nm]), np.concatenate(ref[b]))
    if got.get("joint") is not None:
        out["joint"] = ratio(got["joint"], ref["joint"], ref["b_joint"])
    return out


def judge_paths(c, means, mos, ref=None):
    ref = ref or ld_pointwise(c)
    fk = c.first_kept
    return {"paths": max(ratio(means[i], ref["fit"][i][fk:], ref["b_fit_e"][i][fk:]) for i in range(c.n)),
            "mean_only": max(ratio(mos[i], ref["mo"][i][fk:], ref["b_mo_e"][i][fk:]) for i in range(c.n))}


def judge_cpo(c, mat, ref=None):
    ref = ref or ld_cpo(c)
    fk = c.first_kept
    return {"cpo_ll": ratio(np.asarray(mat)[:, fk:], ref["ll"][:, fk:], ref["b_ll"][:, fk:])}
