"""High-precision restatement of k_factor (csrc/kernels_factor.hip, csrc/factor_core.hpp), its error measure, its bounds and
the case list shared by tests/test_factor_ref.py (CPU) and tests/test_gpu_factor.py (device).  (Test infrastructure.)

What the kernel computes, per direction a = j MD + mt of the nu / Phi block:

    Prec_a = f H_aa + Prior_a,   f = beta / sigma^2
    Prior  = tau_j P_mat                                  (mt = 0)
             (1 / tau_j) I                                (mt = 0, multivariate model; UpdateNu.h:197)
             tilde_tau(j, mt) diag(gamma[j, :, mt - 1]),  tilde_tau = prod_{m' <= mt} delta(j, m')      (UpdatePhi.h:76-78)
    C_a = Prec_a^-1,   L_a = chol_lower(C_a),   L_a z_a

by a reverse Cholesky factorisation Prec = U U' (pivots from the last row up), X = U^-1, C = X'X, L z = X'z.

Reference.  `precisions` builds Prec_a in np.longdouble from the DEVICE's band rows of H_aa (so the contraction's rounding stays
out of this test; tests/pair_gram_ref.py owns that) and the pushed state.  `inverse_ld` is a hand-written reverse Cholesky and
triangular inverse in longdouble on the equilibrated matrix D^-1/2 Prec D^-1/2, D = diag(Prec), scaled back.  `pinv_ld` is a
cyclic Jacobi eigen-decomposition in longdouble with Armadillo's pinv tolerance (P max|w| 2^-52) for the singular route.
The reference's own error is about kappa_s 2^-64, i.e. 2^-11 / P of the bound below: it does not enter the comparison.
(tests/test_factor_ref.py checks inverse_ld against 50-digit mpmath.)

Measure.  The algorithm is invariant under diagonal scaling (D^1/2 U is the factor of D^1/2 A D^1/2 with the same rounding
errors up to the scaling's own), and the precisions here are badly scaled (gamma spans decades), so errors are measured in the
equilibrated frame:

    err_C  = || D^1/2 (C^ - C_ref) D^1/2 ||_2 / || D^1/2 C_ref D^1/2 ||_2
    err_Lz = || D^1/2 (Lz^ - L_ref z) ||_2 / ( || D^1/2 L_ref ||_2 ||z||_2 )

    err_C <= g_C P 2^-53 kappa_s,      err_Lz <= g_L P 2^-53 kappa_s,      kappa_s = kappa_2(D^-1/2 Prec D^-1/2).

Why kappa_s and not kappa_2(Prec): Cholesky's backward error is componentwise relative to sqrt(a_ii a_jj) (Demmel 1989), so
the computed factor is the exact factor of D^1/2 (A_s + E) D^1/2 with ||E||_2 = O(P u), and the forward error of the inverse is
governed by the condition of the equilibrated A_s -- which, by van der Sluis (1969), is within a factor P of the best any
diagonal scaling achieves.  kappa_2(Prec) would admit errors ten decades larger on the stiff states than the algorithm makes.

Constants.  g_C and g_L are 4 x the largest err / (P 2^-53 kappa_s) that `emulate`, a float64 numpy emulation of the device's
order of operations (root-free recursion, pivots from the last row up, the square roots afterwards, the back substitution
with the band entered from its far end, X'X summed over k in groups of four with kend = (P + 3) & ~3; the dense right-looking
form for bands above 5) with exact 1 / d and 1 / sqrt(d), shows over every direction of every case of CASES.  The factor 4 allows
for a different but equally valid summation order on the device and for the fma contraction of f H + prior.  They come from
the emulation, never from a device run.  Measured (tests/test_factor_ref.py recomputes them and asserts they have not grown):

    largest err_C  / (P 2^-53 kappa_s) = 0.197  (mid_5x5-prior, a diagonal precision)   ->  G_C = 0.8   (4 x, rounded up)
    largest err_Lz / (P 2^-53 kappa_s) = 0.0606 (lin_P6-benign)                         ->  G_L = 0.25
    pseudo-inverse route (float64 Jacobi emulation, kappa_s replaced by kappa+ = w_max / w_min+ of the retained eigenvalues;
    the null component of Lz, |n'Lz^| / (||L||_2 ||z||_2), is held to the same bound):
    largest err / (P 2^-53 kappa+)     = 0.0394 (cubic_P40-empty)                       ->  G_J = 0.16
On the stiff and wide cases the emulation stays below 0.02 P 2^-53 kappa_s: the constants are set by the smallest and the
diagonal matrices, where the bound is a few units of 2^-53 P.

Diagonal model (BW = 0 and BWP = 0): no condition number is involved.  |C^_pp d_p - 1| <= 16 2^-53 and
|Lz^_p sqrt(d_p) / z_p - 1| <= 16 2^-53 with d_p in longdouble, off-diagonal entries exactly 0: d_p carries about 2 roundings
(up to 4 with those of f and 1 / tau), a converged Newton step leaves about 3, the square doubles that and adds one.

Regimes (kappa_s over the directions of the cases, from the CPU restatement of H; test_factor_ref.py asserts the guards):
    benign   random_state's scales                                        kappa_s in [3, 560]
    stiff    sigma^2 = 1e-5, tau in [1e2, 1e4], tilde_tau to ~1e3,
             gamma log-uniform over [1e-3, 1e3]                           largest kappa_s of a case in [1.0e6, 2.9e7]
    prior    one cluster with Z_ik = 1e-4 (H_aa ~ 1e-8 of the others)     Cholesky route, rho >= 1e-9
    empty    one cluster without members: Prec = tau P_mat, rank P - 1    pseudo-inverse route, kappa+ in [27, 650]
The stiff states come with their own data: every curve observed on G = P / 2 common sites, so that H_aa has rank <= G and the
prior alone -- at 1e-6 .. 1e-9 of the data term -- holds the rest of the spectrum (all directions: kappa_s in [150, 2.9e7]; the
prior cases reach 1.0e6).  The diagonal model has kappa_s = 1 in every regime (its stiff cases exercise extreme d_p only).
rho = (smallest pivot of the reverse factorisation) / (largest diagonal entry) is what factor_wave judges against 1e-12:
every Cholesky-route direction has rho >= 1e-9, every pseudo-inverse direction a structurally zero cluster column.
"""
import zlib

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)

# measured by tests/test_factor_ref.py::test_emulation_passes_and_constants_hold (see the docstring above)
MEASURED_C, MEASURED_L, MEASURED_J = 0.197, 0.0606, 0.0394
G_C, G_L, G_J = 0.8, 0.25, 0.16
DIAG_TOL = 16 * U

UPD_PHI, UPD_NU = 7, 12            # update ids of the keyed generator (oracle/oracle.h, csrc/rng.hpp)
BWMAX, BWMID, BWWIDE = 5, 15, 31   # band instantiations (csrc/model.hpp)
SEED = 5                           # the run's RNG seed


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, kind, P, regime, deg=None, degs=None, n_int=None, K=2, M=2, nch=1, special=None, pen_band=0):
        self.name, self.kind, self.P, self.regime, self.K, self.M, self.nch = name, kind, P, regime, K, M, nch
        self.deg, self.degs, self.n_int, self.special = deg, degs, n_int, special
        self.n, self.MD, self.A = 24, M + 1, K * (M + 1)
        self.PP = 32 if P <= 32 else 64
        if kind == "spline":
            self.band, self.pen_band = min(deg, P - 1), 1
            self.BW, self.BWP = self.band, max(self.band, 1)
        elif kind == "tensor":
            Pl = [k + g + 1 for k, g in zip(n_int, degs)]
            strides = [int(np.prod(Pl[l + 1:])) for l in range(len(Pl))]
            assert int(np.prod(Pl)) == P
            self.band, self.pen_band = sum(g * s for g, s in zip(degs, strides)), max(strides)
            self.BW = self.band if self.band <= BWMAX else BWMID if self.band <= BWMID else BWWIDE
            self.BWP = min(max(self.BW, self.pen_band), BWWIDE if self.BW > BWMAX else BWMAX)
        elif kind == "step":      # a caller-supplied basis with one non-zero per row (B'B diagonal) and a penalty of band pen_band
            self.band, self.pen_band, self.BW, self.BWP = 0, pen_band, 0, pen_band
        else:
            self.band = self.pen_band = self.BW = self.BWP = 0
        self.diag = self.BW == 0 and self.BWP == 0
        self.empty = 1 if special == "empty" else None          # the cluster without members
        self.weak = 1 if special == "prior" else None           # the cluster with Z_ik = 1e-4

    @property
    def data_key(self):
        key = (self.kind, self.P, self.deg, tuple(self.degs or ()), self.K, self.M, self.regime == "stiff")
        return key + (self.pen_band,) if self.kind == "step" else key


_INST = [  # one per (band class, PP); among them P = 32 (= PP), 33, 64 (the build limit), P % 4 == 1, P % 4 == 2, a small P
    dict(name="lin_P6", kind="spline", deg=1, P=6), dict(name="lin_P33", kind="spline", deg=1, P=33),
    dict(name="quad_P29", kind="spline", deg=2, P=29), dict(name="quad_P64", kind="spline", deg=2, P=64),
    dict(name="cubic_P30", kind="spline", deg=3, P=30, K=3), dict(name="cubic_P40", kind="spline", deg=3, P=40),
    dict(name="quart_P32", kind="spline", deg=4, P=32), dict(name="quart_P50", kind="spline", deg=4, P=50),
    dict(name="quint_P27", kind="spline", deg=5, P=27), dict(name="quint_P47", kind="spline", deg=5, P=47),
    dict(name="mid_5x5", kind="tensor", degs=[1, 1], n_int=[3, 3], P=25),           # band 6: BWMID, PP = 32
    dict(name="mid_6x6", kind="tensor", degs=[1, 1], n_int=[4, 4], P=36),           # band 7: BWMID, PP = 64
    dict(name="wide_5x6", kind="tensor", degs=[3, 3], n_int=[1, 2], P=30),          # band 21: BWWIDE, PP = 32
    dict(name="wide_7x7", kind="tensor", degs=[3, 3], n_int=[3, 3], P=49),          # band 24: BWWIDE, PP = 64
    dict(name="mv_P7", kind="mv", P=7, K=3), dict(name="mv_P64", kind="mv", P=64),
]
_BY_INST = {d["name"]: d for d in _INST}


def _mk(inst, regime, **kw):
    d = dict(_BY_INST[inst])
    d.update(kw)
    d["name"] = f"{inst}-{regime}" + ("-2chains" if kw.get("nch", 1) > 1 else "")
    return Case(regime=regime if regime in ("benign", "stiff") else "benign", special=None if regime in ("benign", "stiff") else regime, **d)


CASES = ([_mk(i["name"], "benign") for i in _INST] + [_mk(i["name"], "stiff") for i in _INST]
         + [_mk("cubic_P30", "prior"), _mk("mid_5x5", "prior")]
         + [_mk("cubic_P30", "empty"), _mk("cubic_P40", "empty"), _mk("wide_5x6", "empty")]
         + [_mk("cubic_P30", "stiff", nch=2)])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# data and states of the cases (the same on the CPU and on the device)
# ---------------------------------------------------------------------------------------------------------------------
_data = {}
# seeds of the stiff states that did not meet the regime guards (test_factor_ref.py) with salt 0: tuned on the CPU, from the
# reference alone
STATE_SALT = {"mid_5x5-stiff": 1, "mid_6x6-stiff": 1, "wide_7x7-stiff": 1}


def case_data(c):
    """n = 24 ragged curves.  spline: y, t lists, internal / boundary knots; tensor: y, basis rows B (the oracle's tensor
    B-spline), P_mat; multivariate: Y (n x P); step: y, t, one-hot basis rows B, P_mat (RW1, or I for pen_band 0)."""
    key = c.data_key
    if key in _data:
        return _data[key]
    import oracle_lib as O
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    n = c.n
    # stiff regime: every curve is observed on a few of G < P common sites, so H_aa has rank <= G and the prior alone holds the
    # rest of the spectrum, at 1e-6 .. 1e-9 of the data term
    G = max(2, c.P // 2)
    sparse = c.regime == "stiff"
    if c.kind == "mv":
        d = dict(Y=rng.standard_normal((n, c.P)) * 2.0, Pmat=np.eye(c.P))
    elif c.kind == "step":
        ni = rng.integers(14, 31, size=n)
        t = [np.sort(rng.uniform(0.0, 1.0, size=k)) for k in ni]
        B = [np.eye(c.P)[np.minimum((x * c.P).astype(int), c.P - 1)] for x in t]
        d = dict(y=[rng.standard_normal(k) * 2.0 for k in ni], t=t, B=B, Pmat=O.pmat_rw1(c.P) if c.pen_band else np.eye(c.P))
    elif c.kind == "spline":
        if sparse:
            sites = (np.arange(G) + rng.uniform(0.0, 1.0, size=G)) / G          # one site in each of G equal intervals
            t = [np.sort(rng.choice(sites, size=int(k))) for k in rng.integers(100, 241, size=n)]
            ni = [len(x) for x in t]
        else:
            ni = rng.integers(14, 31, size=n)
            t = [np.sort(rng.uniform(0.0, 1.0, size=k)) for k in ni]
        y = [rng.standard_normal(k) * 2.0 for k in ni]
        ik = np.linspace(0.0, 1.0, c.P - c.deg - 1 + 2)[1:-1]
        bk = np.array([0.0, 1.0])
        d = dict(y=y, t=t, ik=ik, bk=bk, B=[O.bspline_basis(x, ik, c.deg, bk) for x in t], Pmat=O.pmat_rw1(c.P))
    else:
        dim = len(c.degs)
        iks = [np.linspace(0.0, 1.0, k + 2)[1:-1] for k in c.n_int]
        if sparse:
            sites = rng.uniform(0.0, 1.0, size=(G, dim))
            t = [sites[rng.choice(G, size=int(k))] for k in rng.integers(100, 241, size=n)]
            ni = [len(x) for x in t]
        else:
            ni = rng.integers(20, 41, size=n)
            t = [rng.uniform(0.0, 1.0, size=(k, dim)) for k in ni]
        B = [np.ascontiguousarray(O.tensor_bspline(x, c.degs, [[0.0, 1.0]] * dim, iks)) for x in t]
        d = dict(y=[rng.standard_normal(k) * 2.0 for k in ni], t=t, B=B, Pmat=np.ascontiguousarray(O.get_P(c.degs, c.n_int)))
    _data.clear()
    _data[key] = d
    return d


def case_state(c, q=0):
    """the state pushed to chain q of case c"""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) + 7919 * q + 104729 * STATE_SALT.get(c.name, 0))
    n, K, M, P = c.n, c.K, c.M, c.P
    Z = rng.dirichlet(np.full(K, 2.0), size=n)
    if c.empty is not None:
        Z[:, c.empty] = 0.0
        Z /= Z.sum(axis=1, keepdims=True)
    if c.weak is not None:
        Z[:, c.weak] = 0.0
        Z *= (1.0 - 1e-4) / Z.sum(axis=1, keepdims=True)
        Z[:, c.weak] = 1e-4
    st = dict(nu=rng.standard_normal((K, P)), Phi=0.3 * rng.standard_normal((K, P, M)), chi=rng.standard_normal((n, M)), Z=Z,
              pi=rng.dirichlet(np.full(K, 5.0)), alpha_3=np.array([3.5]), A=rng.gamma(2.0, 1.0, size=(K, 2)))
    if c.regime == "benign":        # gpu_parity.random_state's scales
        st.update(delta=rng.gamma(2.0, 1.0, size=(K, M)), gamma=rng.gamma(2.0, 0.7, size=(K, P, M)),
                  tau=rng.gamma(3.0, 0.5, size=K), sigma_sq=np.array([0.01 * (1.0 + rng.uniform())]))
    else:
        lu = lambda lo, hi, size: np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))
        st.update(delta=lu(20.0, 45.0, (K, M)) if M == 2 else lu(1e3 ** (1.0 / M) * 0.7, 1e3 ** (1.0 / M) * 1.4, (K, M)),
                  gamma=lu(1e-3, 1e3, (K, P, M)), tau=lu(1e2, 1e4, K), sigma_sq=np.array([1e-5]))
    return st


def normals(c, q=0, it=0, tt=0):
    """z_a of every direction from the oracle's keyed generator with k_factor's index layout: idx0 = j P (nu, UPD_NU),
    (j M + mt - 1) P (Phi, UPD_PHI); iteration `it` (tt: sweep of a tempered-transition block, 0 a plain iteration), chain id q.
    Returns (A, P)."""
    import oracle_lib as O
    K, M, P, MD = c.K, c.M, c.P, c.MD
    znu = O.fill(1, K * P, seed=SEED, chain=q, it=it, upd=UPD_NU, tt=tt)
    zphi = O.fill(1, K * M * P, seed=SEED, chain=q, it=it, upd=UPD_PHI, tt=tt)
    z = np.zeros((c.A, P))
    for j in range(K):
        z[j * MD] = znu[j * P:(j + 1) * P]
        for mt in range(1, MD):
            z[j * MD + mt] = zphi[(j * M + mt - 1) * P:(j * M + mt) * P]
    return z


def tri(n, a, b):
    a, b = min(a, b), max(a, b)
    return a * n - a * (a - 1) // 2 + (b - a)


def hrow(c, a, b):
    """row of H that holds H_ab (a = j MD + mt); as tests/test_gpu_parity.py::test_pair_gram_mfma indexes it"""
    MD = c.MD
    ncc = MD * (MD + 1) // 2
    return tri(c.K, a // MD, b // MD) * ncc + tri(MD, a % MD, b % MD)


def hbands_from_H(c, H):
    """H (R x LG, the device's debug array) -> hb[a, t, p] = H_aa[p, p + t], t = 0 .. BW"""
    H = np.asarray(H).reshape(-1, c.BW + 1, c.P)
    return np.stack([H[hrow(c, a, a)] for a in range(c.A)])


def host_H(c, st):
    """the same array computed on the host in float64 from the basis rows (CPU tests; rounding differs from the device's)"""
    d = case_data(c)
    n, K, MD, P, BW = c.n, c.K, c.MD, c.P, c.BW
    chit = np.concatenate([np.ones((n, 1)), st["chi"]], axis=1)
    W = np.einsum("ij,im->ijm", st["Z"], chit).reshape(n, K * MD)
    G = np.stack([np.eye(P)] * n) if c.kind == "mv" else np.stack([B.T @ B for B in d["B"]])
    R = (K * (K + 1) // 2) * (MD * (MD + 1) // 2)
    H = np.zeros((R, BW + 1, P))
    for a in range(c.A):
        for b in range(a, c.A):
            Hab = np.einsum("i,ipq->pq", W[:, a] * W[:, b], G)
            for t in range(min(BW, P - 1) + 1):
                H[hrow(c, a, b), t, :P - t] = np.diagonal(Hab, t)
    return H.reshape(R, (BW + 1) * P)


# ---------------------------------------------------------------------------------------------------------------------
# the precision matrices
# ---------------------------------------------------------------------------------------------------------------------
def build_prec(c, hb_a, st, a, dtype, mut=None):
    """Prec_a (P x P, dense) in `dtype` from the band rows hb_a[t, p] = H_aa[p, p + t] and the state.  float64: the device's
    order (f = 1 / sigma^2 rounded, tilde_tau a running product, f h + scale * prior).  mut: a mutation's name."""
    P, MD = c.P, c.MD
    j, mt = a // MD, a % MD
    T = dtype
    hb_a = np.asarray(hb_a, dtype=np.float64)
    if mut == "h_shift":                       # row p reads the band of row p + 1
        hb_a = hb_a[:, np.minimum(np.arange(P) + 1, P - 1)]
    f = T(1.0) / T(st["sigma_sq"][0])
    Prec = np.zeros((P, P), dtype=T)
    for t in range(min(c.band, P - 1) + 1):
        v = f * hb_a[t, :P - t].astype(T)
        Prec[np.arange(P - t), np.arange(t, P)] = v
        Prec[np.arange(t, P), np.arange(P - t)] = v
    if mt == 0:
        tau = T(st["tau"][j])
        if c.kind == "mv":
            Prec += np.diag(np.full(P, T(1.0) / tau))
        else:
            Pm = case_data(c)["Pmat"].astype(T)
            if mut == "drop_prior_edge":       # the prior's outermost band entry of one row
                Pm = Pm.copy()
                p0 = P // 2
                Pm[p0, p0 + c.pen_band] = Pm[p0 + c.pen_band, p0] = T(0.0)
            Prec += tau * Pm
    else:
        tt = T(1.0)
        for m2 in range(mt - 1 if mut == "tilde_tau_short" else mt):
            tt = tt * T(st["delta"][j, m2])
        Prec += np.diag(tt * st["gamma"][j, :, mt - 1].astype(T))
    return Prec


def precisions(c, hb, st):
    """Prec_a in np.longdouble for every direction a = j MD + mt"""
    return [build_prec(c, hb[a], st, a, LD) for a in range(c.A)]


# ---------------------------------------------------------------------------------------------------------------------
# longdouble reference
# ---------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _norm2(M):
    return float(np.linalg.norm(np.asarray(M, dtype=np.float64), 2))


def inverse_ld(Prec):
    """C_ref = Prec^-1 and L_ref = chol_lower(C_ref) in longdouble by a reverse Cholesky Prec = U U' of the equilibrated matrix
    and U^-1; also D = diag(Prec), kappa_s and rho (see the module docstring)."""
    A = np.array(Prec, dtype=LD)
    P = A.shape[0]
    D = np.diagonal(A).copy()
    sd = np.sqrt(D)
    As = A / np.outer(sd, sd)
    W = As.copy()
    Um = np.zeros((P, P), dtype=LD)
    piv = np.zeros(P, dtype=LD)
    for k in range(P - 1, -1, -1):
        piv[k] = W[k, k]
        if not piv[k] > 0:
            return Ref(ok=False, D=D, rho=float(piv[k] * D[k] / D.max()))
        Um[k, k] = np.sqrt(W[k, k])
        Um[:k, k] = W[:k, k] / Um[k, k]
        W[:k, :k] -= np.outer(Um[:k, k], Um[:k, k])
    X = np.zeros((P, P), dtype=LD)             # X = U^-1, upper
    for i in range(P - 1, -1, -1):
        X[i, i] = LD(1.0) / Um[i, i]
        if i + 1 < P:
            X[i, i + 1:] = -(Um[i, i + 1:] @ X[i + 1:, i + 1:]) / Um[i, i]
    Cs = X.T @ X
    C = Cs / np.outer(sd, sd)
    L = X.T / sd[:, None]
    return Ref(ok=True, C=C, L=L, D=D, Cs=Cs, kappa_s=_norm2(As) * _norm2(Cs), rho=float((piv * D).min() / D.max()))


def jacobi_ld(A, dtype=LD, sweeps=40):
    """cyclic Jacobi: eigenvalues w and eigenvectors V (columns) of the symmetric A in `dtype`"""
    S = np.array(A, dtype=dtype)
    P = S.shape[0]
    V = np.eye(P, dtype=dtype)
    eps = np.finfo(dtype).eps
    for _ in range(sweeps):
        off = np.sqrt(((S - np.diag(np.diagonal(S))) ** 2).sum())
        if off <= eps * np.sqrt((np.diagonal(S) ** 2).sum()) * 1e-3:
            break
        for p in range(P - 1):
            for q in range(p + 1, P):
                if S[p, q] == 0:
                    continue
                th = (S[q, q] - S[p, p]) / (2 * S[p, q])
                t = (1 if th >= 0 else -1) / (abs(th) + np.sqrt(th * th + 1))
                cs = 1 / np.sqrt(t * t + 1)
                sn = t * cs
                cp, cq = S[:, p].copy(), S[:, q].copy()
                S[:, p], S[:, q] = cs * cp - sn * cq, sn * cp + cs * cq
                rp, rq = S[p, :].copy(), S[q, :].copy()
                S[p, :], S[q, :] = cs * rp - sn * rq, sn * rp + cs * rq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = cs * vp - sn * vq, sn * vp + cs * vq
    return np.diagonal(S).copy(), V


def pinv_ld(Prec):
    """pseudo-inverse by a longdouble eigen-decomposition; eigenvalues at or below Armadillo's tolerance P max|w| 2^-52 are
    dropped.  Returns C, the null vectors (columns), kappa+ = w_max / w_min+ of the retained ones, and D."""
    A = np.array(Prec, dtype=LD)
    P = A.shape[0]
    w, V = jacobi_ld(A)
    tol = P * np.abs(w).max() * LD(2.0) ** -52
    keep = np.abs(w) > tol
    C = (V[:, keep] / w[keep]) @ V[:, keep].T
    return Ref(C=C, null=V[:, ~keep], kappa_p=float(w[keep].max() / w[keep].min()), D=np.diagonal(A).copy(),
               Lnorm=float(1 / np.sqrt(w[keep].min())), n_null=int((~keep).sum()))


def err_C(C_hat, C_ref, D):
    """(err, (p, q) of the worst entry in the scaled frame)"""
    sd = np.sqrt(np.asarray(D, dtype=LD))
    E = (np.asarray(C_hat, dtype=np.float64).astype(LD) - C_ref) * np.outer(sd, sd)
    Ef = np.asarray(np.abs(E), dtype=np.float64)
    pq = np.unravel_index(np.argmax(Ef), Ef.shape)
    return _norm2(E) / _norm2(C_ref * np.outer(sd, sd)), (int(pq[0]), int(pq[1]))


def err_Lz(Lz_hat, L_ref, z, D):
    sd = np.sqrt(np.asarray(D, dtype=LD))
    e = (np.asarray(Lz_hat, dtype=np.float64).astype(LD) - L_ref @ np.asarray(z, dtype=LD)) * sd
    ef = np.asarray(np.abs(e), dtype=np.float64)
    return float(np.sqrt((e * e).sum())) / (_norm2(L_ref * sd[:, None]) * float(np.linalg.norm(z))), int(np.argmax(ef))


def bound(P, kappa, g):
    return g * P * U * kappa


def check_diag(C_hat, Lz_hat, Prec, z):
    """the diagonal model's check: (worst |C^_pp d_p - 1|, worst |Lz^_p sqrt(d_p) / z_p - 1|, off-diagonal entries all zero)"""
    d = np.diagonal(np.asarray(Prec, dtype=LD))
    C_hat = np.asarray(C_hat, dtype=np.float64)
    eC = float(np.abs(np.diagonal(C_hat).astype(LD) * d - 1).max())
    eL = float(np.abs(np.asarray(Lz_hat, dtype=np.float64).astype(LD) * np.sqrt(d) / np.asarray(z, dtype=LD) - 1).max())
    off = C_hat - np.diag(np.diagonal(C_hat))
    return eC, eL, bool((off == 0.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulation of the device's order of operations
# ---------------------------------------------------------------------------------------------------------------------
def _xtx(X, P, kend):
    """C = X'X with k summed in groups of four (the 16x16x4 MFMA): rows k >= kend do not enter"""
    C = np.zeros((P, P))
    Xp = np.zeros((max(kend, P) + 4, P))
    Xp[:P] = X
    for k0 in range(0, kend, 4):
        g = np.outer(Xp[k0], Xp[k0])
        for k in range(k0 + 1, k0 + 4):
            g = g + np.outer(Xp[k], Xp[k])
        C = C + g
    return C


def emulate(Prec, z, bw, mut=None):
    """C^, Lz^ of a float64 precision by the device's algorithm with exact 1 / d and 1 / sqrt(d) (each rounded once).
    bw: the band half-width the kernel runs (BWP); above 5 the dense right-looking form.  mut: a mutation's name."""
    A = np.array(Prec, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    P = A.shape[0]
    if mut == "forward":                        # first row down: the same algorithm on the reversed matrix
        C, Lz = emulate(A[::-1, ::-1], z[::-1], bw)
        return C[::-1, ::-1].copy(), Lz[::-1].copy()
    rerr = 1.0 + 1e-13 if mut == "recip" else 1.0
    X = np.zeros((P, P))                        # X[i, c] = U^-1(i, c), upper
    if bw == 0:                                 # the diagonal branch
        d = np.diagonal(A)
        rk = (1.0 / np.sqrt(d)) * rerr
        return np.diag(rk * rk), rk * z
    if bw > BWMAX:
        S = A.copy()
        Um = np.zeros((P, P))
        for k in range(P - 1, -1, -1):
            dk = S[k, k]
            rk = (1.0 / np.sqrt(dk)) * rerr
            Um[k, k] = dk * rk
            Um[:k, k] = S[:k, k] * rk
            S[:k, :k] -= np.outer(Um[:k, k], Um[:k, k])
        for i in range(P - 1, -1, -1):
            acc = np.zeros(P)
            for ql in range(4):                 # four partial sums per column, m = i + 1 + ql, + 4, ...
                part = np.zeros(P)
                for m in range(i + 1 + ql, P, 4):
                    part[m:] = part[m:] + Um[i, m] * X[m, m:]
                acc = part if ql == 0 else acc + part
            X[i, i] = (1.0 - 0.0) / Um[i, i]
            X[i, i + 1:] = -acc[i + 1:] / Um[i, i]
        if mut == "uinv_z":
            Lz = X @ z
        else:
            Lz = np.zeros(P)
            for i in range(P):
                Lz[i:] = Lz[i:] + X[i, i:] * z[i]
    else:
        d = np.diagonal(A).copy()
        v = np.zeros((P, P))                    # v[i, k] = v(i, k), i < k
        w = np.zeros((P, P))                    # w[i, k] = v(i, k) / d_k
        for k in range(P - 1, -1, -1):
            dk = d[k]
            for t in range(min(bw, k), 0, -1):
                i = k - t
                acc = A[i, k]
                for m in range(1, bw - t + 1):
                    if k + m < P:
                        acc -= w[i, k + m] * v[k, k + m]
                v[i, k] = acc
            inv = (1.0 / dk) * rerr
            for t in range(1, min(bw, k) + 1):
                i = k - t
                w[i, k] = v[i, k] * inv
                d[i] = d[i] - v[i, k] * w[i, k]
        rk = (1.0 / np.sqrt(d)) * rerr
        Um = np.zeros((P, P))
        Um[np.arange(P), np.arange(P)] = d * rk
        for t in range(1, bw + 1):
            Um[np.arange(P - t), np.arange(t, P)] = v[np.arange(P - t), np.arange(t, P)] * rk[t:]
        Lz = np.zeros(P)
        for i in range(P - 1, -1, -1):
            acc = np.zeros(P)
            for t in range(min(bw, P - 1 - i), 0, -1):       # the far end of the band first
                acc = acc + Um[i, i + t] * X[i + t]
            row = -(acc * rk[i])
            row[:i + 1] = 0.0
            row[i] = rk[i]
            X[i] = row
            if mut != "uinv_z":
                Lz = Lz + row * z[i]
        if mut == "uinv_z":
            Lz = X @ z
    kend = (P & ~3) if mut == "kend" else (P + 3) & ~3
    return _xtx(X, P, kend), Lz


def emulate_pinv(Prec, z):
    """float64 emulation of factor_pinv: round-robin parallel Jacobi (disjoint rotations of a round applied together), pinv
    tolerance P max|w| 2^-52, eigenpairs by ascending w, the generic-weights sign rule, L z in index order"""
    S = np.array(Prec, dtype=np.float64)
    P = S.shape[0]
    PP = 32 if P <= 32 else 64
    Sp = np.zeros((PP, PP))
    Sp[:P, :P] = S
    V = np.eye(PP)
    for _ in range(30):
        flag = False
        for r in range(PP - 1):
            J = np.eye(PP)
            for i in range(PP // 2):
                p = (r + i) % (PP - 1)
                q = PP - 1 if i == 0 else (r - i + (PP - 1)) % (PP - 1)
                apq, app, aqq = Sp[p, q], Sp[p, p], Sp[q, q]
                if abs(apq) > 1e-20 * np.sqrt(abs(app * aqq)) and apq != 0.0:
                    th = (aqq - app) / (2.0 * apq)
                    t = (1.0 if th >= 0 else -1.0) / (abs(th) + np.sqrt(th * th + 1.0))
                    cs = 1.0 / np.sqrt(t * t + 1.0)
                    sn = t * cs
                    J[p, p], J[q, q], J[p, q], J[q, p] = cs, cs, sn, -sn
                    flag = True
            Sp = J.T @ (Sp @ J)
            V = V @ J
        if not flag:
            break
    w = np.diagonal(Sp)[:P].copy()
    Vp = V[:P, :P]
    tol = P * np.abs(w).max() * 2.220446049250313e-16
    winv = np.where(np.abs(w) > tol, 1.0 / np.where(w == 0, 1.0, w), 0.0)
    C = np.zeros((P, P))
    for k in range(P):
        C = C + np.outer(Vp[:, k] * winv[k], Vp[:, k])
    order = np.lexsort((np.arange(P), w))
    sg = np.where((Vp / (np.arange(P)[:, None] + 1.37)).sum(axis=0) < 0, -1.0, 1.0)
    Lz = np.zeros(P)
    for r, k in enumerate(order):
        Lz = Lz + sg[k] * Vp[:, k] * np.sqrt(max(winv[k], 0.0)) * z[r]
    return C, Lz


# ---------------------------------------------------------------------------------------------------------------------
# one direction against the reference
# ---------------------------------------------------------------------------------------------------------------------
def is_pinv_direction(c, a):
    """the directions that take the pseudo-inverse route: nu of the cluster without members (Prec = tau P_mat, rank P - 1)"""
    return c.empty is not None and a == c.empty * c.MD


def reference(c, a, Prec):
    """the longdouble reference of direction a: pinv_ld on the pseudo-inverse route, inverse_ld otherwise (None: diagonal model)"""
    if c.diag:
        return None
    return pinv_ld(Prec) if is_pinv_direction(c, a) else inverse_ld(Prec)


def check_direction(c, a, Prec, C_hat, Lz_hat, z, R=None):
    """compare one direction with the reference (R: reference(c, a, Prec), computed here if not given).  Returns a dict: ok,
    route, ratios (error / bound) and a message."""
    j, mt = a // c.MD, a % c.MD
    head = f"{c.name}: direction a {a} = (j {j}, mt {mt}), instantiation (PP {c.PP}, BW {c.BW}, BWP {c.BWP})"
    C_hat, Lz_hat = np.asarray(C_hat, dtype=np.float64), np.asarray(Lz_hat, dtype=np.float64)
    if not (np.isfinite(C_hat).all() and np.isfinite(Lz_hat).all()):
        return dict(ok=False, route="-", rC=np.inf, rL=np.inf, kappa=np.nan, msg=head + ": not finite")
    if c.diag:
        eC, eL, off = check_diag(C_hat, Lz_hat, Prec, z)
        ok = eC <= DIAG_TOL and eL <= DIAG_TOL and off
        return dict(ok=ok, route="diag", rC=eC / DIAG_TOL, rL=eL / DIAG_TOL, kappa=1.0,
                    msg=head + f": diagonal model: |C d - 1| = {eC / U:.2f} u, |Lz sqrt(d) / z - 1| = {eL / U:.2f} u (<= 16 u), "
                               f"off-diagonal zero: {off}")
    if is_pinv_direction(c, a):
        R = pinv_ld(Prec) if R is None else R
        eC, pq = err_C(C_hat, R.C, R.D)
        bC = bound(c.P, R.kappa_p, G_J)
        comp = float(np.abs(R.null.T @ Lz_hat.astype(LD)).max()) if R.n_null else 0.0
        bN = bound(c.P, R.kappa_p, G_J) * R.Lnorm * float(np.linalg.norm(z))
        ok = R.n_null >= 1 and eC <= bC and comp <= bN
        return dict(ok=ok, route="pinv", rC=eC / bC if bC else np.inf, rL=comp / bN if bN else np.inf, kappa=R.kappa_p, raw=(eC, comp / (R.Lnorm * float(np.linalg.norm(z)))),
                    msg=head + f": pseudo-inverse route, {R.n_null} null vector(s), kappa+ {R.kappa_p:.3g}: err_C {eC:.3g} "
                               f"(bound {bC:.3g}, worst entry {pq}), null component of Lz {comp:.3g} (bound {bN:.3g})")
    R = inverse_ld(Prec) if R is None else R
    if not R.ok:
        return dict(ok=False, route="chol", rC=np.inf, rL=np.inf, kappa=np.inf, msg=head + ": the reference factorisation broke down")
    eC, pq = err_C(C_hat, R.C, R.D)
    eL, pl = err_Lz(Lz_hat, R.L, z, R.D)
    bC, bL = bound(c.P, R.kappa_s, G_C), bound(c.P, R.kappa_s, G_L)
    ok = eC <= bC and eL <= bL
    return dict(ok=ok, route="chol", rC=eC / bC if bC else np.inf, rL=eL / bL if bL else np.inf, kappa=R.kappa_s, rho=R.rho, raw=(eC, eL),
                msg=head + f", kappa_s {R.kappa_s:.3g}, rho {R.rho:.3g}: err_C {eC:.3g} (bound {bC:.3g}, worst entry (p, q) = {pq} "
                           f"in the scaled frame), err_Lz {eL:.3g} (bound {bL:.3g}, worst entry p = {pl})")


def emulate_direction(c, hb_a, st, a, z, mut=None):
    """the emulation's C^, Lz^ of direction a (float64 precision built in the device's order)"""
    Prec = build_prec(c, hb_a, st, a, np.float64, mut=mut)
    if is_pinv_direction(c, a):
        return emulate_pinv(Prec, z)
    return emulate(Prec, z, c.BWP, mut=mut)


# ---------------------------------------------------------------------------------------------------------------------
# r_a = t_a - sum_b H_ab theta_b and H_aa theta_a (k_factor's other output)
# ---------------------------------------------------------------------------------------------------------------------
def rvec_ref(c, H, tvec, st):
    """r (A x P), hq (A x P) in longdouble from the device's H, tvec and the pushed nu / Phi, and the sums of absolute terms"""
    P, A, MD, BW = c.P, c.A, c.MD, c.BW
    H = np.asarray(H).reshape(-1, BW + 1, P).astype(LD)
    theta = np.zeros((A, P), dtype=LD)
    for a in range(A):
        j, mt = a // MD, a % MD
        theta[a] = st["nu"][j] if mt == 0 else st["Phi"][j, :, mt - 1]
    r = np.asarray(tvec, dtype=np.float64).reshape(A, P).astype(LD)
    ra = np.abs(r)
    hq, hqa = np.zeros((A, P), dtype=LD), np.zeros((A, P), dtype=LD)
    for a in range(A):
        for b in range(A):
            hb = H[hrow(c, a, b)]
            v, va = np.zeros(P, dtype=LD), np.zeros(P, dtype=LD)
            for t in range(min(BW, P - 1) + 1):
                g = hb[t, :P - t]
                v[:P - t] += g * theta[b, t:]
                va[:P - t] += np.abs(g * theta[b, t:])
                if t > 0:
                    v[t:] += g * theta[b, :P - t]
                    va[t:] += np.abs(g * theta[b, :P - t])
            r[a] -= v
            ra[a] += va
            if a == b:
                hq[a], hqa[a] = v, va
    return r, ra, hq, hqa


def rvec_bound(c, S_abs):
    return (c.A * (2 * c.BW + 1) + 4) * U * np.asarray(S_abs, dtype=np.float64)
