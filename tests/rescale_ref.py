"""numpy restatement, in long double, of the reference's rescale step per draw (kernels_rescale.hip):

    curve[k]  = the smallest i that attains max_i Z[i, perm[k]]          (arma::index_max; a NaN is never the maximum)
    A[k][c]   = Z[curve[k], c]                                           (copied: exact)
    Ainv      = A^-1 by Gauss-Jordan elimination with partial pivoting, the device's order (kernels_rescale.hip), here in long double
    rcond     = 1 / (|A|_1 |Ainv|_1),      z_min = min_{i,k} (Z Ainv)[i, k]
    nu~_k     = sum_c A[k][c] nu_c   (Phi, eta, xi alike),      Z~ = Z Ainv
    mean      v[k, g]    = sum_p E_gp sum_c A[k][c] (nu_c,p + sum_d x_d eta[p, d, c])
    cov       c_r(g, h)  = sum_m W~1_k[g][m] W~2_l[h][m],  W~_k = sum_c A[k][c] W_c,  W_c[g][m] = sum_p E_gp (Phi[c, p, m] + sum_d x_d xi[p, d, m, c])

Arrays are in get_chain's layout without the slot axis: Z (n, K), nu (K, P), Phi (K, P, M), eta (P, D, K), xi (P, D, M, K).

Bound of the inverse (inverse_bound), derived for the elimination actually used, with u = 2^-52 (the project's convention: twice
the unit roundoff).  Gauss-Jordan elimination with partial pivoting computes X with |X - A^-1| <= c_K u |A^-1| |L| |U| |A^-1| to
first order (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 14.4: the forward error of GJE is that of
Gaussian elimination), with c_K = 3 K the constant of K steps of one division, one product and one difference each, applied to
both halves of [A | I]; | |L| |U| |_1 <= K rho |A|_1 with rho the growth factor of this elimination of this A: the largest entry of
the reduced matrices (rows and columns j .. K - 1 at the start of step j, which are Gaussian elimination's: a row is divided by
its pivot only when its step comes) over the largest entry of A, read off the restatement's own elimination (growth(); at most
2^(K - 1) under partial pivoting, and near 1 for membership rows).  Taking norms, every entry of X is within
        b = 8 K^2 rho u kappa_1(A) |A^-1|_1          (8 >= 2 x 3 for the two halves, and room for the second-order terms)
of the exact inverse, which the long-double elimination gives to 2^-11 of that.  rcond = 1 / (|A|_1 |X|_1): |X|_1 moves by at most
K b, so rcond by rcond K b / |A^-1|_1 (first order) plus three roundings.  z_min: every Z~[i, k] is a sum of K products of entries
in [0, 1] with entries of X, so it moves by at most K b + K u max|Z~ terms|; a minimum is 1-Lipschitz."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -52


def curve_rule(Z, perm=None):
    """curve[k] of the aligned components; Z (n, K)"""
    Z = np.asarray(Z)
    K = Z.shape[1]
    perm = np.arange(K) if perm is None else np.asarray(perm)
    out = np.zeros(K, dtype=np.int32)
    for k in range(K):
        col = Z[:, perm[k]].astype(np.float64)
        col = np.where(np.isnan(col), -np.inf, col)
        out[k] = int(np.argmax(col))              # the first maximum
    return out


def transform(Z, perm=None):
    """(A, curve): A[k, c] = Z[curve[k], c], float64 copies"""
    cv = curve_rule(Z, perm)
    return np.ascontiguousarray(np.asarray(Z, dtype=np.float64)[cv, :]), cv


def _eliminate(A, dtype):
    """(Ainv, singular, rho) by the device's Gauss-Jordan order in `dtype`; rho: the growth factor, the largest entry of the reduced
    matrices over the largest of A"""
    A = np.asarray(A)
    K = A.shape[0]
    if not np.all(np.isfinite(A.astype(np.float64))):
        return np.full((K, K), np.nan, dtype=dtype), True, np.nan
    m = np.concatenate([A.astype(dtype), np.eye(K, dtype=dtype)], axis=1)
    top = big0 = float(np.max(np.abs(m[:, :K])))
    for j in range(K):
        top = max(top, float(np.max(np.abs(m[j:, j:K]))))
        p = j
        big = abs(m[j, j])
        for r in range(j + 1, K):
            if abs(m[r, j]) > big:
                big, p = abs(m[r, j]), r
        piv = m[p, j]
        if piv == 0 or piv != piv:
            return np.full((K, K), np.nan, dtype=dtype), True, np.nan
        if p != j:
            m[[j, p]] = m[[p, j]]
        m[j] = m[j] / piv
        for r in range(K):
            if r != j:
                f = m[r, j]
                m[r] = m[r] - f * m[j]
    return m[:, K:].copy(), False, top / big0


def inverse(A, dtype=LD):
    """(Ainv, singular); singular: a zero pivot or a non-finite A, Ainv = NaN"""
    return _eliminate(A, dtype)[:2]


def growth(A):
    return _eliminate(A, LD)[2]


def norm1(A):
    return np.max(np.sum(np.abs(A), axis=0))


def rcond(A, Ainv):
    if not np.all(np.isfinite(np.asarray(Ainv, dtype=np.float64))):
        return 0.0
    return 1.0 / (norm1(np.asarray(A, dtype=LD)) * norm1(np.asarray(Ainv, dtype=LD)))


def z_tilde(Z, Ainv):
    return np.asarray(Z, dtype=LD) @ np.asarray(Ainv, dtype=LD)


def z_min(Z, Ainv):
    """the smallest rescaled membership; a NaN among them is kept, as the device keeps it"""
    zt = z_tilde(Z, Ainv)
    return np.nan if np.any(np.isnan(zt.astype(np.float64))) else zt.min()


def inverse_bound(A, Ainv):
    """the entrywise bound b of the module docstring, from the long-double inverse"""
    K = np.asarray(A).shape[0]
    n1, ni = float(norm1(np.asarray(A, dtype=LD))), float(norm1(np.asarray(Ainv, dtype=LD)))
    return 8.0 * K * K * growth(A) * U * (n1 * ni) * ni


def draw(Z, perm=None, given=None):
    """everything k_rescale_transform returns for one draw, the inverse in long double: dict(curve, A, Ainv, singular, rcond, z_min)"""
    if given is None:
        A, cv = transform(Z, perm)
    else:
        A, cv = np.ascontiguousarray(given, dtype=np.float64), np.full(np.asarray(given).shape[0], -1, dtype=np.int32)
    Ai, sing = inverse(A)
    if given is None and len(set(cv.tolist())) < len(cv):      # two components share their pure curve: two equal rows
        Ai, sing = np.full(A.shape, np.nan, dtype=LD), True
    return dict(curve=cv, A=A, Ainv=Ai, singular=sing, rcond=0.0 if sing else float(rcond(A, Ai)),
                z_min=np.nan if sing else float(z_min(Z, Ai)))


def mix(x, name, A, Ainv, dtype=LD):
    """one draw of `name` after the step: nu, Phi, eta, xi by A over their component axis, Z by Ainv"""
    x = np.asarray(x, dtype=dtype)
    if name == "Z":
        return x @ np.asarray(Ainv, dtype=dtype)
    A = np.asarray(A, dtype=dtype)
    if name in ("nu", "Phi"):
        return np.tensordot(A, x, axes=(1, 0))
    if name in ("eta", "xi"):
        return np.tensordot(x, A, axes=(x.ndim - 1, 1))
    raise ValueError(f"the reference defines no rescale for {name}")


def mix_abs(x, name, A, Ainv):
    """sum_c |w_c x_c| of every element of mix(): what its rounding bound K u sum_c |w_c x_c| scales with"""
    return mix(np.abs(np.asarray(x, dtype=LD)), name, np.abs(np.asarray(A, dtype=LD)), np.abs(np.asarray(Ainv, dtype=LD)))


def mean_values(E, nu, A, eta=None, x=None):
    """v[k, g] of one draw, and a[k, g] = sum_p |E_gp| sum_c |A[k][c]| (|nu| + sum_d |x_d eta|)"""
    E, nu, A = np.asarray(E, dtype=LD), np.asarray(nu, dtype=LD), np.asarray(A, dtype=LD)
    t, ta = nu.copy(), np.abs(nu)                                   # (K, P)
    if x is not None:
        ex = np.tensordot(np.asarray(eta, dtype=LD), np.asarray(x, dtype=LD), axes=(1, 0))      # (P, K)
        t = t + ex.T
        ta = ta + np.tensordot(np.abs(np.asarray(eta, dtype=LD)), np.abs(np.asarray(x, dtype=LD)), axes=(1, 0)).T
    return (A @ t) @ E.T, (np.abs(A) @ ta) @ np.abs(E).T


def cov_tables(E, Phi, A, xi=None, x=None):
    """W~[k, g, m] of one draw and its absolute companion"""
    E, Phi, A = np.asarray(E, dtype=LD), np.asarray(Phi, dtype=LD), np.asarray(A, dtype=LD)
    th, tha = Phi.copy(), np.abs(Phi)                               # (K, P, M)
    if x is not None:
        xi = np.asarray(xi, dtype=LD)                               # (P, D, M, K)
        xv = np.asarray(x, dtype=LD)
        th = th + np.einsum("pdmk,d->kpm", xi, xv)
        tha = tha + np.einsum("pdmk,d->kpm", np.abs(xi), np.abs(xv))
    W = np.einsum("gp,cpm->cgm", E, th)
    Wa = np.einsum("gp,cpm->cgm", np.abs(E), tha)
    return np.einsum("kc,cgm->kgm", A, W), np.einsum("kc,cgm->kgm", np.abs(A), Wa)


def cov_values(E1, E2, Phi, A, pairs, xi=None, x=None):
    """c[r, g, h] of one draw and a[r, g, h] = sum_m |W~1| |W~2|"""
    W1, W1a = cov_tables(E1, Phi, A, xi, x)
    W2, W2a = (W1, W1a) if E2 is None else cov_tables(E2, Phi, A, xi, x)
    c = np.stack([W1[k] @ W2[l].T for k, l in pairs])
    a = np.stack([W1a[k] @ W2a[l].T for k, l in pairs])
    return c, a
