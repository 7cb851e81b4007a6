"""numpy restatement of the cluster eigenvalues and eigenfunctions of chain slots under aligned labels (DESIGN.md 7l;
kernels_cluster_eig.hip):

    theta_km = phi_{perm[k], m} + sum_d x_d xi_{perm[k], m, d}                 (cluster_cov_ref.aligned_theta)
    Q        = E' diag(w) E,   S_k = Theta_k' Q Theta_k = V diag(lambda) V'     (lambda descending, ties in index order, >= 0)
    total_k  = trace S_k,   pve_kj = lambda_kj / total_k                        (0 where total_k == 0)
    b_kj     = Theta_k v_j / sqrt(lambda_kj)                                    (0 where lambda_kj <= M 2^-53 lambda_k1)
    psi_kj   = sgn_kj E b_kj,   sgn_kj = +1 if b_kj . (E' diag(w) ref_kj) >= 0 else -1
               (ref None: the sign of the entry of largest sqrt(w_g) |E_g . b_kj|, lowest g first on ties)

from get_chain copies, a permutation row per draw, E, w, x and ref, with the kernel's Jacobi iteration: round-robin pairs (with n =
M rounded up to even, round r pairs (r, n - 1) and ((r + i) mod (n - 1), (r - i) mod (n - 1)), a pair holding the index M a
bye), every pair of a round rotated from the matrix at the round's start (columns of S and V, then rows of S, then s_pp - t s_pq,
s_qq + t s_pq and exact zeros), a pair skipped when |s_pq| <= u max(sqrt(|s_pp s_qq|), u ||S||_F of the start), u = 2^-53, a
stop after a sweep without a rotation and a cap of 40 sweeps.  Every function runs in numpy.longdouble (the reference) and in
float64 (`dtype`).

Bounds.  bound_S is counted, entry by entry, against A = |Theta|' |Q| |Theta|, |Q| = |E|' diag(w) |E|: a term theta_pi E_gp w_g
E_gp2 theta_p2j of S_ij carries D + 1 roundings in either theta (D products and additions; 0 without x), G + 2 in Q (the two
products and at most G additions), P + 1 in Q Theta and P + 1 in Theta' (Q Theta), whatever the order of the sums and fewer where
a product is fused, as in an MFMA's chained accumulation.  That is G + 2 P + 2 D + 6 roundings of 2^-53, and with 2 added for what
first order leaves out and for the long-double reference's own error (the allowance of tests/cluster_cov_ref.py)

    |S^ - S| <= c_S 2^-52 A,   c_S = (G + 2 P + 2 D + 6) / 2 + 2
    |lambda^_j - lambda_j| <= ||bound_S||_F + C_J 2^-53 ||S||_F                (Weyl, and the Jacobi iteration's own error)
    |total^ - total| <= sum_i bound_S[i][i] + M 2^-52 sum_i A[i][i]             (M - 1 additions)
    |pve^ - pve| <= (b_lambda + pve b_total) / (total - b_total) + 2^-52 pve    (one division)

and for the returned eigenfunctions, with A_E = E Theta_k and S of the long-double run, kappa_j = lambda^_1 / lambda^_j and the
w-weighted norm, conditions that need no eigenvalue gap:

    residual       ||A_E A_E' (w o psi^_j) - lambda^_j psi^_j||_w <= sqrt(kappa_j) (C_PSI 2^-53 ||S||_F + ||bound_S||_F)
    orthonormality |<psi^_i, psi^_j>_w - delta_ij| <= C_O 2^-53 sqrt(kappa_i kappa_j)
    sign           <psi^_j, ref_j>_w >= -(C_O 2^-53 kappa_j ||ref_j||_w + (G + 2 P + 4) 2^-52 sum_g w_g (|E| |b_j|)_g |ref_j(g)|)
                   (the second term: the roundings of R, of b . R and of E b that stand between the kernel's test and this one)
    zero rule      psi^_j == 0 exactly where lambda_j <= M 2^-53 lambda_1 in the run that produced it

(the residual: with x = S v^ - lambda^ v^, the residual is A_E x / sqrt(lambda^_j) and ||A_E x||_w <= sqrt(lambda_1) ||x||).
C_J, C_PSI and C_O cannot be counted that way.  They are fixed from the float64 run of this module against its long-double run on
the inputs of tests/test_cluster_eig_ref.py (`cases`; random Theta, E, w, x in the shapes of the GPU tests), the worst ratio
times 4 and rounded up: the device's sqrt and division, its order within the fixed scheme and its sums may round differently from
numpy's.  Never from device output.  Measured worst ratios of the float64 run (`check`'s "lam_units", "resid_units" and
"orth_units": the eigenvalue error over 2^-53 ||S||_F, the residual over sqrt(kappa_j) 2^-53 ||S||_F, the orthonormality defect over
2^-53 sqrt(kappa_i kappa_j)): 44.3, 44.3 and 54.7; so C_J = 180, C_PSI = 180, C_O = 220.  The float64 run took at most 13 sweeps
(the rank-9 case at M = 16), 6 at most elsewhere."""
import numpy as np

import cluster_cov_ref as CR

U = 2.0 ** -53
CAP = 40
C_J = 180.0
C_PSI = 180.0
C_O = 220.0
LD = np.longdouble


def c_S(P, G, D):
    return (G + 2 * P + 2 * D + 6) / 2.0 + 2.0


def rr_pairs(M):
    """the rounds of a sweep: a list of lists of pairs (p, q), p < q < M (byes dropped)"""
    n = (M + 1) & ~1
    out = []
    for r in range(n - 1):
        rnd = []
        for i in range(n // 2):
            a = r if i == 0 else (r + i) % (n - 1)
            b = n - 1 if i == 0 else (r - i + (n - 1)) % (n - 1)
            p, q = min(a, b), max(a, b)
            if q < M:
                rnd.append((p, q))
        out.append(rnd)
    return out


def gram(E, w, dtype=np.float64, absolute=False):
    """Q = sum_g (E_gp w_g) E_gp2, g in order from 0"""
    Ef = np.abs(np.asarray(E, dtype=dtype)) if absolute else np.asarray(E, dtype=dtype)
    G, P = Ef.shape
    wf = np.ones(G, dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
    Q = np.zeros((P, P), dtype=dtype)
    for g in range(G):
        Q = Q + (Ef[g] * wf[g])[:, None] * Ef[g][None, :]
    return Q


def form_S(Q, Th):
    """S (B, M, M) = Theta' (Q Theta) of Theta (B, P, M), in the dtype of its arguments"""
    Y = np.einsum("pr,brm->bpm", Q, Th)
    return np.einsum("bpi,bpj->bij", Th, Y)


def jacobi(S0):
    """the kernel's iteration on S0 (B, M, M), in its dtype: (diagonal (B, M), V (B, M, M), sweeps (B,), capped (B,))"""
    S = np.array(S0, copy=True)
    dt = S.dtype.type
    B, M = S.shape[:2]
    iu = np.triu_indices(M, 1)
    S[:, iu[1], iu[0]] = S[:, iu[0], iu[1]]                      # only the upper triangle is read
    V = np.broadcast_to(np.eye(M, dtype=S.dtype), S.shape).copy()
    u = dt(U)
    dg = np.einsum("bii->bi", S)
    fro2 = np.sum(dg * dg, axis=1) + dt(2) * np.sum(S[:, iu[0], iu[1]] ** 2, axis=1)
    ufro = u * np.sqrt(fro2)
    sweeps = np.zeros(B, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    capped = np.zeros(B, dtype=bool)
    rounds = rr_pairs(M)
    for sweep in range(1, CAP + 1):
        rot = np.zeros(B, dtype=bool)
        for rnd in rounds:
            if not rnd:
                continue
            ps = np.array([p for p, _ in rnd])
            qs = np.array([q for _, q in rnd])
            app, aqq, apq = S[:, ps, ps], S[:, qs, qs], S[:, ps, qs]
            act = np.abs(apq) > u * np.maximum(np.sqrt(np.abs(app * aqq)), ufro[:, None])
            if not act.any():
                continue
            rot |= act.any(axis=1)
            safe = np.where(act, apq, dt(1))
            tau = (aqq - app) / (dt(2) * safe)
            t = np.where(tau >= 0, dt(1), dt(-1)) / (np.abs(tau) + np.sqrt(dt(1) + tau * tau))
            c = dt(1) / np.sqrt(dt(1) + t * t)
            s = t * c
            c = np.where(act, c, dt(1))
            s = np.where(act, s, dt(0))
            npp, nqq = app - t * apq, aqq + t * apq
            cc, ss = c[:, None, :], s[:, None, :]
            x0, x1 = S[:, :, ps], S[:, :, qs]
            S[:, :, ps], S[:, :, qs] = cc * x0 - ss * x1, ss * x0 + cc * x1
            v0, v1 = V[:, :, ps], V[:, :, qs]
            V[:, :, ps], V[:, :, qs] = cc * v0 - ss * v1, ss * v0 + cc * v1
            cr, sr = c[:, :, None], s[:, :, None]
            x0, x1 = S[:, ps, :], S[:, qs, :]
            S[:, ps, :], S[:, qs, :] = cr * x0 - sr * x1, sr * x0 + cr * x1
            S[:, ps, ps] = np.where(act, npp, S[:, ps, ps])
            S[:, qs, qs] = np.where(act, nqq, S[:, qs, qs])
            S[:, ps, qs] = np.where(act, dt(0), S[:, ps, qs])
            S[:, qs, ps] = np.where(act, dt(0), S[:, qs, ps])
        sweeps[live] = sweep
        live &= rot
        if not live.any():
            break
    capped = live.copy()
    return np.einsum("bii->bi", S).copy(), V, sweeps, capped


def largest_entry_sign(psi, w):
    """+1 / -1 per function of psi (..., G): the sign of the entry of largest sqrt(w) |psi|, lowest g first"""
    a = np.abs(psi) if w is None else np.sqrt(np.asarray(w, dtype=psi.dtype)) * np.abs(psi)
    g = np.argmax(a, axis=-1)                                      # the first of several
    v = np.take_along_axis(psi, g[..., None], axis=-1)[..., 0]
    return np.where(v >= 0, 1.0, -1.0).astype(psi.dtype)


def solve(Th, E, w=None, ref=None, J=None, dtype=np.float64):
    """One component's draws: Theta (B, P, M), E (G, P), w (G) or None, ref (J, G) or None.  Returns a dict of lam (B, M), total
    (B,), pve (B, M), b (B, J, P), psi (B, J, G), zero (B, J), sweeps (B,), capped (B,), S (B, M, M), all in `dtype`."""
    Th = np.asarray(Th, dtype=dtype)
    Ef = np.asarray(E, dtype=dtype)
    B, P, M = Th.shape
    J = M if J is None else J
    dt = Th.dtype.type
    Q = gram(Ef, w, dtype)
    S = form_S(Q, Th)
    total = np.zeros(B, dtype=dtype)
    for i in range(M):
        total = total + S[:, i, i]
    dg, V, sweeps, capped = jacobi(S)
    # descending, ties in index order
    order = np.argsort(-dg, axis=1, kind="stable")
    lam = np.maximum(np.take_along_axis(dg, order, axis=1), dt(0))
    pve = np.where(total[:, None] == 0, dt(0), lam / np.where(total == 0, dt(1), total)[:, None])
    Vs = np.take_along_axis(V, order[:, None, :], axis=2)[:, :, :J]                  # (B, M, J)
    zero = ~(lam[:, :J] > dt(M) * dt(U) * lam[:, :1])
    b = np.einsum("bpm,bmj->bjp", Th, Vs) / np.sqrt(np.where(zero, dt(1), lam[:, :J]))[:, :, None]
    b = np.where(zero[:, :, None], dt(0), b)
    psi = np.einsum("gp,bjp->bjg", Ef, b)
    if J > 0:
        if ref is not None:
            wf = np.ones(Ef.shape[0], dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
            R = np.einsum("gp,g,jg->jp", Ef, wf, np.asarray(ref, dtype=dtype))
            sg = np.where(np.einsum("bjp,jp->bj", b, R) >= 0, dt(1), dt(-1))
        else:
            sg = largest_entry_sign(psi, w)
        b, psi = b * sg[:, :, None], psi * sg[:, :, None]
    return dict(lam=lam, total=total, pve=pve, b=b, psi=psi, zero=zero, sweeps=sweeps, capped=capped, S=S)


def bound_S(Th, E, w, D):
    """c_S 2^-52 |Theta|' |Q| |Theta| (B, M, M) and the absolute-valued form itself"""
    G, P = np.shape(E)
    A = form_S(gram(E, w, LD, absolute=True), np.abs(np.asarray(Th, dtype=LD)))
    return LD(c_S(P, G, D) * 2.0 ** -52) * A, A


def check(got, Th, E, w=None, ref=None, D=0, ref_rule=None, extra_S=None):
    """The conditions of the module docstring on `got` (lam (B, M), total (B,), pve (B, M), psi (B, J, G): a device result or the
    float64 run) against the long-double run of Theta (B, P, M).  ref (J, G): the sign condition against it; ref_rule "largest":
    the largest-entry rule instead.  Returns the worst ratio to each bound (all must be <= 1), the exact-zero verdict and the
    long-double run.  extra_S (B,): a further perturbation of S in the Frobenius norm that the caller accounts for, added to
    ||bound_S||_F."""
    Th = np.asarray(Th, dtype=np.float64)
    B, P, M = Th.shape
    psi = np.asarray(got["psi"], dtype=LD)
    J = psi.shape[1]
    G = np.shape(E)[0]
    ld = solve(Th, E, w, ref, J, LD)
    assert not ld["capped"].any()
    bS, A = bound_S(Th, E, w, D)
    nbS = np.sqrt(np.sum(bS * bS, axis=(1, 2)))
    if extra_S is not None:
        nbS = nbS + np.asarray(extra_S, dtype=LD)
    nS = np.sqrt(np.sum(ld["S"] ** 2, axis=(1, 2)))
    out = {}

    def ratio(err, bnd):
        err, bnd = np.broadcast_arrays(np.asarray(err, dtype=LD), np.asarray(bnd, dtype=LD))
        bad = (bnd == 0) & (err != 0)
        r = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), 0)
        return float("inf") if bad.any() else float(np.max(r, initial=0.0))

    lam = np.asarray(got["lam"], dtype=LD)
    b_lam = nbS + LD(C_J * U) * nS
    out["lam"] = ratio(np.abs(lam - ld["lam"]), b_lam[:, None])
    out["lam_units"] = ratio(np.abs(lam - ld["lam"]), (LD(U) * nS)[:, None])
    dA = np.einsum("bii->b", A)
    b_tot = np.einsum("bii->b", bS) + LD(M * 2.0 ** -52) * dA
    if extra_S is not None:
        b_tot = b_tot + np.sqrt(LD(M)) * np.asarray(extra_S, dtype=LD)
    out["total"] = ratio(np.abs(np.asarray(got["total"], dtype=LD) - ld["total"]), b_tot)
    den = ld["total"] - b_tot
    b_pve = np.where(den[:, None] > 0, (b_lam[:, None] + ld["pve"] * b_tot[:, None]) / np.where(den > 0, den, 1)[:, None], np.inf) + \
        LD(2.0 ** -52) * ld["pve"]
    b_pve = np.where(ld["total"][:, None] == 0, 0, b_pve)
    out["pve"] = ratio(np.abs(np.asarray(got["pve"], dtype=LD) - ld["pve"]), b_pve)
    out["sum"] = ratio(np.abs(np.sum(lam, axis=1) - ld["total"]), M * b_lam + b_tot)
    if J == 0:
        return out, True, ld
    Ef = np.asarray(E, dtype=LD)
    wf = np.ones(G, dtype=LD) if w is None else np.asarray(w, dtype=LD)
    AE = np.einsum("gp,bpm->bgm", Ef, np.asarray(Th, dtype=LD))                     # (B, G, M)
    lj = lam[:, :J]
    zero = ~(lj > LD(M * U) * lam[:, :1])
    kap = np.where(zero, 1, lam[:, :1] / np.where(zero, 1, lj))                     # (B, J)
    wpsi = wf[None, None, :] * psi
    res = np.einsum("bgm,bjm->bjg", AE, np.einsum("bgm,bjg->bjm", AE, wpsi)) - lj[:, :, None] * psi
    nres = np.sqrt(np.einsum("g,bjg->bj", wf, res * res))
    live = ~zero
    out["resid"] = ratio(np.where(live, nres, 0), np.sqrt(kap) * (LD(C_PSI * U) * nS + nbS)[:, None])
    out["resid_units"] = ratio(np.where(live, nres, 0), np.sqrt(kap) * (LD(U) * nS)[:, None])
    gr = np.einsum("big,bjg->bij", wpsi, psi)
    both = live[:, :, None] & live[:, None, :]
    dev = np.abs(gr - np.eye(J, dtype=LD)[None])
    kk = np.sqrt(kap[:, :, None] * kap[:, None, :])
    out["orth"] = ratio(np.where(both, dev, 0), LD(C_O * U) * kk)
    out["orth_units"] = ratio(np.where(both, dev, 0), LD(U) * kk)
    exact_zero = bool(np.all(psi[zero] == 0))
    if ref is not None:
        rf = np.asarray(ref, dtype=LD)
        ip = np.einsum("bjg,jg->bj", wpsi, rf)
        nref = np.sqrt(np.einsum("g,jg->j", wf, rf * rf))
        absb = np.einsum("gp,bjp->bjg", np.abs(Ef), np.abs(ld["b"]))
        sb = LD(C_O * U) * kap * nref[None, :] + LD((G + 2 * P + 4) * 2.0 ** -52) * np.einsum("g,bjg,jg->bj", wf, absb, np.abs(rf))
        out["sign"] = ratio(np.where(live, np.maximum(-ip, 0), 0), sb)
    elif ref_rule == "largest":
        g64 = np.asarray(got["psi"], dtype=np.float64)
        out["sign"] = 0.0 if np.all(largest_entry_sign(g64, w)[live] == 1.0) else float("inf")
    return out, exact_zero, ld


def thetas(chains, perm, first, n_slots, x=None):
    """Theta (K, N, P, M) of every aligned component and draw, N = C S chain-major, float64, from the get_chain copies"""
    sl = slice(first, first + n_slots)
    out = []
    for q, ch in enumerate(chains):
        kw = dict(xi=ch["xi"][..., sl], x=x) if x is not None else {}
        out.append(CR.aligned_theta(ch["Phi"][..., sl], perm[q], **kw))                # (K, P, M, S)
    return np.ascontiguousarray(np.transpose(np.concatenate(out, axis=-1), (0, 3, 1, 2)))


def cases():
    """random inputs in the shapes of tests/test_gpu_cluster_eig.py: (label, Theta (B, P, M), E, w, ref, D)"""
    rng = np.random.default_rng(20)
    out = []

    def one(label, B, P, M, G, w=None, D=0, ident=False, rank=None, with_ref=True):
        Th = rng.standard_normal((B, P, M)) * np.exp(-0.7 * np.arange(M))[None, None, :]
        if D:                                                    # theta = phi + sum_d x_d xi_d, formed as the kernel forms it
            xv = rng.standard_normal(D)
            for d in range(D):
                Th = Th + xv[d] * (0.3 * rng.standard_normal((B, P, M)))
        if rank is not None:
            Th[:, :, rank:] = Th[:, :, :rank] @ rng.standard_normal((rank, M - rank))
        E = np.eye(P) if ident else rng.standard_normal((G, P))
        ref = rng.standard_normal((M, E.shape[0])) if with_ref else None
        out.append((label, Th, E, w, ref, D))

    for G in (1, 7, 16, 17, 65):
        one(f"(a) M=2 G={G}", 24, 9, 2, G, w=None if G % 2 else rng.uniform(0.1, 2.0, G))
    wz = rng.uniform(0.1, 2.0, 17)
    wz[4] = 0.0
    one("(a) M=2 G=17, a zero weight", 24, 9, 2, 17, w=wz)
    one("(b) M=5 P=5", 24, 5, 5, 7, w=rng.uniform(0.1, 2.0, 7))
    one("(b) M=5 P=5, no ref", 24, 5, 5, 17, with_ref=False)
    one("(b) M=1 P=5", 24, 5, 1, 7)
    one("(c) M=16 P=64 E=I", 12, 64, 16, 64, ident=True)
    one("(c) M=16 P=64 E=I, rank 9", 12, 64, 16, 64, ident=True, rank=9)
    one("(d) D=2", 24, 9, 2, 16, w=rng.uniform(0.1, 2.0, 16), D=2)
    one("README shape P=30 M=6 G=48", 12, 30, 6, 48, w=np.full(48, 1.0 / 48))
    return out
