"""numpy restatement of the label alignment against a pivot (k_align_gram in kernels_align.hip):

    A[c][l] = sum_i Z_ic Zref_il,    perm = argmax over all K! permutations p of sum_l A[p(l)][l],    score = that sum,

A in np.longdouble (or the dtype asked for), the permutations enumerated in lexicographic order and the first strict maximum
kept, and the tolerance a device result is held to.  The tolerance is derived, not tuned: with u = 2^-52 every product
Z_ic Zref_il is non-negative (memberships), so a sum of n of them in ANY order carries a relative error of at most
gamma_n = n u / (1 - n u) plus one rounding per product, and the K entries of a trace add at most K - 1 further roundings of
non-negative partial sums:

    |score - score_ref| <= gamma_{n + K} score <= bound(score, n, K) = (n + K + 2) u score.

A draw is DECIDABLE when the restatement's best and second-best scores (over all permutations) differ by more than the sum of
their bounds: then every summation order gives the same permutation, and only such draws are compared.  K = 1 is always
decidable."""
import itertools

import numpy as np

U = 2.0 ** -52


def gram(Z, Zref, dtype=np.longdouble):
    """A (K, K) = Z' Zref in dtype"""
    return np.asarray(Z, dtype=dtype).T @ np.asarray(Zref, dtype=dtype)


_PERMS = {}


def permutations(K):
    """the K! permutations in lexicographic order, (K!, K)"""
    if K not in _PERMS:
        _PERMS[K] = np.array(list(itertools.permutations(range(K))), dtype=np.int64).reshape(-1, K)
    return _PERMS[K]


def scores(A):
    """(the K! permutations in lexicographic order, the score of each as the right-nested sum A[p0][0] + (A[p1][1] + (..)))"""
    K = A.shape[0]
    perms = permutations(K)
    s = np.zeros(len(perms), dtype=A.dtype)
    for l in range(K - 1, -1, -1):
        s = A[perms[:, l], l] + s
    return perms, s


def assign(A):
    """(perm, score, second): the first strict maximum in lexicographic order, its score and the best score of any other
    permutation (None for K = 1)"""
    perms, sc = scores(A)
    best = int(np.argmax(sc))      # the first occurrence of the maximum
    second = None
    if len(perms) > 1:
        second = np.delete(sc, best).max()
    return perms[best].astype(np.int32), sc[best], second


def assign_subsets(A):
    """(perm, score) by the device's route: g[l][mask] = max over c in mask of A[c][l] + g[l + 1][mask \\ c] for l = K - 1 .. 0,
    then the permutation read off from l = 0 taking the smallest c that attains g[l][mask] exactly"""
    K = A.shape[0]
    full = (1 << K) - 1
    g = [dict() for _ in range(K + 1)]
    g[K][0] = A.dtype.type(0)
    for l in range(K - 1, -1, -1):
        for mask in range(full + 1):
            if bin(mask).count("1") != K - l:
                continue
            best = None
            for c in range(K):
                if mask >> c & 1:
                    v = A[c, l] + g[l + 1][mask ^ (1 << c)]
                    if best is None or v > best:
                        best = v
            g[l][mask] = best
    perm, mask = [], full
    for l in range(K):
        c = min(c for c in range(K) if mask >> c & 1 and A[c, l] + g[l + 1][mask ^ (1 << c)] == g[l][mask])
        perm.append(c)
        mask ^= 1 << c
    return np.array(perm, dtype=np.int32), g[0][full]


def bound(score, n, K):
    return (n + K + 2.0) * U * np.asarray(score, dtype=np.float64)


def decidable(score, second, n, K):
    if second is None:
        return True
    return bool(float(score - second) > float(bound(float(score), n, K) + bound(float(second), n, K)))


def align(chains, Zref, first, n_slots, dtype=np.longdouble):
    """perm (C, S, K) int32, score (C, S) float64 and decidable (C, S) bool of slots [first, first + n_slots) of the chains'
    Z copies (n, K, T) against Zref (n, K)"""
    C = len(chains)
    n, K = np.shape(Zref)
    perm = np.zeros((C, n_slots, K), dtype=np.int32)
    score = np.zeros((C, n_slots))
    dec = np.zeros((C, n_slots), dtype=bool)
    for q, Zc in enumerate(chains):
        for s in range(n_slots):
            p, sc, second = assign(gram(Zc[:, :, first + s], Zref, dtype))
            perm[q, s], score[q, s], dec[q, s] = p, float(sc), decidable(sc, second, n, K)
    return perm, score, dec


def relabel(x, name, perm_cs, K):
    """get_chain(name) copy x of one chain (draw shape + (T,), "tau": (T, K)) with the component axis of slot t relabelled by
    perm_cs[t] (T, K); arrays without a component axis come back as they are"""
    axis = {"nu": 0, "Phi": 0, "gamma": 0, "Z": 1, "pi": 0, "delta": 0, "A": 0, "eta": 2, "xi": 3, "gamma_xi": 3, "tau_eta": 0,
            "delta_xi": 0, "A_xi": 0}
    x = np.asarray(x)
    if name == "tau":
        return np.stack([x[t, perm_cs[t]] for t in range(x.shape[0])])
    if name not in axis:
        return x.copy()
    out = np.empty_like(x)
    for t in range(x.shape[-1]):
        out[..., t] = np.take(x[..., t], perm_cs[t], axis=axis[name])
    return out
