"""numpy restatement of the least-squares loss of every draw against the pooled co-membership matrix (DESIGN.md 7i;
k_similarity_loss in kernels_similarity.hip), on top of similarity_ref.draws:

    loss(c, t) = sum_i sum_j (d_ij(c, t) - m_ij)^2,    d_ij = sum_k Z_ik Z_jk,    m = the mean of d over the N = C S draws

over all n^2 ordered pairs, the diagonal included, from get_chain("Z") copies (n, K, T) of every chain, and the tolerance a
device result is held to.  The tolerance is derived, not measured.  With u = 2^-52, d and m in [0, 1] and every term of every
sum non-negative, each side's e = d - m carries at most

    delta = (2 N + 3 K + 7) u

of absolute error ((K + 1) u from d, (N + K + 1) u from m, one rounding of the difference, and as much again for the other
side, rounded up).  Each side then sums n^2 squares with relative error at most (n^2 + 2) u / 2, and by Cauchy-Schwarz over the
n^2 terms sum |e_a^2 - e_b^2| <= 2 delta sum |e| + n^2 delta^2 <= 2 n delta sqrt(loss) + n^2 delta^2.  Device against the float64
restatement:

    |loss - loss_ref| <= 2 [ (n^2 + 2) u loss_ref + 2 n delta sqrt(loss_ref) + n^2 delta^2 ]

for any summation order, an MFMA's internal one included."""
import numpy as np

import similarity_ref as SR

U = SR.U


def loss(chains, first, n_slots, dtype=np.float64):
    """loss (C, S) of every draw of slots [first, first + n_slots) of the chains' Z copies (n, K, T); numpy's own summation order"""
    d = SR.draws(chains, first, n_slots, dtype=dtype)      # (n, n, C, S)
    n, _, C, S = d.shape
    m = d.reshape(n, n, C * S).mean(axis=-1)
    e = d - m[:, :, None, None]
    return (e * e).sum(axis=(0, 1))


def loss_sequential(chains, first, n_slots):
    """the same in float64 one addition at a time: k in order, the draws in slot-then-chain order for m, the pairs in order"""
    Zs = np.stack([np.asarray(Z, dtype=np.float64)[..., first:first + n_slots] for Z in chains])      # (C, n, K, S)
    C, n, K, S = Zs.shape
    d = np.zeros((n, n, C, S))
    for k in range(K):
        zk = Zs[:, :, k, :]
        d = d + np.einsum("cis,cjs->ijcs", zk, zk)          # no index is summed: one product per entry
    m = np.zeros((n, n))
    for c in range(C):
        for s in range(S):
            m = m + d[:, :, c, s]
    m = m / float(C * S)
    out = np.zeros((C, S))
    for i in range(n):
        for j in range(n):
            e = d[i, j] - m[i, j]
            out = out + e * e
    return out


def delta(N, K):
    return (2.0 * N + 3.0 * K + 7.0) * U


def bound(loss_ref, n, N, K):
    L = np.asarray(loss_ref, dtype=np.float64)
    dl = delta(N, K)
    return 2.0 * ((n * n + 2.0) * U * L + 2.0 * n * dl * np.sqrt(L) + n * n * dl * dl)


def argmin(loss_cs):
    """(chain, slot offset) of the first minimum in (chain, slot) order"""
    c, s = np.unravel_index(int(np.argmin(loss_cs)), loss_cs.shape)
    return int(c), int(s)


def two_smallest_are_apart(loss_cs, n, K):
    """the condition under which the argmin is decided: the two smallest losses differ by more than the sum of their bounds"""
    C, S = loss_cs.shape
    v = np.sort(loss_cs.reshape(-1))
    b = bound(v[:2], n, C * S, K)
    return bool(v[1] - v[0] > b[0] + b[1]), float((v[1] - v[0]) / (b[0] + b[1]))
