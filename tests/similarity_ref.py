"""numpy restatement of the pooled co-membership of curves from chain slots (kernels_similarity.hip):

    d_ij(c, t) = sum_k Z_ik(c, t) Z_jk(c, t),    mean and two-pass sd (N - 1) over the N = C S draws, per-chain means

from get_chain("Z") copies (n, K, T) of every chain, and the tolerance a device result is held to.  The tolerance is derived,
not measured.  With u = 2^-52 and every term of every sum non-negative: each side's d carries at most (K + 1) u d of error,
summing N of them at most (N - 1) u sum d, and the sd is Lipschitz in the draws with constant sqrt(N / (N - 1)) in the
max-norm.  Device against the float64 restatement:

    |mean - mean_ref| <= 2 (N + K + 2) u mean_ref
    |sd - sd_ref|     <= 4 N u sd_ref + 4 (K + 1) u sqrt(N / (N - 1))

(chain_mean: the first line with S for N)."""
import numpy as np

U = 2.0 ** -52


def draws(chains, first, n_slots, curves=None, dtype=np.float64):
    """d of every draw: (m, n, C, S) from the chains' Z copies (n, K, T)"""
    sl = slice(first, first + n_slots)
    idx = slice(None) if curves is None else np.asarray(curves, dtype=np.int64)
    out = []
    for Z in chains:
        Zs = np.asarray(Z, dtype=dtype)[..., sl]
        out.append(np.einsum("iks,jks->ijs", Zs[idx], Zs))
    return np.stack(out, axis=2)


def summarise(d):
    """mean (m, n), two-pass sd (m, n; NaN for one draw) and per-chain means (m, C, n) of d (m, n, C, S)"""
    m, n, C, S = d.shape
    flat = d.reshape(m, n, C * S)
    mean = flat.mean(axis=-1)
    sd = np.full(mean.shape, np.nan) if C * S < 2 else flat.std(axis=-1, ddof=1)
    return mean, sd, np.ascontiguousarray(d.mean(axis=-1).transpose(0, 2, 1))


def similarity(chains, first, n_slots, curves=None):
    """what Sampler.similarity(sd=True, per_chain=True) returns"""
    mean, sd, cm = summarise(draws(chains, first, n_slots, curves))
    return {"mean": mean, "sd": sd, "chain_mean": cm}


def mean_bound(mean_ref, N, K):
    return 2.0 * (N + K + 2) * U * np.asarray(mean_ref, dtype=np.float64)


def sd_bound(sd_ref, N, K):
    return 4.0 * N * U * np.asarray(sd_ref, dtype=np.float64) + 4.0 * (K + 1) * U * np.sqrt(N / (N - 1.0))


def pair_moments(Zi, Zj, dtype=np.float64):
    """mean and two-pass sd of d over the draws of cases of one pair each: Zi, Zj (cases, N, K); numpy's own summation order"""
    d = np.einsum("cnk,cnk->cn", np.asarray(Zi, dtype=dtype), np.asarray(Zj, dtype=dtype))
    N = d.shape[1]
    mean = d.sum(axis=1) / dtype(N)
    q = ((d - mean[:, None]) ** 2).sum(axis=1)
    return mean, np.sqrt(q / dtype(N - 1))


def pair_moments_sequential(Zi, Zj):
    """the same in float64 with k in order and the draws in order, one addition at a time"""
    Zi, Zj = np.asarray(Zi, dtype=np.float64), np.asarray(Zj, dtype=np.float64)
    cases, N, K = Zi.shape
    d = np.zeros((cases, N))
    for k in range(K):
        d = d + Zi[:, :, k] * Zj[:, :, k]
    s = np.zeros(cases)
    for t in range(N):
        s = s + d[:, t]
    mean = s / float(N)
    q = np.zeros(cases)
    for t in range(N):
        e = d[:, t] - mean
        q = q + e * e
    return mean, np.sqrt(q / float(N - 1))


def pair_sd_one_pass(Zi, Zj):
    """the one-pass variance sum d^2 - (sum d)^2 / N in float64: what the device must not do"""
    d = np.einsum("cnk,cnk->cn", np.asarray(Zi, dtype=np.float64), np.asarray(Zj, dtype=np.float64))
    N = d.shape[1]
    s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)
    with np.errstate(invalid="ignore"):
        return np.sqrt((s2 - s1 * s1 / N) / (N - 1.0))
