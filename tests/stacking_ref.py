"""Restatement of the stacking of predictive distributions (kernels_stacking.hip, api.stacking, api.stack_models) in
np.longdouble: the prepare step, the EM fixed point with the device's stopping rule, the certificate and the pointwise values
(`em`, `evaluate`); the compare table of api.stack_models (`compare_table`); and two float64 twins of `em` that differ from each
other only in the order of the sum over rows, one forward and one a pairwise tree (`SUMS`), from which the GPU test takes its
bound (`weights_bound`).  `mutate` switches on the wrong forms tests/test_stacking_ref.py must be able to tell from the right one."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def sum_forward(A):
    """sum over rows of a float64 (n, Q) array, row after row"""
    return np.cumsum(A, axis=0)[-1]


def sum_pairwise(A):
    """the same sum as a balanced tree over neighbouring rows"""
    A = np.array(A)
    while A.shape[0] > 1:
        if A.shape[0] % 2:
            A = np.concatenate([A, np.zeros_like(A[:1])])
        A = A[0::2] + A[1::2]
    return A[0]


def sum_ld(A):
    return np.sum(A, axis=0)


SUMS = {"forward": (np.float64, sum_forward), "pairwise": (np.float64, sum_pairwise)}


def prepare(L, dtype=LD, mutate=None):
    """(m, P): the row maxima and exp(L - m); refuses what the entry point refuses, naming the first (unit, candidate)"""
    L = np.asarray(L, dtype=np.float64)
    bad = np.isnan(L) | (L == np.inf)
    bad[:, 0] |= np.all(L == -np.inf, axis=1)
    if bad.any():
        i, q = np.argwhere(bad)[0]
        raise ValueError(f"{int(bad.sum())} offending entries or units, the first at unit {i}, candidate {q}")
    Lx = L.astype(dtype)
    m = np.zeros(L.shape[0], dtype=dtype) if mutate == "no_row_max" else Lx.max(axis=1)
    with np.errstate(over="ignore", under="ignore"):
        P = np.exp(Lx - m[:, None])
    return m, P


def _terms(P, m, w):
    """d_i, the n x Q terms P_iq / d_i and the n terms m_i + log d_i; the sum over q runs in candidate order"""
    d = np.zeros(P.shape[0], dtype=P.dtype)
    for q in range(P.shape[1]):
        d = d + w[q] * P[:, q]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return d, P / d[:, None], m + np.log(d)


def evaluate(L, w, dtype=LD, row_sum=sum_ld):
    """f(w), gap(w) and the pointwise stacked log densities at the weights w"""
    m, P = prepare(L, dtype)
    w = np.asarray(w, dtype=dtype)
    d, R, l = _terms(P, m, w)
    n = dtype(P.shape[0])
    g = row_sum(R)
    return dict(objective=row_sum(l[:, None])[0], gap=np.max(g) / n - dtype(1), pointwise=l, g=g)


def em(L, init=None, max_iter=10000, check_every=16, tol=1e-8, dtype=LD, row_sum=sum_ld, mutate=None, snapshots=()):
    """The iteration of bfmmm_post_stacking.  Returns weights, pointwise, objective, gap, n_iter, converged, "history": (t, gap(w_t),
    f(w_t)) of every iterate the stopping rule looked at, and "snapshots": {t: w_t} for the requested t.
    mutate: "no_row_max" (P = exp(L)), "div_by_Q" (w g / Q), "gap_before" (the gap of the iterate before the returned one)."""
    m, P = prepare(L, dtype, mutate)
    n, Q = P.shape
    w = np.full(Q, dtype(1) / dtype(Q), dtype=dtype) if init is None else np.asarray(init, dtype=dtype)
    div = dtype(Q if mutate == "div_by_Q" else n)
    nd = dtype(n)
    hist, snaps = [], {}
    t, prev_gap = 0, None
    while True:
        d, R, l = _terms(P, m, w)
        g = row_sum(R)
        gap = np.max(g) / nd - dtype(1)
        f = row_sum(l[:, None])[0]
        if t in snapshots:
            snaps[t] = w.copy()
        shown = prev_gap if (mutate == "gap_before" and prev_gap is not None) else gap
        if t >= 1 and (t % check_every == 0 or t == max_iter):
            hist.append((t, shown, f))
            conv = bool(shown <= tol)
            if t == max_iter or (conv and tol > 0):
                return dict(weights=w, pointwise=l, objective=f, gap=shown, n_iter=t, converged=conv, history=hist, snapshots=snaps)
        prev_gap = gap
        w = w * g / div
        t += 1


def total_se(v, dtype=LD):
    v = np.asarray(v, dtype=dtype)
    n = len(v)
    s = np.sum(v)
    if n < 2:
        return s, dtype("nan")
    return s, np.sqrt(dtype(n) * np.sum((v - s / dtype(n)) ** 2) / dtype(n - 1))


def compare_table(L, mutate=None):
    """api.compare_table in long double.  mutate "unpaired": se_diff from the two columns' own variances"""
    L = np.asarray(L, dtype=LD)
    n, Q = L.shape
    tot = [total_se(L[:, q]) for q in range(Q)]
    elpd = np.array([t[0] for t in tot])
    se = np.array([t[1] for t in tot])
    best = int(np.argmax(elpd))
    diff, se_diff = np.zeros(Q, dtype=LD), np.zeros(Q, dtype=LD)
    for q in range(Q):
        if q != best:
            diff[q], se_diff[q] = total_se(L[:, q] - L[:, best])
            if mutate == "unpaired":
                se_diff[q] = np.sqrt(se[q] ** 2 + se[best] ** 2)
    e = np.exp(elpd - elpd[best])
    return dict(elpd=elpd, se=se, best=best, elpd_diff=diff, se_diff=se_diff, pseudo_bma=e / np.sum(e))


# ---- the cases of tests/test_gpu_stacking.py and their bound ------------------------------------------------------------------
SMALL_N = (1, 63, 64, 65, 255, 256, 257)
QS = (1, 2, 3, 8, 17, 64)
BIG_QS = (1, 8, 64)          # with the n just above one grid-stride pass
ITERS = (1, 2, 20)


def simulate(n, Q, seed):
    """(L, init): Q candidates of differing quality on n units.  Every case carries the edge inputs: a third of the rows offset by
    -1e5 and a third by +700, about 5 % of the entries -inf (never a whole row), and a start off the centre of the simplex in the
    odd-numbered cases (None: uniform)."""
    rng = np.random.default_rng(seed)
    L = -1.0 + rng.standard_normal((n, Q)) * rng.uniform(0.3, 1.5, size=Q) - rng.uniform(0.0, 0.5, size=Q)
    keep = rng.integers(0, Q, size=n)
    drop = rng.uniform(size=(n, Q)) < 0.05
    drop[np.arange(n), keep] = False
    L[drop] = -np.inf
    rows = np.arange(n)
    L[rows % 3 == 1] += -1e5
    L[rows % 3 == 2] += 700.0
    init = None
    if seed % 2:
        init = rng.uniform(0.2, 1.0, size=Q)
        init /= init.sum()
        init[np.argmax(init)] += 1.0 - init.sum()      # on the simplex to the last bit or two
    return L, init


def weights_bound(L, init, iters=ITERS):
    """{t: (w_ld at t iterations, the GPU test's bound on |w_device - w_ld|)}: 8 x the larger of the two float64 twins' largest
    |w - w_ld|, at least 64 eps.  8: the device's order of the row sum is a third order of the same family (grid-stride partials, a
    butterfly, a short forward sum) and its exp may differ from libm's by an ulp or two."""
    top = max(iters)
    ref = em(L, init, max_iter=top, tol=0.0, snapshots=iters)["snapshots"]
    tw = [em(L, init, max_iter=top, tol=0.0, dtype=dt, row_sum=fn, snapshots=iters)["snapshots"] for dt, fn in SUMS.values()]
    out = {}
    for t in iters:
        worst = max(float(np.max(np.abs(s[t].astype(LD) - ref[t]))) for s in tw)
        out[t] = (ref[t], max(8.0 * worst, 64.0 * EPS))
    return out
