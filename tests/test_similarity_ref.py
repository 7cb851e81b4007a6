"""CPU checks of the restatement the device tests of the pooled co-membership matrix compare with (tests/similarity_ref.py;
DESIGN.md 7f): its float64 form and a sequential-order form against np.longdouble within half of the derived bounds, on 2000
random pairs of membership rows; a one-pass variance breaks the sd bound on nearly constant rows (so the device test can tell
the two methods apart); invariance under a relabelling of one chain; and the new entry of the C ABI."""
import os
import re

import numpy as np
import pytest

import similarity_ref as R

KS = range(2, 9)
NS = (2, 3, 23, 92, 500, 4000)
KINDS = ("dirichlet 0.05", "dirichlet 1", "dirichlet 50", "exact zeros", "nearly constant")


def _cases(K, N, count, rng):
    """count pairs of membership rows over N draws: Zi, Zj (count, N, K) and the kind of each case"""
    kind = np.arange(count) % len(KINDS)
    Zi, Zj = np.empty((count, N, K)), np.empty((count, N, K))
    for c in range(count):
        if kind[c] < 3:
            a = (0.05, 1.0, 50.0)[kind[c]]
            Zi[c], Zj[c] = rng.dirichlet(np.full(K, a), size=N), rng.dirichlet(np.full(K, a), size=N)
        elif kind[c] == 3:
            for Zx in (Zi, Zj):
                Zx[c] = rng.dirichlet(np.ones(K), size=N)
                Zx[c][rng.uniform(size=(N, K)) < 0.3] = 0.0
        else:      # a fixed membership plus 1e-6 noise, i = j
            Zi[c] = np.abs(rng.dirichlet(np.ones(K))[None, :] + 1e-6 * rng.standard_normal((N, K)))
            Zj[c] = Zi[c]
    return Zi, Zj, kind


def test_restatements_within_half_the_bounds_and_one_pass_variance_is_not():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    rng = np.random.default_rng(20)
    groups = [(K, N) for K in KS for N in NS]
    total, worst = 0, {"mean": 0.0, "sd": 0.0}
    broke, flat = 0, 0
    for g, (K, N) in enumerate(groups):
        count = 2000 // len(groups) + (1 if g < 2000 % len(groups) else 0)
        total += count
        Zi, Zj, kind = _cases(K, N, count, rng)
        mean_x, sd_x = R.pair_moments(Zi, Zj, dtype=np.longdouble)
        bm = R.mean_bound(mean_x.astype(np.float64), N, K)
        bs = R.sd_bound(sd_x.astype(np.float64), N, K)
        for label, (mean, sd) in (("float64", R.pair_moments(Zi, Zj)), ("sequential", R.pair_moments_sequential(Zi, Zj))):
            em = np.abs(mean.astype(np.longdouble) - mean_x).astype(np.float64)
            es = np.abs(sd.astype(np.longdouble) - sd_x).astype(np.float64)
            assert np.all(em <= 0.5 * bm), (label, K, N, float(np.max(em[bm > 0] / bm[bm > 0])))
            assert np.all(es <= 0.5 * bs), (label, K, N, float(np.max(es / bs)))
            if np.any(bm > 0):
                worst["mean"] = max(worst["mean"], float(np.max(em[bm > 0] / bm[bm > 0])))
            worst["sd"] = max(worst["sd"], float(np.max(es / bs)))
        if N >= 23:
            nc = kind == 4
            one = R.pair_sd_one_pass(Zi[nc], Zj[nc])
            e1 = np.abs(one.astype(np.longdouble) - sd_x[nc]).astype(np.float64)
            broke += int(np.count_nonzero(~(e1 <= bs[nc])))          # (a negative variance, NaN, breaks it too)
            flat += int(np.count_nonzero(nc))
    assert total == 2000
    print(f"worst error / full bound over {total} cases: mean {worst['mean']:.3f}, sd {worst['sd']:.3f}; "
          f"one-pass variance outside the sd bound on {broke} of {flat} nearly constant rows of 23 draws or more")
    assert flat >= 200 and broke > 0.9 * flat


def test_relabelling_one_chain_leaves_the_restatement_within_its_bounds():
    rng = np.random.default_rng(6)
    n, K, T, first, S = 9, 5, 14, 3, 11
    chains = [np.ascontiguousarray(rng.dirichlet(np.full(K, 0.7), size=(n, T)).transpose(0, 2, 1)) for _ in range(3)]
    a = R.similarity(chains, first, S)
    perm = [3, 0, 4, 1, 2]
    b = R.similarity([chains[0], np.ascontiguousarray(chains[1][:, perm]), chains[2]], first, S)
    N = 3 * S
    assert np.all(np.abs(a["mean"] - b["mean"]) <= R.mean_bound(a["mean"], N, K))
    assert np.all(np.abs(a["sd"] - b["sd"]) <= R.sd_bound(a["sd"], N, K))
    assert np.all(np.abs(a["chain_mean"] - b["chain_mean"]) <= R.mean_bound(a["chain_mean"], S, K))
    # and it is the labels of Z itself that differ: chain 1's Z does not survive the relabelling
    assert not np.array_equal(chains[1], chains[1][:, perm])
    # shapes, selection and the diagonal
    sel = [4, 0, 0, 8]
    s = R.similarity(chains, first, S, curves=sel)
    assert s["mean"].shape == (4, n) and s["sd"].shape == (4, n) and s["chain_mean"].shape == (4, 3, n)
    for k in ("mean", "sd", "chain_mean"):
        assert np.array_equal(s[k], a[k][sel])
    Zs = np.stack([Z[..., first:first + S] for Z in chains])          # (C, n, K, S)
    np.testing.assert_allclose(np.diag(a["mean"]), (Zs ** 2).sum(axis=2).mean(axis=(0, 2)), rtol=1e-14)
    one = R.summarise(R.draws(chains[:1], 2, 1))
    assert np.all(np.isnan(one[1])) and np.array_equal(one[0], R.draws(chains[:1], 2, 1)[:, :, 0, 0])


def test_new_symbol_is_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    declared = set(re.findall(r"\b(bfmmm_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ("bfmmm_chain_similarity", "bfmmm_set_similarity_block"):
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
