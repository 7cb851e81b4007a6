"""CPU checks of the restatement of the label alignment (tests/align_ref.py): the float64 restatement within half
the derived bound of the long-double one with every draw decidable, on random memberships and on an oracle-run chain; exact ties
go to the lexicographically smallest permutation; the subset recursion the device runs returns what full enumeration returns."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import align_ref as R

NS = (5, 17, 61, 130, 515)
KS = (1, 2, 3, 5, 8)
CONCS = (0.05, 1.0, 50.0)


def _memberships(rng, n, K, conc):
    Z = rng.dirichlet(np.full(K, conc), size=n)
    Z = np.clip(Z, 1e-300, None)      # a concentration of 0.05 underflows some entries to 0 / 0 rows
    return Z / Z.sum(axis=1, keepdims=True)


def _check_pair(Z, Zref, label):
    """float64 against long double: same permutation, score within half the bound, decidable; returns the ratio to the bound"""
    n, K = Zref.shape
    p64, s64, _ = R.assign(R.gram(Z, Zref, np.float64))
    pld, sld, second = R.assign(R.gram(Z, Zref, np.longdouble))
    assert R.decidable(sld, second, n, K), label
    assert np.array_equal(p64, pld), label
    b = float(R.bound(float(sld), n, K))
    err = abs(float(np.longdouble(s64) - sld))
    assert err <= 0.5 * b, (label, err, b)
    return err / b if b > 0 else 0.0


@pytest.mark.parametrize("K", KS)
def test_float64_within_half_the_bound_and_every_draw_decidable(K):
    worst = 0.0
    for n in NS:
        for conc in CONCS:
            rng = np.random.default_rng(1000 * K + n + int(10 * conc))
            Zref = _memberships(rng, n, K, conc)
            for draw in range(4):
                # a noisy, relabelled copy of the pivot: the draws a sampler aligns
                Z = 0.7 * Zref + 0.3 * _memberships(rng, n, K, conc)
                Z = Z[:, rng.permutation(K)]
                worst = max(worst, _check_pair(Z, Zref, (n, K, conc, draw)))
    print(f"K={K}: worst |float64 - long double| / bound {worst:.3e}")


def test_oracle_chain_is_decidable():
    """draws of a chain the CPU oracle samples (n = 41, K = 3), aligned against its last draw"""
    import oracle_lib as O
    from gpu_parity import random_state
    from simdata import simulate_functional, truth_chain
    sim = simulate_functional(n=41, M=2, sigma_sq=0.01, seed=9)
    T = 6
    model, ch = truth_chain(sim, T)
    random_state(sim, ch, 7)
    O.run_sweeps(model, O.make_hyper(sim["K"]), ch, O.SWEEP_WARM, n_iter=T, seed=13, chain_id=2)
    Zc = np.array(ch.Z)
    assert Zc.shape == (41, 3, T)
    Zref = Zc[:, :, T - 1]
    worst = 0.0
    for t in range(T):
        for p in itertools.permutations(range(3)):
            worst = max(worst, _check_pair(Zc[:, list(p), t], Zref, (t, p)))
    perm, score, dec = R.align([Zc], Zref, 0, T)
    assert dec.all() and perm.shape == (1, T, 3)
    assert np.array_equal(perm[0, T - 1], [0, 1, 2])
    print(f"oracle chain: worst |float64 - long double| / bound {worst:.3e}")


def _exact_first_maximum(Z, Zref):
    """the lexicographically first maximiser in exact rational arithmetic"""
    K = Zref.shape[1]
    A = [[sum(Fraction(float(Z[i, c])) * Fraction(float(Zref[i, l])) for i in range(Z.shape[0])) for l in range(K)] for c in range(K)]
    best, bp = None, None
    for p in itertools.permutations(range(K)):
        s = sum(A[p[l]][l] for l in range(K))
        if best is None or s > best:
            best, bp = s, p
    return np.array(bp, dtype=np.int32)


def tied_cases():
    """memberships with entries in {0, 1/2, 1}: every product and sum is exact in fp64.  (Z, Zref, what is tied)"""
    rng = np.random.default_rng(5)
    out = []
    for n, K in ((5, 2), (17, 3), (61, 3), (130, 4), (61, 5)):
        hard = np.eye(K)[rng.integers(0, K, size=n)]
        soft = 0.5 * (np.eye(K)[rng.integers(0, K, size=n)] + np.eye(K)[rng.integers(0, K, size=n)])
        base = np.where(rng.uniform(size=(n, 1)) < 0.5, hard, soft)
        two = hard.copy()
        two[:, K - 1] = two[:, 0] = 0.5 * (hard[:, 0] + hard[:, K - 1])      # columns 0 and K - 1 equal, entries still in {0, 1/2, 1}
        out.append((base, two, f"n={n} K={K}: Zref with two equal columns"))
        out.append((two, base, f"n={n} K={K}: Z with two equal columns"))
        out.append((two, two, f"n={n} K={K}: both"))
    return out


def test_exact_ties_go_to_the_lexicographically_smallest_permutation():
    for Z, Zref, label in tied_cases():
        want = _exact_first_maximum(Z, Zref)
        for dtype in (np.float64, np.longdouble):
            A = R.gram(Z, Zref, dtype)
            p, s, second = R.assign(A)
            assert np.array_equal(p, want), (label, dtype)
            assert second is not None and s == second, label      # a tie indeed: another permutation has the same score
            pd, sd = R.assign_subsets(A)
            assert np.array_equal(pd, want) and sd == s, (label, dtype)
    # the smaller index first: with Zref's columns 0 and K - 1 equal and Z = the untied base, column 0 keeps the smaller label
    Z, Zref, _ = tied_cases()[3]
    p = R.assign(R.gram(Z, Zref))[0]
    assert p[0] < p[-1]


def test_subset_recursion_equals_enumeration():
    """400 random and tied matrices, K <= 6: the recursion's permutation and score are the enumeration's"""
    rng = np.random.default_rng(11)
    for case in range(400):
        K = 1 + case % 6
        if case % 2:
            A = rng.integers(0, 3, size=(K, K)).astype(np.float64) * 0.5      # many exact ties
        else:
            A = R.gram(_memberships(rng, 23, K, 1.0), _memberships(rng, 23, K, 1.0), np.float64)
        p, s, _ = R.assign(A)
        pd, sd = R.assign_subsets(A)
        assert np.array_equal(p, pd) and s == sd, (case, A)


def test_bound_and_relabel():
    assert R.bound(2.0, 61, 3) == (61 + 3 + 2) * 2.0 ** -52 * 2.0
    x = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)       # an (n, K, T) array
    perm = np.array([[0, 1, 2], [2, 0, 1], [1, 0, 2], [2, 1, 0]])
    y = R.relabel(x, "Z", perm, 3)
    for t in range(4):
        assert np.array_equal(y[:, :, t], x[:, perm[t], t])
    assert np.array_equal(R.relabel(x, "chi", perm, 3), x)
