"""CPU checks of the restatement the device tests of the least-squares loss compare with (tests/similarity_loss_ref.py; DESIGN.md
7i): its float64 form and a sequential-order form (k in order, draws in slot-then-chain order for the mean, pairs in order for
the loss) against an np.longdouble evaluation within half of the derived bound, on n in {5, 17, 61, 130} x K in {2, 3, 5, 8} x
(C, S) in {(1, 1), (1, 2), (4, 23), (2, 200)} x Dirichlet concentrations 0.05 (every third row an exact vertex), 1 and 50; and
that on every case with more than two draws the two smallest losses are further apart than the sum of their bounds, so that
the argmin condition of the device test excludes nothing on such inputs."""
import numpy as np
import pytest

import similarity_loss_ref as R

NS = (5, 17, 61, 130)
KS = (2, 3, 5, 8)
CSS = ((1, 1), (1, 2), (4, 23), (2, 200))
CONCS = (0.05, 1.0, 50.0)


def _chains(n, K, C, S, conc, rng):
    out = []
    for _ in range(C):
        Z = rng.dirichlet(np.full(K, conc), size=(n, S))      # (n, S, K)
        if conc < 0.1:
            v = np.eye(K)[rng.integers(0, K, size=(len(range(0, n, 3)), S))]
            Z[::3] = v
        out.append(np.ascontiguousarray(Z.transpose(0, 2, 1)))
    return out


@pytest.mark.parametrize("n", NS)
def test_restatements_within_half_the_bound_of_long_double(n):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    rng = np.random.default_rng(70 + n)
    worst = {"float64": 0.0, "sequential": 0.0}
    gap = np.inf
    for K in KS:
        for C, S in CSS:
            for conc in CONCS:
                chains = _chains(n, K, C, S, conc, rng)
                N = C * S
                exact = R.loss(chains, 0, S, dtype=np.longdouble)
                b = R.bound(exact.astype(np.float64), n, N, K)
                assert np.all(b > 0)
                for label, got in (("float64", R.loss(chains, 0, S)), ("sequential", R.loss_sequential(chains, 0, S))):
                    err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
                    ratio = float(np.max(err / b))
                    assert np.all(err <= 0.5 * b), (label, n, K, C, S, conc, ratio)
                    worst[label] = max(worst[label], ratio)
                if N == 1:
                    assert R.loss(chains, 0, S)[0, 0] == 0.0
                if N > 2:
                    apart, ratio = R.two_smallest_are_apart(R.loss(chains, 0, S), n, K)
                    assert apart, (n, K, C, S, conc, ratio)
                    gap = min(gap, ratio)
    print(f"n={n}: worst error / full bound: float64 {worst['float64']:.4f}, sequential {worst['sequential']:.4f}; "
          f"smallest gap of the two smallest losses / sum of their bounds {gap:.3e}")


def test_relabelling_a_chain_leaves_the_loss_within_its_bound_and_argmin_is_first_minimum():
    rng = np.random.default_rng(8)
    n, K, C, S = 9, 5, 3, 11
    chains = _chains(n, K, C, S + 3, 0.7, rng)
    a = R.loss(chains, 3, S)
    perm = [3, 0, 4, 1, 2]
    b = R.loss([chains[0], np.ascontiguousarray(chains[1][:, perm]), chains[2]], 3, S)
    assert a.shape == (C, S)
    assert np.all(np.abs(a - b) <= R.bound(a, n, C * S, K))
    assert not np.array_equal(chains[1], chains[1][:, perm])
    assert R.argmin(np.array([[3.0, 1.0, 2.0], [1.0, 0.5, 0.5]])) == (1, 1)
    assert R.argmin(np.array([[1.0, 1.0], [1.0, 1.0]])) == (0, 0)
    # the sum of the losses is (N - 1) times the sum of the pooled variances
    import similarity_ref as SR
    sd = SR.similarity(chains, 3, S)["sd"]
    np.testing.assert_allclose(a.sum(), (C * S - 1) * (sd ** 2).sum(), rtol=1e-12)
