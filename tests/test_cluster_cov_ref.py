"""The numpy restatement of the cluster covariance surfaces (tests/cluster_cov_ref.py) against itself: float64
within the derived bound b = c_v 2^-52 A of an np.longdouble evaluation, the invariance under joint sign changes of the
eigenfunctions that lets the chains pool, exact transposition, and the simultaneous band per pair on a hand-worked case."""
import itertools

import numpy as np
import pytest

import cluster_cov_ref as R

K, C, S, T = 3, 2, 5, 7


def _case(P, M, D, seed, flipped=False):
    """C chains of T slots of random Phi and xi, a random permutation row per draw, two bases and a covariate setting"""
    rng = np.random.default_rng(seed)
    chains = []
    for _ in range(C):
        ch = {"Phi": rng.standard_normal((K, P, M, T))}
        if flipped:      # every eigenfunction of every draw with a sign of its own, jointly over k
            ch["Phi"] = ch["Phi"] * rng.choice([-1.0, 1.0], size=(1, 1, M, T))
        if D:
            ch["xi"] = rng.standard_normal((P, D, M, K, T))
        chains.append(ch)
    perm = np.stack([np.stack([rng.permutation(K) for _ in range(S)]) for _ in range(C)]).astype(np.int32)
    E1, E2 = rng.standard_normal((5, P)), rng.standard_normal((3, P))
    x = rng.standard_normal(D) if D else None
    return chains, perm, E1, E2, x


@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("M", [1, 4, 5, 16])
@pytest.mark.parametrize("P", [4, 14, 30])
@pytest.mark.parametrize("flipped", [False, True])
def test_float64_within_the_bound_of_long_double(P, M, D, flipped):
    chains, perm, E1, E2, x = _case(P, M, D, 1000 * P + 10 * M + D, flipped)
    first = T - S
    worst = 0.0
    for e2, diagonal in ((E2, False), (None, False), (None, True)):
        v = R.values(chains, perm, E1, e2, first, S, x=x, diagonal=diagonal)
        vl = R.values(chains, perm, E1, e2, first, S, x=x, diagonal=diagonal, dtype=np.longdouble)
        b = R.bound(chains, perm, E1, e2, first, S, x=x, diagonal=diagonal)
        m = K * (K + 1) // 2
        assert v.shape == ((m, 5, C * S) if diagonal else (m, 5, 5 if e2 is None else 3, C * S))
        assert vl.dtype == np.longdouble and np.all(b > 0)
        err = np.abs(vl - v).astype(np.float64)
        worst = max(worst, float(np.max(err / b)))
        assert np.all(err <= b)
    print(f"P={P} M={M} D={D} flipped={flipped}: worst |float64 - long double| / b = {worst:.3e}")


@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_joint_sign_changes_leave_the_values(M, D):
    """(phi_.m, xi_.m) -> -(phi_.m, xi_.m) jointly over k, for every subset of m: each value stays within 2 b"""
    P = 14
    chains, perm, E1, E2, x = _case(P, M, D, 77 + M + D)
    first = T - S
    v = R.values(chains, perm, E1, E2, first, S, x=x)
    b = R.bound(chains, perm, E1, E2, first, S, x=x)
    for subset in itertools.product([1.0, -1.0], repeat=M):
        sg = np.array(subset)
        flipped = []
        for ch in chains:
            f = {"Phi": ch["Phi"] * sg[None, None, :, None]}
            if D:
                f["xi"] = ch["xi"] * sg[None, None, :, None, None]
            flipped.append(f)
        w = R.values(flipped, perm, E1, E2, first, S, x=x)
        assert np.all(np.abs(w - v) <= 2 * b), subset
        assert np.array_equal(R.bound(flipped, perm, E1, E2, first, S, x=x), b)


def test_joint_sign_changes_random_subsets_of_sixteen():
    P, M, D = 14, 16, 2
    chains, perm, E1, E2, x = _case(P, M, D, 5)
    first = T - S
    v = R.values(chains, perm, E1, E2, first, S, x=x)
    b = R.bound(chains, perm, E1, E2, first, S, x=x)
    rng = np.random.default_rng(6)
    for _ in range(8):
        sg = rng.choice([-1.0, 1.0], size=M)
        flipped = [{"Phi": ch["Phi"] * sg[None, None, :, None], "xi": ch["xi"] * sg[None, None, :, None, None]} for ch in chains]
        assert np.all(np.abs(R.values(flipped, perm, E1, E2, first, S, x=x) - v) <= 2 * b)


@pytest.mark.parametrize("D", [0, 2])
def test_exact_transposition(D):
    """(k, l, E1, E2) -> (l, k, E2, E1) transposes the restatement's surface exactly"""
    chains, perm, E1, E2, x = _case(14, 5, D, 9 + D)
    first = T - S
    pairs = [(0, 1), (2, 0), (1, 1), (2, 1)]
    a = R.values(chains, perm, E1, E2, first, S, pairs=pairs, x=x)
    b = R.values(chains, perm, E2, E1, first, S, pairs=[(l, k) for k, l in pairs], x=x)
    assert a.shape == (4, 5, 3, C * S) and b.shape == (4, 3, 5, C * S)
    assert np.array_equal(a, np.swapaxes(b, 1, 2))
    # one basis: pair (l, k) is the transpose of pair (k, l), and (k, k) is symmetric
    s = R.values(chains, perm, E1, None, first, S, pairs=[(0, 2), (2, 0), (1, 1)], x=x)
    assert np.array_equal(s[0], np.swapaxes(s[1], 0, 1)) and np.array_equal(s[2], np.swapaxes(s[2], 0, 1))
    # the diagonal is the surface's diagonal
    d = R.values(chains, perm, E1, None, first, S, pairs=[(0, 2), (2, 0), (1, 1)], x=x, diagonal=True)
    assert np.array_equal(d, np.einsum("rggs->rgs", s))


def test_default_pair_order_is_the_interfaces():
    """a null pair list means all k <= l in the order include/bfmmm.h states, which is the restatement's and the sampler's"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = " ".join(open(os.path.join(root, "include", "bfmmm.h")).read().split())
    assert "int bfmmm_chain_cluster_cov_bands(" in hdr
    assert "all m = K (K + 1) / 2 pairs with k <= l in the order * (0, 0), (0, 1), .., (0, K - 1), (1, 1), .." in hdr
    assert R.all_pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)] and len(R.all_pairs(8)) == 36
    from bayesfmmm_amd.sampler import Sampler
    assert Sampler.cluster_cov_bands.__doc__ and "all k <= l, (0, 0), (0, 1), .." in " ".join(Sampler.cluster_cov_bands.__doc__.split())


def test_relabelling_is_by_the_draws_own_row():
    """perm[k] names the component of the draw that aligned component k is read from"""
    chains, perm, E1, E2, x = _case(4, 4, 2, 21)
    first = T - S
    v = R.values(chains, perm, E1, E2, first, S, x=x)
    pairs = R.all_pairs(K)
    for q in range(C):
        for s in range(S):
            phi, xi = chains[q]["Phi"][..., first + s], chains[q]["xi"][..., first + s]      # (K, P, M), (P, D, M, K)
            theta = phi + np.einsum("d,pdmk->kpm", x, xi)
            for r, (k, l) in enumerate(pairs):
                w1 = E1 @ theta[perm[q, s, k]]          # (G1, M)
                w2 = E2 @ theta[perm[q, s, l]]
                assert np.allclose(v[r, :, :, q * S + s], w1 @ w2.T, rtol=1e-12, atol=1e-12)


def test_simultaneous_band_per_pair_by_hand():
    """one pair on a 2 x 2 grid under four draws, the entry (0, 1) constant: its sd is 0, it is left out of the maximum and its band
    is its mean"""
    trace = np.array([[[[1.0, 3.0, 5.0, 7.0], [2.0, 2.0, 2.0, 2.0]],
                       [[0.0, 0.0, 0.0, 4.0], [-1.0, 1.0, -1.0, 1.0]]]])            # (1, 2, 2, 4)
    mean = np.array([[[4.0, 2.0], [1.0, 0.0]]])
    s0, s3 = np.sqrt(20.0 / 3.0), np.sqrt(4.0 / 3.0)
    sd = np.array([[[s0, 0.0], [2.0, s3]]])
    assert np.allclose(trace.mean(axis=-1), mean) and np.allclose(trace.std(axis=-1, ddof=1), sd)
    # largest standardised deviation of every draw: max(3 / s0, 0.5, 1 / s3), max(1 / s0, 0.5, 1 / s3), the same, max(3 / s0, 1.5, 1 / s3)
    dev = np.array([3.0 / s0, 1.0 / s3, 1.0 / s3, 1.5])
    # alpha = 0.25: p = 0.75 lies halfway between the plotting positions 0.625 and 0.875 of the third and fourth order statistic
    crit = 0.5 * (3.0 / s0) + 0.5 * 1.5
    got = R.sim_bands(trace, 0.25, mean, sd)
    assert got["crit"].shape == (1,) and got["lower"].shape == (1, 2, 2) and got["upper"].shape == (1, 2, 2)
    assert np.isclose(got["crit"][0], crit, rtol=1e-15)
    assert np.allclose(got["lower"], mean - crit * sd, rtol=1e-15) and np.allclose(got["upper"], mean + crit * sd, rtol=1e-15)
    assert got["lower"][0, 0, 1] == 2.0 and got["upper"][0, 0, 1] == 2.0
    assert np.all(np.isfinite(got["lower"])) and np.all(np.isfinite(got["upper"]))
    # the maxima themselves
    import curve_sim_ref as SR
    assert np.allclose(SR.sim_bands(trace.reshape(1, 4, 4), 0.25, mean.reshape(1, 4), sd.reshape(1, 4))["C"][0], dev, rtol=1e-15)
    # two pairs are banded one by one: the second pair's wider spread does not move the first pair's crit
    two = np.concatenate([trace, 10.0 * trace[:, ::-1]], axis=0)
    m2, s2 = np.concatenate([mean, 10.0 * mean[:, ::-1]]), np.concatenate([sd, 10.0 * sd[:, ::-1]])
    g2 = R.sim_bands(two, 0.25, m2, s2)
    assert g2["crit"][0] == got["crit"][0] and np.isclose(g2["crit"][1], crit, rtol=1e-14)
