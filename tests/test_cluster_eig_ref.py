"""The numpy restatement of the cluster eigenvalues and eigenfunctions (tests/cluster_eig_ref.py) against
itself, without a device: on random inputs in every shape of tests/test_gpu_cluster_eig.py the float64 run stays inside every bound
of the long-double run, the cap of 40 sweeps is never reached, the eigenvalues are numpy.linalg.eigvalsh's and sum to the total;
rotating Theta, flipping the signs of its columns and relabelling through perm change nothing beyond the bounds; and the zero rule
and the sign rule hold on hand-made cases.  The constants C_J, C_PSI, C_O of the module are four times the worst ratios this file
prints, rounded up (run with -s)."""
import numpy as np
import pytest

import cluster_eig_ref as R

LD = np.longdouble
CASES = R.cases()


def _inside(out, label):
    bad = {k: v for k, v in out.items() if not k.endswith("_units") and not v <= 1.0}
    assert not bad, (label, bad)


def test_round_robin_covers_every_pair_once():
    for M in range(1, 17):
        rounds = R.rr_pairs(M)
        assert len(rounds) == ((M + 1) & ~1) - 1
        flat = [p for rnd in rounds for p in rnd]
        assert sorted(flat) == [(p, q) for p in range(M) for q in range(p + 1, M)], M
        for rnd in rounds:                                       # the pairs of a round are disjoint
            idx = [i for p in rnd for i in p]
            assert len(idx) == len(set(idx)), M


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_float64_run_inside_the_bounds(case):
    label, Th, E, w, ref, D = case
    M = Th.shape[2]
    f64 = R.solve(Th, E, w, ref, M, np.float64)
    out, exact_zero, ld = R.check(f64, Th, E, w, ref, D, ref_rule=None if ref is not None else "largest")
    print(label, {k: round(v, 3) for k, v in out.items()}, "sweeps", int(f64["sweeps"].max()), int(ld["sweeps"].max()))
    _inside(out, label)
    assert exact_zero
    assert not f64["capped"].any() and not ld["capped"].any() and f64["sweeps"].max() < R.CAP and ld["sweeps"].max() < R.CAP
    # the constants are at least four times what this run needs
    assert 4 * out["lam_units"] <= R.C_J and 4 * out["resid_units"] <= R.C_PSI and 4 * out["orth_units"] <= R.C_O
    # numpy's own eigenvalues of W^1/2 A A' W^1/2
    sw = np.ones(E.shape[0]) if w is None else np.sqrt(w)
    AE = sw[None, :, None] * np.einsum("gp,bpm->bgm", E, Th)
    ev = np.linalg.eigvalsh(np.einsum("bgm,bhm->bgh", AE, AE))[:, ::-1]
    n = min(M, ev.shape[1])
    bS, _ = R.bound_S(Th, E, w, D)
    nS = np.sqrt(np.sum(ld["S"] ** 2, axis=(1, 2)))
    b_lam = np.sqrt(np.sum(bS * bS, axis=(1, 2))) + LD(R.C_J * R.U) * nS
    # eigvalsh's own error: a small multiple of 2^-53 ||.||_2 of a G x G matrix
    b_np = LD(4 * E.shape[0] * R.U) * ev[:, :1]
    assert np.all(np.abs(f64["lam"][:, :n] - ev[:, :n]) <= (b_lam[:, None] + b_np)), label
    assert np.all(np.abs(f64["lam"][:, n:]) <= b_lam[:, None]), label


@pytest.mark.parametrize("case", [c for c in CASES if c[4] is not None and c[1].shape[2] > 1][::2], ids=lambda c: c[0])
def test_rotation_sign_and_relabelling_invariance(case):
    label, Th, E, w, ref, D = case
    B, P, M = Th.shape
    rng = np.random.default_rng(5)
    # sign flips of the columns: exact in Theta, so every condition holds against the unflipped long-double run
    sg = rng.choice([-1.0, 1.0], size=(B, 1, M))
    out, ez, _ = R.check(R.solve(Th * sg, E, w, ref, M, np.float64), Th, E, w, ref, D)
    _inside(out, label + " signs")
    assert ez
    # a random orthogonal rotation, applied in float64: Theta O is within (M + 1) 2^-53 |Theta| |O| of exact, which moves S by at most
    # (M + 2) 2^-52 ||(|Theta| |O|)' |Q| (|Theta| |O|)||_F
    O = np.linalg.qr(rng.standard_normal((B, M, M)))[0]
    ThO = np.einsum("bpm,bmj->bpj", Th, O)
    AO = R.form_S(R.gram(E, w, LD, absolute=True), np.einsum("bpm,bmj->bpj", np.abs(Th), np.abs(O)).astype(LD))
    extra = LD((M + 2) * 2.0 ** -52) * np.sqrt(np.sum(AO * AO, axis=(1, 2)))
    got = R.solve(ThO, E, w, ref, M, np.float64)
    out, ez, _ = R.check(got, Th, E, w, ref, D, extra_S=extra)
    print(label, "rotation", {k: round(v, 3) for k, v in out.items()})
    _inside(out, label + " rotation")
    assert ez


def test_relabelling_through_perm():
    """perm relabels whole components: the aligned Theta of a relabelled chain under the matching perm is the same array"""
    rng = np.random.default_rng(6)
    K, P, M, T, first, S = 3, 5, 2, 9, 2, 6
    ch = {"Phi": rng.standard_normal((K, P, M, T)), "xi": rng.standard_normal((P, 2, M, K, T))}
    perm = np.stack([rng.permutation(K) for _ in range(S)])[None].astype(np.int32)
    x = np.array([0.4, -1.1])
    A = R.thetas([ch], perm, first, S, x)
    assert A.shape == (K, S, P, M)
    # relabel the stored components by a fixed sigma and compose the permutation rows with it
    sigma = np.array([2, 0, 1])
    ch2 = {"Phi": ch["Phi"][sigma], "xi": ch["xi"][:, :, :, sigma]}
    inv = np.argsort(sigma)
    B = R.thetas([ch2], inv[perm], first, S, x)
    assert A.tobytes() == B.tobytes()
    # a constant permutation applied to every draw permutes the components of the result
    C = R.thetas([ch], perm[:, :, sigma], first, S, x)
    assert C.tobytes() == np.ascontiguousarray(A[sigma]).tobytes()


def test_hand_made_cases():
    rng = np.random.default_rng(7)
    P, M = 5, 3
    Th = rng.standard_normal((4, P, M))
    for dtype in (np.float64, LD):
        # G = 1: rank one, every later eigenvalue under the zero rule and its function exactly zero
        E1 = rng.standard_normal((1, P))
        r = R.solve(Th, E1, None, None, M, dtype)
        assert np.all(r["zero"][:, 1:]) and not r["zero"][:, 0].any() and np.all(r["psi"][:, 1:] == 0) and np.all(r["b"][:, 1:] == 0)
        assert np.all(r["psi"][:, 0, 0] > 0)                       # the largest-entry rule on the only entry
        assert np.all(np.abs(r["pve"][:, 0] - 1) <= 8 * 2.0 ** -52) and np.all(r["pve"][:, 1:] <= M * 2.0 ** -52)
        # a zero row of E and a zero weight: psi is exactly 0 on the zero row, and the zero-weight entry takes no part in the sign
        E = rng.standard_normal((6, P))
        E[2] = 0.0
        w = np.array([1.0, 0.5, 2.0, 0.0, 1.5, 1.0])
        r = R.solve(Th, E, w, None, M, dtype)
        assert np.all(r["psi"][:, :, 2] == 0) and not r["zero"].any()
        a = np.sqrt(w)[None, None, :] * np.abs(np.asarray(r["psi"], dtype=np.float64))
        g = np.argmax(a, axis=-1)
        assert np.all(g != 3) and np.all(np.take_along_axis(r["psi"], g[..., None], axis=-1) > 0)
        # against a reference: the inner product is not negative, and -ref flips every function
        ref = rng.standard_normal((M, 6))
        rp, rm = R.solve(Th, E, w, ref, M, dtype), R.solve(Th, E, w, -ref, M, dtype)
        assert np.all(np.einsum("g,bjg,jg->bj", w, np.asarray(rp["psi"], dtype=np.float64), ref) >= 0)
        assert np.all(rp["psi"] == -rm["psi"]) and np.all(rp["lam"] == rm["lam"])
        # Theta = 0: everything is zero, one sweep, no rotation
        r = R.solve(np.zeros((2, P, M)), E, w, ref, M, dtype)
        assert np.all(r["lam"] == 0) and np.all(r["total"] == 0) and np.all(r["pve"] == 0) and np.all(r["psi"] == 0) and np.all(r["zero"])
        assert np.all(r["sweeps"] == 1) and not r["capped"].any()
