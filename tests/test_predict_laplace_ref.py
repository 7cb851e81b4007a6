"""CPU checks of the numpy restatement of the Laplace mixture proposal (tests/predict_laplace_ref.py): the gradient and
the Hessian of g against central differences in np.longdouble; the float64 floors of g, its derivatives, the Newton decrement and the
mixture density against np.longdouble, which the device tolerances are built on; the estimator against a quadrature where K = 2,
with a case whose start at alpha / alpha_0 does not converge; and the staged Dirichlet against the mixture on the fixture of the
device's comparison."""
import math

import numpy as np
import pytest

import predict_laplace_ref as Lr
import predict_ref as R

LD = np.longdouble


def _richardson(f, x, k, h):
    """central difference of f along coordinate k, Richardson-extrapolated from h and h / 2 (error of order h^4)"""
    def cd(hh):
        e = np.zeros_like(x)
        e[k] = hh
        return (f(x + e) - f(x - e)) / (2 * hh)
    return (4 * cd(h / 2) - cd(h)) / 3


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("D,cadj", [(0, False), (2, True)])
def test_gradient_and_hessian_against_central_differences(K, D, cadj):
    """float64 derivatives against long-double differences of g (gradient) and of the long-double gradient (Hessian), h = 1e-6.
    The bound is one for the formulas, 1e-6 of the largest entry: a wrong term is an error of order 1, the differences are good to
    eps_ld |g| / h = 1e-13 |g| and h^4 times a fifth derivative, and float64 itself to the floor of the next test."""
    assert np.finfo(LD).eps < 1e-18
    rng = np.random.default_rng(100 * K + D)
    worst_g = worst_h = 0.0
    done = 0
    while done < 6:
        case, eta = Lr.random_laplace_case(rng, K=K, M=int(rng.choice([1, 2, 3])), D=D, covariance_adj=cadj)
        g, grad, H = Lr.evaluate(case, eta)
        if not np.isfinite(g):
            continue
        done += 1
        x = eta.astype(LD)
        h = LD(1e-6)
        fd_g = np.array([_richardson(lambda e: Lr.evaluate(case, e, LD, derivs=False), x, k, h) for k in range(K - 1)])
        fd_h = np.array([_richardson(lambda e: Lr.evaluate(case, e, LD)[1], x, k, h) for k in range(K - 1)])
        worst_g, worst_h = max(worst_g, Lr.rel(grad, fd_g)), max(worst_h, Lr.rel(H, fd_h))
        assert Lr.rel(grad, fd_g) < 1e-6 and Lr.rel(H, fd_h) < 1e-6, (K, D, done, Lr.rel(grad, fd_g), Lr.rel(H, fd_h))
        # the dense form of l gives the same g
        assert abs(Lr.g_dense(case, eta[None, :])[0] - g) <= 1e-9 * max(1.0, abs(g))
    print(f"K = {K}, D = {D}: worst relative difference gradient {worst_g:.2e}, Hessian {worst_h:.2e}")


def test_float64_floors_against_long_double():
    """the floors DESIGN.md 7p records; the bounds here are those of tests/test_loo_marginal_ref.py's floor (1e-9), ten times that for
    the Hessian, whose entries cancel between terms of size |H| / sigma^2"""
    w = Lr.derivative_floor()
    print("float64 against long double over 600 inputs: " + ", ".join(f"{k} {v:.3e}" for k, v in w.items()))
    assert w["g"] < 1e-9 and w["grad"] < 1e-9 and w["dec"] < 1e-9 and w["logq"] < 1e-9 and w["H"] < 1e-8


def test_t4_density_integrates_and_matches_its_samples():
    """d = 1: the density sums to 1 on a grid; d = 2: the share of standardised coordinates inside the t4 quartile 0.7407 is 1 / 2"""
    x = np.linspace(-400.0, 400.0, 800001)[:, None]
    c = {"eta": np.array([0.3]), "L": np.array([[0.7]]), "J": 5}
    assert abs(np.exp(Lr.log_t4(x, c["eta"], c["L"])).sum() * (x[1, 0] - x[0, 0]) - 1.0) < 1e-6
    rng = np.random.default_rng(4)
    c2 = {"eta": np.array([0.3, -1.0]), "L": np.array([[0.7, 0.0], [0.2, 1.5]]), "J": 4096}
    s = np.linalg.solve(c2["L"], (Lr.draw([c2], rng) - c2["eta"]).T).T
    share = np.mean(np.abs(s) < 0.7407)
    assert abs(share - 0.5) <= 4 * math.sqrt(0.25 / s.size)


def k2_case(seed, n, sig=0.01):
    """K = 2, M = 2, P = 6 (tests/loo_marginal_ref.py's K = 2 curve with random memberships and prior, and sharper)"""
    rng = np.random.default_rng(seed)
    K, M, P = 2, 2, 6
    B = rng.uniform(0.0, 1.0, size=(n, P))
    th = R.directions(rng.standard_normal((K, P)), 0.4 * rng.standard_normal((K, P, M)))
    u = rng.uniform(0.05, 0.95)
    y = B @ (np.array([u, 1 - u]) @ th[:, 0]) + math.sqrt(sig) * rng.standard_normal(n)
    return Lr.make_case(B, y, th, sig, rng.uniform(0.3, 4.0, size=2))


@pytest.mark.parametrize("n", [20, 100])
def test_estimator_against_quadrature_k2(n):
    J = 256
    devs, stalled_first = [], 0
    for seed in range(215, 223):
        case = k2_case(seed, n)
        exact = Lr.k2_exact(case)
        assert abs(exact - Lr.k2_exact(case, nodes=50001)) < 1e-10      # the quadrature has converged
        est = Lr.estimate(case, J, np.random.default_rng(1000 + seed))
        runs, comps = est["runs"], est["comps"]
        stalled_first += not runs[0]["conv"]
        # only converged starts are components, each a maximum with a small decrement
        assert len(comps) - 1 <= sum(r["conv"] for r in runs) and len(comps) >= 2
        for c in comps[1:]:
            g, grad, H = Lr.evaluate(case, c["eta"], LD)
            assert Lr.decrement(grad, H) is not None and Lr.decrement(grad, H) < 1e-5
            assert any(r["conv"] and np.array_equal(r["eta"], c["eta"]) for r in runs)
        assert sum(c["J"] for c in comps) == J and comps[0]["J"] == J // 16
        se = math.sqrt(max(1.0 / est["ess"] - 1.0 / J, 0.0))      # delta method, as tests/test_predict_ref.py
        devs.append(abs(est["lpd"] - exact) / se)
        print(f"n = {n}, seed {seed}: converged {[r['conv'] for r in runs]}, iterations {[r['iters'] for r in runs]}, J_c {[c['J'] for c in comps]}, "
              f"lpd {est['lpd']:.6f}, exact {exact:.6f}, ess {est['ess']:.1f}, |dev| / se = {devs[-1]:.2f}")
    assert max(devs) < 5.0
    if n == 100:
        assert stalled_first >= 1, "the set must hold a case whose start at alpha / alpha_0 does not converge"


def test_no_converged_start_leaves_the_defensive_component():
    case = k2_case(215, 20)
    orig = Lr.search
    try:
        Lr.search = lambda c, e, dtype=np.float64: dict(orig(c, e, dtype), conv=False)
        comps, _ = Lr.components(case, 64)
    finally:
        Lr.search = orig
    assert len(comps) == 1 and comps[0]["J"] == 64
    est_eta = Lr.draw(comps, np.random.default_rng(0))
    out = Lr.weigh(Lr.g_batch(case, est_eta), est_eta, comps)
    assert np.isfinite(out["lpd"]) and 1.0 <= out["ess"] <= 64.0


def test_sharp_fixture_separates_the_proposals():
    """the fixture of the device's comparison (tests/test_gpu_predict_laplace.py), on the CPU alone: over its 24 pairs the staged
    Dirichlet (R = 3, J = 256) has a median ess below half of J and the mixture's median exceeds it; every pair has a converged mode"""
    sim, draws = Lr.sharp_fixture()
    cases = Lr.sharp_cases(sim, draws)
    flat = [case for per_curve in cases for row in per_curve for case in row]
    J = 256
    for seed in range(3):          # (the staged estimator's ess of a pair is anywhere from 1 to J with the seed: the median is held for three)
        rng = np.random.default_rng(seed)
        old = [Lr.staged_dirichlet_ess(case, J, 3, rng) for case in flat]
        ests = [Lr.estimate(case, J, rng) for case in flat]
        new = [e["ess"] for e in ests]
        assert all(len(e["comps"]) >= 2 for e in ests)
        print(f"seed {seed}: median ess over {len(old)} pairs: staged Dirichlet {np.median(old):.1f} (least {min(old):.1f}), mixture {np.median(new):.1f} "
              f"(least {min(new):.1f})")
        assert len(old) == 24 and np.median(old) < 0.5 * J and np.median(new) > np.median(old)
