"""The restatements of the leave-block-out quantities within a curve (tests/loo_blocks_ref.py) against each other on the CPU:
explicit conditioning on the dense n_i x n_i covariance and the closed form on the M x M system that k_loo_blocks evaluates
(DESIGN.md 7s), and the identities that tie them to the observation-level form and to the curve's log-density.  The worst
differences are the floors the forms themselves impose; the GPU tests hold the kernel to ten times them (GPU_TOL_*).  The device is
not consulted here."""
import numpy as np

import curve_ll_ref as CL
import loo_blocks_ref as R
import loo_pointwise_ref as LP
from test_curve_ll_ref import _random_curve


def _block(rng, ni, mode):
    """whole-curve (where it fits), contiguous, trailing or scattered, of size 1 to min(64, n_i)"""
    b = min(ni, 64) if mode == 0 else int(rng.integers(1, min(64, ni) + 1))
    if mode == 0 and ni <= 64:
        return np.arange(ni)
    if mode in (0, 1):
        st = int(rng.integers(0, ni - b + 1))
        return np.arange(st, st + b)
    if mode == 2:
        return np.arange(ni - b, ni)
    return rng.permutation(ni)[:b]


def test_closed_and_dense_forms_agree():
    rng = np.random.default_rng(20251)
    P, M, K = 12, 3, 3
    names = ("l", "m", "sqrt v", "z")
    worst, at = [0.0] * 4, [None] * 4
    modes = [0, 0, 0, 0]
    for it in range(2000):
        D = 0 if it % 2 == 0 else 2
        y, B, sigma_sq, z, nu, Phi, x, eta, xi = _random_curve(rng, P, M, K, D)
        c, V = CL.coefficients(z, nu, Phi, x, eta, xi)
        idx = _block(rng, len(y), it % 4)
        modes[it % 4] += 1
        dl, dm, dv, dz = R.dense(y, B, c, V, sigma_sq, idx)
        cl, cm, cvv, cz = R.closed(y, B, c, V, sigma_sq, idx, B.T @ B, B.T @ y)
        assert np.all(cvv > 0) and np.all(dv > 0) and np.isfinite(cl)
        for q, (a, b) in enumerate(((cl, dl), (cm, dm), (np.sqrt(cvv), np.sqrt(dv)), (cz, dz))):
            e = float(np.max(R.rel_diff(a, b)))
            if e > worst[q]:
                worst[q], at[q] = e, (it, len(y), len(idx), sigma_sq)
    for q in range(4):
        print(f"worst |closed - dense| / max(1, |.|) of {names[q]} over 2000 curves: {worst[q]:.3e} at (index, n_i, |b|, sigma^2) = {at[q]}")
    # the rest's covariance has condition number up to (sigma^2 + lambda_max(UU')) / sigma^2, about 1e7 here, and its solve loses that
    # factor times the unit roundoff in m and v; l and z divide the residual by sqrt(v) >= sigma >= 1e-2: 1e7 x 1.1e-16 x 1e2 = 1e-7
    assert max(worst) < 1e-7
    # the recorded floors are what this run measures (same seed, same order of magnitude)
    for w, floor in zip(worst, (R.FORM_FLOOR_L, R.FORM_FLOOR_M, R.FORM_FLOOR_SD, R.FORM_FLOOR_Z)):
        assert floor / 3.0 < w < 3.0 * floor, (worst, floor)
    assert (R.GPU_TOL_L, R.GPU_TOL_M, R.GPU_TOL_SD, R.GPU_TOL_Z) == tuple(10.0 * f for f in (R.FORM_FLOOR_L, R.FORM_FLOOR_M, R.FORM_FLOOR_SD,
                                                                                             R.FORM_FLOOR_Z))
    assert R.GPU_TOL_PIT == 0.4 * R.GPU_TOL_Z + 1e-15


def _curves(seed, count):
    rng = np.random.default_rng(seed)
    for j in range(count):
        y, B, sigma_sq, z, nu, Phi, x, eta, xi = _random_curve(rng, 12, 3, 3, 2 if j % 2 else 0)
        c, V = CL.coefficients(z, nu, Phi, x, eta, xi)
        yield rng, y, B, c, V, sigma_sq


def test_single_observation_block_is_the_pointwise_law():
    for rng, y, B, c, V, sigma_sq in _curves(11, 40):
        pl, pm, pv, pz = LP.dense(y, B, c, V, sigma_sq)
        for j in {0, len(y) - 1, int(rng.integers(0, len(y)))}:
            for form in (R.dense, R.closed):
                l, m, v, z = form(y, B, c, V, sigma_sq, [j])
                assert m.shape == v.shape == z.shape == (1,)
                # both sides are dense conditionings or within the floors of the two forms of either helper
                assert float(R.rel_diff(l, pl[j])) < 3.0 * (LP.FORM_FLOOR_L + R.FORM_FLOOR_L)
                assert float(R.rel_diff(m[0], pm[j])) < 3.0 * (LP.FORM_FLOOR_M + R.FORM_FLOOR_M)
                assert float(R.rel_diff(np.sqrt(v[0]), np.sqrt(pv[j]))) < 3.0 * (LP.FORM_FLOOR_SD + R.FORM_FLOOR_SD)
                assert float(R.rel_diff(z[0], pz[j])) < 3.0 * (LP.FORM_FLOOR_Z + R.FORM_FLOOR_Z)


def test_whole_curve_block_is_the_curve_density():
    seen = 0
    for rng, y, B, c, V, sigma_sq in _curves(12, 200):
        if len(y) > 64:
            continue
        seen += 1
        ref = CL.dense(y, B, c, V, sigma_sq)
        idx = rng.permutation(len(y))                    # in any order
        for form in (R.dense, R.closed):
            l, m, v, z = form(y, B, c, V, sigma_sq, idx)
            assert float(R.rel_diff(l, ref)) < 3.0 * R.FORM_FLOOR_L + CL.GPU_TOL
            np.testing.assert_allclose(m, (B @ c)[idx], rtol=0, atol=3.0 * R.FORM_FLOOR_M * max(1.0, float(np.abs(B @ c).max())))
    assert seen >= 20


def test_chain_rule():
    """log p(y) = l_b + log p(y_-b), the sub-curve's density from curve_ll_ref.dense"""
    for rng, y, B, c, V, sigma_sq in _curves(13, 60):
        ni = len(y)
        if ni < 2:
            continue
        idx = _block(rng, ni, 1 + int(rng.integers(0, 3)))
        if len(idx) == ni:
            idx = idx[:-1]
        rest = np.setdiff1d(np.arange(ni), idx)
        full, sub = CL.dense(y, B, c, V, sigma_sq), CL.dense(y[rest], B[rest], c, V, sigma_sq)
        for form in (R.dense, R.closed):
            l = form(y, B, c, V, sigma_sq, idx)[0]
            # the two curve densities carry their own error relative to their size: the difference is held to the floor of l at
            # that scale
            scale = max(1.0, abs(full), abs(sub))
            assert abs(l - (full - sub)) <= (3.0 * R.FORM_FLOOR_L + 2.0 * CL.GPU_TOL) * scale, (ni, len(idx), sigma_sq)
