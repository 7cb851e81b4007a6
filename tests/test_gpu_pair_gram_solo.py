"""The single-chain body of k_pair_gram's G workgroups (pg_solo_g) against the general body of the same
kernel: same data, start state and seeds, whole warm-start trajectories of one chain, every chain slot BIT-identical (both keep
the canonical summation order: slice, k-step, pair-weight product).  Shapes: the benchmark's config 2 (a partial last k-slice
of 48 curves), n = 4096 + 37 (a partial last 16-curve chunk), n = 200 (32-curve slices), K = 2 / 4 and M = 1 / 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN_NAMES = ["nu", "Phi", "chi", "Z", "pi", "alpha_3", "delta", "A", "gamma", "tau", "sigma_sq", "loglik"]


def _trajectories(n, K, M, T=12):
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    from bench import make_config2
    lib = _lib.load()
    w = make_config2(n=n, n_i=100, K=K, M=M)
    out = {}
    try:
        for solo in (1, 0):
            lib.bfmmm_set_solo_pair_gram(solo)
            cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=w["K"], n_eigen=w["M"], basis_degree=3, tot_mcmc_iters=T)
            smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"])
            smp.set_state(**w["state"])
            # two calls: the second continues from the device state the first leaves (deferred jobs, prepared proposals)
            smp.run(bf.sampler.SWEEP_WARM, 5, first_iter=0, seed=7)
            smp.run(bf.sampler.SWEEP_WARM, T - 5, first_iter=5, seed=7)
            out[solo] = {nm: np.array(smp.get_chain(nm), copy=True) for nm in CHAIN_NAMES}
            smp.close()
    finally:
        lib.bfmmm_set_solo_pair_gram(1)
    return out


@pytest.mark.parametrize("n,K,M", [(4096, 3, 6), (4096 + 37, 3, 6), (200, 3, 6), (1000, 2, 1), (1000, 4, 8), (200, 2, 8),
                                   (4096 + 37, 4, 1)])
def test_solo_body_equals_general_body_bitwise(n, K, M):
    out = _trajectories(n, K, M)
    for nm in CHAIN_NAMES:
        assert np.all(np.isfinite(out[1][nm])), nm
        np.testing.assert_array_equal(out[1][nm], out[0][nm], err_msg=f"n={n} K={K} M={M} {nm}")
    # the chain moved (a trajectory, not a copy of the start state)
    assert not np.array_equal(out[1]["nu"][..., 0], out[1]["nu"][..., -1])
