"""The smallest sampler the host-layer tests share: functional model, n = 6 curves, K = 2, n_eigen = 2, cubic basis with one
internal knot (P = 5), 2 chains, T = 4."""
import numpy as np

from simdata import simulate_functional
from test_gpu_chain_batch import make_sampler_batch

N, K, M, P, NCH, T = 6, 2, 2, 5, 2, 4


def make_tiny(D=0, covariance_adj=False, run=False):
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=N, M=M, sigma_sq=0.01, seed=5, K=K)
    sim["internal_knots"] = np.array([495.0])
    smp = make_sampler_batch(sim, T, NCH)
    assert (smp.n, smp.K, smp.M, smp.P, smp.n_chains, smp.T) == (N, K, M, P, NCH, T)
    mask = bf.SWEEP_WARM
    if D:
        smp.set_covariates(np.random.default_rng(2).standard_normal((N, D)), covariance_adj=covariance_adj)
        mask |= bf.sampler.COV_MEAN | (bf.sampler.COV_XI if covariance_adj else 0)
    if run:
        for q in range(NCH):
            smp.select_chain(q)
            smp.init_state(1, 11, chain=q)
        smp.select_chain(0)
        smp.run(mask, T, seed=3)
    return smp


def basis_rows(smp, G):
    """G rows in the sampler's basis: the first observation rows of the first curve's own basis"""
    return np.ascontiguousarray(smp.get_basis()[0][:G])
