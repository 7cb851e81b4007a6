"""The marginal PSIS-LOO under the Laplace mixture proposal on the device (Sampler.loo_marginal(proposal="laplace"),
bfmmm_chain_loo_marginal_laplace): its traces are Sampler.predict's under the same proposal on the training data and
its pointwise arrays api.psis_loo's on that matrix, bit for bit; the counts against numpy; budget, repeat and refusals.  The
estimator itself is held against the restatement in tests/test_gpu_predict_laplace.py."""
import re

import numpy as np
import pytest

import test_gpu_loo_marginal as TL

pytestmark = pytest.mark.gpu

POINTWISE = TL.POINTWISE
N_CURVES, NCH, T = 6, 2, 21      # PSIS wants at least 21 draws a row; 2 chains x 21 slots pooled


@pytest.fixture(scope="module")
def base():
    """test_gpu_loo_marginal.py's curves, the first 6 of them (5 .. 25 points), K = 3, M = 2, 2 chains x 21 slots after a short run"""
    sim, ts, ys, Bs = TL._functional_data()
    ts, ys = ts[:N_CURVES], ys[:N_CURVES]
    smp = TL.tiny_sampler(sim, ys, ts, iters=T)
    TL._start(smp, 7)
    yield dict(smp=smp, data=dict(Y_new=ys, time_new=ts))
    smp.close()


@pytest.mark.parametrize("J", [37, 300])
def test_traces_are_predicts_and_psis_is_apis(base, J):
    from bayesfmmm_amd import api
    smp = base["smp"]
    n, Cn, S = smp.n, smp.n_chains, smp.T
    lm = smp.loo_marginal(n_samples=J, seed=5, trace=True, proposal="laplace", ess_floor=0.25 * J)
    pr = smp.predict(n_samples=J, seed=5, trace=True, proposal="laplace", **base["data"])
    assert lm["lpd_trace"].shape == (n, Cn, S)
    TL._same_bits(lm, pr, ("lpd_trace", "ess_trace", "n_modes", "components", "eta_samples", "n_modes_mean"))
    ps = api.psis_loo(lm["lpd_trace"].reshape(n, -1))
    TL._same_bits(lm, ps, POINTWISE)
    for k, v in api.loo_totals({k: lm[k] for k in POINTWISE}, Cn * S).items():
        assert np.array_equal(np.asarray(lm[k]), np.asarray(v)), k
    ess = lm["ess_trace"].reshape(n, -1)
    assert np.array_equal(lm["n_below"], np.sum((ess < 0.25 * J) | ~np.isfinite(lm["lpd_trace"].reshape(n, -1)), axis=1))
    assert np.array_equal(lm["ess_min"], ess.min(axis=1)) and np.allclose(lm["ess_mean"], ess.mean(axis=1), rtol=1e-13, atol=0)
    assert np.all(lm["n_modes"] >= 1) and lm["proposal"] == "laplace" and lm["n_samples"] == J and "n_refined" not in lm
    print(f"J = {J}: median ess {np.median(ess):.1f}, least {ess.min():.1f}, below the floor {int(lm['n_below'].sum())} of {ess.size}, "
          f"modes {np.bincount(lm['n_modes'].reshape(-1))}, worst pareto_k {lm['pareto_k'].max():.2f}")


def test_bits_under_budget_and_repeat_and_the_default_call(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    keys = POINTWISE + ("ess_mean", "ess_min", "n_below", "lpd_trace", "ess_trace", "n_modes", "components", "eta_samples")
    before = smp.loo_marginal(n_samples=37, seed=3, trace=True)
    kw = dict(n_samples=37, seed=3, trace=True, proposal="laplace")
    one = smp.loo_marginal(**kw)
    TL._same_bits(smp.loo_marginal(**kw), one, keys)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_marginal_laplace: 'max_workspace_bytes' below the") as ei:
        smp.loo_marginal(max_workspace_bytes=1, **kw)
    per_curve = int(re.search(r"\(0 shared by all curves \+ (\d+) per curve\)", str(ei.value)).group(1))
    TL._same_bits(smp.loo_marginal(max_workspace_bytes=4 * per_curve, **kw), one, keys)
    assert smp.timing("loo_marginal_laplace")[1] == 4 and smp.timing("loo_marginal_psis")[1] == 2       # two chunks of 4 and 2 curves
    plain = smp.loo_marginal(n_samples=37, seed=3, proposal="laplace")
    TL._same_bits(plain, one, POINTWISE + ("ess_mean", "ess_min", "n_below", "n_modes_mean"))
    assert "lpd_trace" not in plain
    # the default proposal is as it was
    after = smp.loo_marginal(n_samples=37, seed=3, trace=True)
    TL._same_bits(after, before, [k for k, v in before.items() if isinstance(v, np.ndarray)])


def test_refusals_by_name(base):
    from bayesfmmm_amd import _lib
    smp = base["smp"]
    with pytest.raises(ValueError, match="loo_marginal: 'n_stages' has no meaning with proposal='laplace'"):
        smp.loo_marginal(n_stages=2, proposal="laplace")
    with pytest.raises(ValueError, match="loo_marginal: 'refine' has no meaning with proposal='laplace'"):
        smp.loo_marginal(refine=True, proposal="laplace")
    with pytest.raises(ValueError, match="loo_marginal: 'refine_samples' has no meaning with proposal='laplace'"):
        smp.loo_marginal(refine_samples=64, proposal="laplace")
    assert smp.loo_marginal(n_samples=8, refine=False, proposal="laplace")["n_samples"] == 8
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_loo_marginal_laplace: n x n_samples x \(K \+ 1\) = 6 x 2000000000 x 4 exceeds the 4294967296"):
        smp.loo_marginal(n_samples=2_000_000_000, proposal="laplace")
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_chain_loo_marginal_laplace: k_predict_lap: the tables of a draw .* need \d+ bytes of LDS, above the limit of 163840"):
        smp.loo_marginal(n_samples=8192, proposal="laplace")
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_marginal_laplace: 'ess_floor' must be finite and not negative"):
        smp.loo_marginal(ess_floor=-1.0, proposal="laplace")
