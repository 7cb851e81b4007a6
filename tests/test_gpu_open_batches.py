"""api.open_batches: saved chains as the chain slots of a Sampler.  The chain the reference ships opens to a sampler
whose slot log-likelihood is the oracle's and FLLik's (the three covariate settings of tests/test_gpu_reference_functional_trace.py),
whose "loglik" slots hold it, and whose other chain-slot calls read the file's draws; a batched run of our own, opened again,
holds the in-memory chain of the same seed bit for bit (except alpha_3 at the first draw of every file); two directories give a
2-chain sampler."""
import os
import shutil

import numpy as np
import pytest

import curve_ll_ref as CR
import oracle_lib as O
from rds_reader import read_rds
from simdata import simulate_functional
from test_gpu_post import _oracle_chain

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRACE = os.path.join(GOLD, "Functional_trace") + "/"
BK, IK = [0.0, 1000.0], [250.0, 500.0, 750.0]


@pytest.fixture(scope="module")
def example():
    Y = [np.asarray(v).reshape(-1) for v in read_rds(os.path.join(GOLD, "Sim_data.RDS"))]
    t = [np.asarray(v).reshape(-1) for v in read_rds(os.path.join(GOLD, "time.RDS"))]
    return dict(y=Y, t=t, boundary_knots=BK, internal_knots=IK, n=40)


@pytest.mark.parametrize("with_x,cov_adj", [(False, False), (True, False), (True, True)])
def test_the_shipped_chain(example, with_x, cov_adj):
    from bayesfmmm_amd import api
    e = example
    X = np.random.default_rng(7).standard_normal((40, 1)) if with_x else None     # as the existing test builds it
    kw = dict(X=X, cov_adj=cov_adj) if with_x else {}
    smp = api.open_batches(TRACE, 1, e["y"], e["t"], 3, BK, IK, **kw)
    assert (smp.n, smp.K, smp.M, smp.T, smp.P, smp.n_chains) == (40, 2, 3, 150, 7, 1)
    model, ch, B = _oracle_chain(e, X, TRACE, 1, cov_adj)
    ll = smp.slot_loglik()
    assert ll.shape == (1, 150)
    ref_o, ref_f = O.post_llik(model, ch), api.FLLik(TRACE, 1, 3, BK, IK, e["t"], e["y"], **kw)
    print(f"with_x={with_x} cov_adj={cov_adj}: largest relative difference to the oracle {np.abs(ll[0] / ref_o - 1).max():.2e}, to FLLik "
          f"{np.abs(ll[0] / ref_f - 1).max():.2e}")
    np.testing.assert_allclose(ll[0], ref_o, rtol=1e-10)
    np.testing.assert_allclose(ll[0], ref_f, rtol=1e-10)
    np.testing.assert_array_equal(smp.get_chain("loglik"), ll[0])      # open_batches stored them
    sig = api.ReadVec(TRACE + "Sigma0.txt")
    assert abs(float(smp.diagnostics("sigma_sq")["mean"]) - np.mean(sig)) <= 1e-12
    np.testing.assert_array_equal(smp.get_chain("Z"), api.ReadCube(TRACE + "Z0.txt"))
    post = api.post_curve_loglik(e["y"], B, ch.nu, ch.Phi, ch.Z, ch.chi, ch.sigma, first_kept=0, X=X, eta=ch.eta if with_x else None,
                                 xi=ch.xi if cov_adj else None)
    err = CR.rel_diff(smp.curve_loglik()[:, 0, :], post)
    print(f"  curve_loglik against post_curve_loglik: {err.max():.3e} (tolerance {CR.GPU_TOL:.1e})")
    assert err.max() <= CR.GPU_TOL
    smp.close()


def test_two_directories_give_two_chains(example, tmp_path):
    from bayesfmmm_amd import api
    e = example
    d2 = tmp_path / "second"
    shutil.copytree(TRACE, d2)
    api.write_arma_ascii(d2 / "Sigma0.txt", 1.1 * api.ReadVec(TRACE + "Sigma0.txt"))
    smp = api.open_batches([TRACE, str(d2) + "/"], 1, e["y"], e["t"], 3, BK, IK)
    assert smp.n_chains == 2 and smp.T == 150
    dg = smp.diagnostics("sigma_sq")
    assert np.isfinite(float(dg["rhat"]))
    ll = smp.slot_loglik()
    assert ll.shape == (2, 150) and np.all(np.isfinite(ll)) and not np.array_equal(ll[0], ll[1])
    for q in range(2):
        smp.select_chain(q)
        np.testing.assert_array_equal(smp.get_chain("loglik"), ll[q])
    smp.close()


def test_refusals(example, tmp_path):
    from bayesfmmm_amd import api
    e = example
    with pytest.raises(ValueError, match="The number of functions in 'Y' must be equal to the number of rows of the saved 'Z' draws"):
        api.open_batches(TRACE, 1, e["y"][:-1], e["t"][:-1], 3, BK, IK)
    with pytest.raises(ValueError, match="the saved draws do not match the basis"):
        api.open_batches(TRACE, 1, e["y"], e["t"], 3, BK, IK[:-1])
    with pytest.raises(ValueError, match="The number of columns in 'X' must be equal to the number of covariates in the model"):
        api.open_batches(TRACE, 1, e["y"], e["t"], 3, BK, IK, X=np.ones((40, 2)))
    d2 = tmp_path / "other"
    shutil.copytree(TRACE, d2)
    api.write_arma_ascii(d2 / "Nu0.txt", api.ReadCube(TRACE + "Nu0.txt")[..., :100])
    with pytest.raises(ValueError, match="holds 150 draws, 'Nu0.txt' 100"):
        api.open_batches(str(d2) + "/", 1, e["y"], e["t"], 3, BK, IK)


@pytest.mark.parametrize("D,cov_adj", [(0, False), (2, True)])
def test_a_batched_run_of_our_own_opens_to_the_in_memory_chain(tmp_path, D, cov_adj):
    from bayesfmmm_amd import api
    T, r = 120, 40      # (the entry points take no fewer than 100 iterations)
    sim = simulate_functional(n=13, M=2, sigma_sq=0.01, seed=5, ragged=True, D=max(D, 1))
    X = sim["X"][:, :D] if D else None
    common = (sim["K"], sim["y"], sim["t"], sim["n"], 3, sim["M"], sim["boundary_knots"], sim["internal_knots"])
    kw = dict(X=X) if D else {}
    est1 = api.BFMMM_Nu_Z_multiple_try(T, 1, *common, seed=1, **kw)
    kw2 = dict(kw, covariance_adj=cov_adj) if D else {}
    est2 = api.BFMMM_Theta_est(T, 1, *common, est1, seed=2, **kw2)
    full = api.BFMMM_warm_start(T, *common, est1, est2, seed=3, **kw2)
    d = str(tmp_path) + "/"
    api.BFMMM_warm_start(T, *common, est1, est2, seed=3, dir=d, r_stored_iters=r, thinning_num=1, **kw2)
    smp = api.open_batches(d, 3, sim["y"], sim["t"], 3, sim["boundary_knots"], sim["internal_knots"], X=X, cov_adj=cov_adj)
    assert (smp.n, smp.K, smp.M, smp.T) == (13, sim["K"], sim["M"], T)
    # draw 0 of file q is iteration q r, draw p > 0 iteration q r + p - 1 (thinning 1: the reference's rule)
    it = [q * r + (0 if p == 0 else p - 1) for q in range(3) for p in range(r)]
    names = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "gamma", "Phi", "tau"]
    if D:
        names += ["eta", "tau_eta"] + (["xi", "gamma_xi", "delta_xi", "A_xi"] if cov_adj else [])
    for nm in names:
        got, want = smp.get_chain(nm), np.asarray(full[nm])
        want = want[it] if nm == "tau" else want[..., it]
        if nm == "alpha_3":
            assert np.all(got[::r] == 0.0)
            got, want = np.delete(got, np.arange(0, T, r)), np.delete(want, np.arange(0, T, r))
        np.testing.assert_array_equal(got, want, err_msg=nm)
    # and the stored log-likelihood is the run's own, within the bound of tests/test_gpu_slot_loglik.py
    N_obs = sum(len(y) for y in sim["y"])
    want = np.asarray(full["loglik"])[it]
    assert np.all(np.abs(smp.get_chain("loglik") - want) <= 1e-10 * (np.abs(want) + N_obs))
    smp.close()
