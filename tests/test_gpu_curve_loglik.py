"""The per-curve marginal log-density of chain slots on the device (k_chain_curve_ll): Sampler.curve_loglik
against the dense numpy restatement (tests/curve_ll_ref.py) fed the get_chain copies, its two device-resident routes
(curve_diagnostics, loo) against the matrix routes bit for bit, chunking, repeatability, label and sign invariance and the
argument checks.  The tolerance is curve_ll_ref.GPU_TOL: ten times the floor the two forms of the density impose on each
other (tests/test_curve_ll_ref.py), not a figure taken from the kernel."""
import numpy as np
import pytest

import curve_ll_ref as R
from test_gpu_chain_batch import _states, make_sampler_batch
from simdata import simulate_functional

pytestmark = pytest.mark.gpu

NAMES = ["nu", "Phi", "Z", "chi", "sigma_sq"]
DIAG = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")
LOO_ARRAYS = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic")


def _chains(smp, cov=False):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in NAMES + (["eta", "xi"] if cov else [])})
    return out


def _check(smp, Y, B, first, n_slots, X=None, covariance_adj=False, label=""):
    got = smp.curve_loglik(first_slot=first, n_slots=n_slots)
    assert got.shape == (smp.n, smp.n_chains, n_slots)
    ref = R.dense_matrix(Y, B, _chains(smp, X is not None), first, n_slots, X, covariance_adj)
    assert np.all(np.isfinite(ref)), label
    err = R.rel_diff(got, ref)
    print(f"{label}: worst |device - dense| / max(1, |l|) = {err.max():.3e} (tolerance {R.GPU_TOL:.1e}), |l| up to {np.abs(ref).max():.3e}")
    assert err.max() <= R.GPU_TOL, (label, float(err.max()), np.unravel_index(np.argmax(err), err.shape))
    return got


def test_functional_matches_dense_and_post_curve_loglik():
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import api
    sim = simulate_functional(n=61, M=2, sigma_sq=0.01, seed=33, ragged=True)
    T, NCH, first = 30, 4, 7
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(bf.SWEEP_WARM, T, seed=3)
    B = smp.get_basis()
    got = _check(smp, sim["y"], B, first, T - first, label="functional D=0")
    for q, ch in enumerate(_chains(smp)):
        post = api.post_curve_loglik(sim["y"], B, ch["nu"], ch["Phi"], ch["Z"], ch["chi"], ch["sigma_sq"], first_kept=first)
        e = R.rel_diff(got[:, q, :], post)
        print(f"chain {q}: worst |k_chain_curve_ll - k_post_cpo| / max(1, |l|) = {e.max():.3e}")
        assert e.max() <= R.GPU_TOL, q
    smp.close()


@pytest.mark.parametrize("covariance_adj", [True, False])
def test_functional_with_covariates_matches_dense(covariance_adj):
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=60, M=2, sigma_sq=0.01, seed=34)
    X = np.random.default_rng(2).standard_normal((sim["n"], 2))
    T, NCH = 24, 3
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    smp.set_covariates(X, covariance_adj=covariance_adj)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(S.SWEEP_WARM | S.COV_MEAN | (S.COV_XI if covariance_adj else 0), T, seed=3)
    _check(smp, sim["y"], smp.get_basis(), 4, T - 4, X=X, covariance_adj=covariance_adj, label=f"functional D=2 cov_adj={covariance_adj}")
    smp.close()


@pytest.mark.parametrize("NCH", [4, 1])
def test_multivariate_matches_dense(NCH):
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T = 70, 10, 3, 2, 24
    Y = rng.standard_normal((n, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    first = 6 if NCH == 4 else 0
    _check(smp, list(Y), None, first, T - first, label=f"multivariate {NCH} chains")
    smp.close()


@pytest.mark.parametrize("K,M,degs,n_int,n", [
    (2, 2, [2, 2], [2, 2], 31),        # 25 basis functions, band 12: the mid band, 32-lane groups
    (3, 2, [3, 3], [3, 3], 40),        # 49 basis functions, band 24: the wide band, 64-lane groups
])
def test_tensor_product_basis_matches_dense(K, M, degs, n_int, n):
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    T, NCH = 12, 2
    sim = simulate_tensor(n, K, M, degs, n_int, seed=311)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=max(degs), tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 5, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    _check(smp, sim["y"], sim["B"], 2, T - 2, label=f"tensor basis P={sim['P']} band={sim['band']}")
    smp.close()


def _ragged_data(n, seed, extremes=True):
    """curves on [0, 990] of very different lengths: one observation, several hundred, and in between"""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(3, 90, size=n)]
    if extremes:
        lens[0], lens[1], lens[2], lens[n - 1] = 1, 640, 2, 333
    ts = [np.sort(rng.uniform(0.0, 990.0, size=m)) for m in lens]
    ys = [np.sin(t / 150.0 + rng.uniform(0, 3)) * rng.uniform(0.5, 3) + 0.1 * rng.standard_normal(len(t)) for t in ts]
    return ts, ys


@pytest.mark.parametrize("degree,n_knots,M", [(2, 37, 3), (5, 4, 2), (1, 9, 9), (3, 5, 2)])
def test_spline_degrees_and_extreme_curve_lengths_match_dense(degree, n_knots, M):
    """degree 2 with 40 basis functions (64-lane groups), degree 5, degree 1 with n_eigen = 9, and the cubic default; every
    data set holds curves of 1, 2, 333 and 640 observations"""
    import bayesfmmm_amd as bf
    n, K, T, NCH = 37, 3, 10, 2
    ts, ys = _ragged_data(n, 50 + degree)
    ik = np.linspace(0.0, 990.0, n_knots + 2)[1:-1]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=degree, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, ys, ts, ik, [0.0, 990.0], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 9, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=9)
    _check(smp, ys, smp.get_basis(), 3, T - 3, label=f"degree {degree}, P={smp.P}, M={M}")
    smp.close()


@pytest.fixture(scope="module")
def batch():
    import bayesfmmm_amd as bf
    sim = simulate_functional(n=45, M=2, sigma_sq=0.01, seed=35, ragged=True)
    T, NCH = 120, 4
    states = _states(sim, NCH)
    smp = make_sampler_batch(sim, T, NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.set_state(**states[q])
    smp.run(bf.SWEEP_WARM, T, seed=11)
    yield smp
    smp.close()


def test_routes_equal_the_matrix_routes_bitwise(batch):
    from bayesfmmm_amd import api
    first, S = 20, 100
    ll = batch.curve_loglik(first_slot=first, n_slots=S)
    n, C = batch.n, batch.n_chains
    d = batch.curve_diagnostics(first_slot=first, n_slots=S)
    ref = api.diagnostics(np.moveaxis(ll, 0, 2).transpose(1, 0, 2))       # (n, C, S) -> (S, C, n)
    for k in DIAG:
        assert d[k].shape == (n,)
        assert d[k].tobytes() == np.ascontiguousarray(ref[k]).tobytes(), k
    loo = batch.loo(first_slot=first, n_slots=S)
    ref = api.psis_loo(ll.reshape(n, C * S))
    assert set(loo) == set(ref)
    for k in ref:
        if k in LOO_ARRAYS:
            assert loo[k].tobytes() == ref[k].tobytes(), k
        else:
            assert loo[k] == ref[k] or (np.isnan(loo[k]) and np.isnan(ref[k])), k
    assert np.all(np.isfinite(loo["pointwise_elpd_loo"]))


def test_chunks_and_repeatability(batch):
    first, S = 10, 110
    n, C = batch.n, batch.n_chains
    a, b = batch.curve_loglik(first, S), batch.curve_loglik(first, S)
    assert a.tobytes() == b.tobytes()
    # the same (curve, chain, slot) from another slot range, hence another grid and another staging batch
    c = batch.curve_loglik(first + 3, 50)
    assert c.tobytes() == np.ascontiguousarray(a[:, :, 3:53]).tobytes()
    one = batch.curve_diagnostics(first, S)
    per_row = 8 * (C * S + 7)
    few = batch.curve_diagnostics(first, S, max_workspace_bytes=per_row * 7)       # n rows in chunks of 7
    again = batch.curve_diagnostics(first, S)
    for k in DIAG:
        assert one[k].tobytes() == few[k].tobytes(), k
        assert one[k].tobytes() == again[k].tobytes(), k
    one = batch.loo(first, S)
    few = batch.loo(first, S, max_workspace_bytes=8 * C * S * 5)                    # chunks of 5 curves
    again = batch.loo(first, S)
    for k in LOO_ARRAYS:
        assert one[k].tobytes() == few[k].tobytes(), k
        assert one[k].tobytes() == again[k].tobytes(), k
    for k in ("elpd_loo", "p_loo", "elpd_waic", "n_khat_above"):
        assert one[k] == few[k], k


def test_label_and_sign_invariance():
    import bayesfmmm_amd as bf
    S = bf.sampler
    sim = simulate_functional(n=50, M=2, sigma_sq=0.01, seed=36, ragged=True)
    st = _states(sim, 1)[0]
    perm = [2, 0, 1]
    cvals = [8.0, 10.0, 12.0]
    a = make_sampler_batch(sim, 2, 1, c=cvals)
    b = make_sampler_batch(sim, 2, 1, c=[cvals[k] for k in perm])
    a.set_state(**st)
    a.run(S.U_LOGLIK, 1, seed=1)
    pst = dict(st)
    for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
        pst[nm] = np.asarray(st[nm])[perm]
    pst["Z"] = np.asarray(st["Z"])[:, perm]
    b.set_state(**pst)
    b.run(S.U_LOGLIK, 1, seed=1)
    # the slots hold what was set: b's components are a's, relabelled
    np.testing.assert_array_equal(b.get_chain("nu")[:, :, 0], a.get_chain("nu")[perm, :, 0])
    np.testing.assert_array_equal(b.get_chain("Z")[:, :, 0], a.get_chain("Z")[:, perm, 0])
    assert not np.array_equal(b.get_chain("nu")[:, :, 0], a.get_chain("nu")[:, :, 0])
    la, lb = a.curve_loglik(0, 1), b.curve_loglik(0, 1)
    e = R.rel_diff(lb, la)
    print(f"label permutation: worst relative difference {e.max():.3e}")
    assert e.max() <= R.GPU_TOL
    # against the dense form too, so that agreement is not two wrong answers
    ref = R.dense_matrix(sim["y"], a.get_basis(), _chains(a), 0, 1)
    assert R.rel_diff(la, ref).max() <= R.GPU_TOL
    # the sign of one (Phi_.m, chi_.m) pair
    fst = dict(pst)
    fst["Phi"] = np.array(pst["Phi"], copy=True)
    fst["Phi"][:, :, 1] *= -1.0
    fst["chi"] = np.array(pst["chi"], copy=True)
    fst["chi"][:, 1] *= -1.0
    b.set_state(**fst)
    b.run(S.U_LOGLIK, 1, first_iter=1, seed=1)
    np.testing.assert_array_equal(b.get_chain("Phi")[:, :, 1, 1], -b.get_chain("Phi")[:, :, 1, 0])
    lf = b.curve_loglik(1, 1)
    e = R.rel_diff(lf, lb)
    print(f"eigen-sign flip: worst relative difference {e.max():.3e}")
    assert e.max() <= R.GPU_TOL
    a.close()
    b.close()


def test_argument_checks(batch):
    from bayesfmmm_amd import _lib
    b = batch
    T = b.T
    for call in (b.curve_loglik, b.curve_diagnostics, b.loo):
        with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
            call(first_slot=T)
        with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
            call(first_slot=-1, n_slots=4)
        with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
            call(first_slot=2, n_slots=T - 1)
        with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
            call(n_slots=0)
    for call in (b.curve_diagnostics, b.loo):
        with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'"):
            call(max_workspace_bytes=64)
        with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes'"):
            call(max_workspace_bytes=-1)
    lib = b.lib
    n = b.n
    outs = [np.zeros(n) for _ in range(7)]
    p = [o.ctypes.data_as(_lib.c_double_p) for o in outs]
    big = np.zeros(n * b.n_chains * 8)
    pb = big.ctypes.data_as(_lib.c_double_p)

    def err(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    assert "'capacity'" in err(lib.bfmmm_chain_curve_loglik(b.h, 0, 8, pb, big.size - 1))
    assert "'out'" in err(lib.bfmmm_chain_curve_loglik(b.h, 0, 8, None, big.size))
    assert "'h'" in err(lib.bfmmm_chain_curve_loglik(None, 0, 8, pb, big.size))
    assert "'capacity'" in err(lib.bfmmm_chain_curve_diagnostics(b.h, 0, 8, 0, *p, n - 1))
    assert "'ess_tail'" in err(lib.bfmmm_chain_curve_diagnostics(b.h, 0, 8, 0, p[0], p[1], None, *p[3:], n))
    assert "'h'" in err(lib.bfmmm_chain_curve_diagnostics(None, 0, 8, 0, *p, n))
    assert "'capacity'" in err(lib.bfmmm_chain_loo(b.h, 0, 8, 0, *p[:6], n - 1))
    assert "'pareto_k'" in err(lib.bfmmm_chain_loo(b.h, 0, 8, 0, p[0], p[1], p[2], None, p[4], p[5], n))
    assert "'h'" in err(lib.bfmmm_chain_loo(None, 0, 8, 0, *p[:6], n))
    # the derived quantity is not a chain name
    with pytest.raises(_lib.BfmmmError, match="unknown name"):
        b.diagnostics("curve_loglik")


def test_draws_per_row_bound():
    """2^22 draws per row: 2 chains x (2^21 + 1) slots of a two-curve model (the check precedes any work on the slots)"""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    T = (1 << 21) + 1
    rng = np.random.default_rng(1)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=2, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((2, 2)), n_chains=2)
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.curve_diagnostics()
    with pytest.raises(_lib.BfmmmError, match=r"2\^22"):
        smp.loo()
    smp.close()
