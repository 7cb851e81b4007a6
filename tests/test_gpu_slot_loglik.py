"""Sampler.slot_loglik (bfmmm_chain_slot_loglik, k_slot_rss + k_slot_ll_reduce) against the long-double restatement
from the observations (tests/slot_ll_ref.py) and against the "loglik" array the run itself stored, at the smallest shapes at which
the kernel can go wrong:
  * 13 ragged curves, cubic P = 8, 3 chains x 7 slots from slot 2: n no multiple of the 8 curves of a workgroup, S no multiple of
    the 16 staged draws; the same with D = 2 covariates in both modes (eta alone, eta and xi)
  * multivariate P = 5 (the integer division bites) and P = 64 (64-lane groups, band 0)
  * the 5 x 5 quadratic tensor basis (band 12: the record's G part in LDS)
  * K = 8, n_eigen = 16, P = 64 with 3 curves: the build limits.  The sweep does not fit that shape (its LDS), so no run stores
    a "loglik" there: the slots are loaded with set_chain and the kernel is held to the restatement alone.
Both comparisons hold |difference| <= 1e-10 (|ref| + N_obs): 1e-10 is the relative tolerance FLLik is held to against the oracle, and
the N_obs term keeps a log-likelihood near zero from turning it into an absolute demand.  Per curve the same with the curve's n_i.
Then: per-curve rows, chunking, repeatability, store and the refusals."""
import numpy as np
import pytest

import slot_ll_ref as R
from test_gpu_set_chain import data, make, run, chains_of, same, K, M, T, N

pytestmark = pytest.mark.gpu

REF_NAMES = ["nu", "Phi", "Z", "chi", "sigma_sq"]


def check(smp, Y, B, first, S, X=None, covariance_adj=False, label="", own=True):
    """slot_loglik of the range against the restatement (totals and curve by curve) and, with `own`, against the stored "loglik";
    prints the largest errors in units of the bound before it asserts.  Returns (totals, per-curve, restatement)."""
    chains = chains_of(smp, REF_NAMES + (["eta", "xi"] if X is not None else []) + ["loglik"])
    ref_curve = R.curve_matrix(Y, B, chains, first, S, X=X, covariance_adj=covariance_adj)
    ref = R.totals(ref_curve).astype(np.float64)
    assert np.all(np.isfinite(ref)), label
    N_obs = R.n_obs(Y)
    got = smp.slot_loglik(first_slot=first, n_slots=S)
    assert got.shape == (smp.n_chains, S)
    both = smp.slot_loglik(first_slot=first, n_slots=S, per_curve=True)
    same(both["loglik"], got, label + ": totals with per_curve")
    cur = both["curve"]
    assert cur.shape == (smp.n, smp.n_chains, S)
    err = np.abs(got - ref) / R.bound(ref, N_obs)
    ni = np.array([np.asarray(y).size for y in Y], dtype=np.float64)[:, None, None]
    refc = ref_curve.astype(np.float64)
    err_c = np.abs(cur - refc) / (1e-10 * (np.abs(refc) + ni))
    err_s = np.abs(cur.sum(axis=0) - got) / R.bound(got, N_obs)
    msg = f"{label}: |kernel - long double| = {err.max():.3e} of the bound (largest {np.abs(got - ref).max():.3e} at |ll| up to {np.abs(ref).max():.3e}); per curve {err_c.max():.3e}; rows to totals {err_s.max():.3e}"
    if own:
        stored = np.stack([ch["loglik"][first:first + S] for ch in chains])
        err_o = np.abs(stored - ref) / R.bound(ref, N_obs)
        err_k = np.abs(stored - got) / R.bound(got, N_obs)
        msg += f"; |run's own - long double| = {err_o.max():.3e} of the bound (largest {np.abs(stored - ref).max():.3e}); |run's own - kernel| = {err_k.max():.3e}"
    print(msg)
    assert err.max() <= 1.0 and err_c.max() <= 1.0 and err_s.max() <= 1.0, label
    if own:
        assert err_o.max() <= 1.0 and err_k.max() <= 1.0, label
    return got, cur, ref


@pytest.fixture(scope="module")
def base():
    ts, ys = data()
    smp = make(ts, ys, 3)
    run(smp, [0, 1, 2])
    yield smp, ts, ys
    smp.close()


def test_functional_ragged(base):
    smp, ts, ys = base
    check(smp, ys, smp.get_basis(), 2, 7, label="functional n=13 P=8, 3 x 7 from slot 2")
    check(smp, ys, smp.get_basis(), 0, T, label="functional, every slot")


@pytest.mark.parametrize("covariance_adj", [False, True])
def test_functional_with_covariates(covariance_adj):
    import bayesfmmm_amd as bf
    S_ = bf.sampler
    ts, ys = data()
    X = np.random.default_rng(3).standard_normal((N, 2))
    smp = make(ts, ys, 3)
    smp.set_covariates(X, covariance_adj=covariance_adj)
    run(smp, [0, 1, 2], mask=S_.SWEEP_WARM | S_.COV_MEAN | (S_.COV_XI if covariance_adj else 0))
    check(smp, ys, smp.get_basis(), 2, 7, X=X, covariance_adj=covariance_adj, label=f"functional D=2 covariance_adj={covariance_adj}")
    smp.close()


@pytest.mark.parametrize("P", [5, 64])
def test_multivariate(P):
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, NCH = 9, 3
    Y = rng.standard_normal((n, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    run(smp, list(range(NCH)), seed=17)
    # (P = 5: the restatement divides as the reference does, P // 2 = 2; tests/test_slot_ll_ref.py shows that this bites)
    check(smp, list(Y), None, 2, 7, label=f"multivariate P={P}")
    smp.close()


def test_tensor_basis_wide_band():
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    sim = simulate_tensor(11, 2, 2, [2, 2], [2, 2], seed=311)
    assert sim["P"] == 25 and sim["band"] == 12
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=2, n_eigen=2, basis_degree=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=2)
    run(smp, [0, 1], seed=5)
    check(smp, sim["y"], sim["B"], 2, 7, label="5 x 5 quadratic tensor basis, band 12")
    smp.close()


def test_build_limits_on_loaded_draws():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(8)
    K_, M_, P_, T_, n = 8, 16, 64, 5, 3
    ik = np.linspace(0.0, 990.0, P_ - 4 + 2)[1:-1]
    ts = [np.sort(rng.uniform(0.0, 990.0, size=m)) for m in (70, 131, 64)]
    ys = [np.sin(t / 90.0) + 0.3 * rng.standard_normal(len(t)) for t in ts]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K_, n_eigen=M_, basis_degree=3, tot_mcmc_iters=T_)
    smp = bf.Sampler(cfg, ys, ts, ik, [0.0, 990.0], n_chains=2)
    assert smp.P == P_
    for q in range(2):
        smp.load_chain({"nu": 0.3 * rng.standard_normal((K_, P_, T_)), "Phi": 0.05 * rng.standard_normal((K_, P_, M_, T_)),
                        "Z": rng.dirichlet(np.ones(K_), size=(n, T_)).transpose(0, 2, 1), "chi": rng.standard_normal((n, M_, T_)),
                        "sigma_sq": rng.uniform(0.05, 0.5, T_)}, chain=q)
    check(smp, ys, smp.get_basis(), 1, 3, label="K=8 M=16 P=64, loaded draws", own=False)
    smp.close()


def test_chunks_repeats_and_timers(base):
    smp, _, _ = base
    first, S = 2, 7
    one = smp.slot_loglik(first_slot=first, n_slots=S, per_curve=True)
    assert smp.timing("slot_loglik")[1] == 1 and smp.timing("slot_loglik_reduce")[1] == 1
    NB = 8 * smp.n_chains * S
    small = smp.slot_loglik(first_slot=first, n_slots=S, per_curve=True, max_workspace_bytes=NB + 5 * NB)      # 5 curves a chunk: 3 chunks
    assert smp.timing("slot_loglik")[1] == 3 and smp.timing("slot_loglik_reduce")[1] == 3
    same(small, one, "three chunks against one")
    single = smp.slot_loglik(first_slot=first, n_slots=S, max_workspace_bytes=2 * NB)                             # a curve a chunk
    assert smp.timing("slot_loglik")[1] == N
    same(single, one["loglik"], "thirteen chunks against one")
    same(smp.slot_loglik(first_slot=first, n_slots=S, per_curve=True), one, "a second call")
    assert smp.timing("slot_loglik")[0] > 0.0


def test_store_writes_the_range_alone():
    ts, ys = data()
    smp = make(ts, ys, 2)
    run(smp, [0, 1])
    before = chains_of(smp)
    marked = np.full(T, -7.0)
    for q in range(2):
        smp.set_chain("loglik", marked, chain=q)
    got = smp.slot_loglik(first_slot=3, n_slots=4)
    same([c["loglik"] for c in chains_of(smp, ["loglik"])], [marked, marked], "without store")
    same(smp.slot_loglik(first_slot=3, n_slots=4, store=True), got, "with store")
    after = chains_of(smp)
    for q in range(2):
        same(after[q]["loglik"][3:7], got[q], "stored")
        same(after[q]["loglik"][:3], marked[:3], "below the range")
        same(after[q]["loglik"][7:], marked[7:], "above the range")
        for nm in before[q]:
            if nm != "loglik":
                same(after[q][nm], before[q][nm], nm)
    smp.close()


def test_refusals(base):
    from bayesfmmm_amd import _lib
    smp, _, _ = base
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_slot_loglik: 'first_slot' out of range"):
        smp.slot_loglik(first_slot=T)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_slot_loglik: 'n_slots' out of range"):
        smp.slot_loglik(first_slot=2, n_slots=T - 1)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_slot_loglik: 'n_slots' out of range"):
        smp.slot_loglik(n_slots=0)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_slot_loglik: 'max_workspace_bytes' must not be negative"):
        smp.slot_loglik(max_workspace_bytes=-1)
    NB = 8 * smp.n_chains * T
    with pytest.raises(_lib.BfmmmError, match=rf"bfmmm_chain_slot_loglik: 'max_workspace_bytes' below the {2 * NB} bytes one curve needs \({NB} shared by all curves \+ {NB} per curve\)"):
        smp.slot_loglik(max_workspace_bytes=2 * NB - 1)
    ll, cv = np.zeros((smp.n_chains, T)), np.zeros((smp.n, smp.n_chains, T))
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    with pytest.raises(_lib.BfmmmError, match=f"bfmmm_chain_slot_loglik: 'capacity' below {ll.size} entries"):
        _lib.check(smp.lib.bfmmm_chain_slot_loglik(smp.h, 0, T, 0, 0, dp(ll), None, ll.size - 1))
    with pytest.raises(_lib.BfmmmError, match=f"bfmmm_chain_slot_loglik: 'capacity' below {cv.size} entries"):
        _lib.check(smp.lib.bfmmm_chain_slot_loglik(smp.h, 0, T, 0, 0, dp(ll), dp(cv), cv.size - 1))
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_slot_loglik: 'loglik' is null"):
        _lib.check(smp.lib.bfmmm_chain_slot_loglik(smp.h, 0, T, 0, 0, None, None, ll.size))
