"""Sampler.set_chain / load_chain (bfmmm_set_chain): a chain copied get_chain -> set_chain into a fresh sampler
reads back bit for bit and gives every chain-slot summary the bits of the sampler that ran it; a window write touches its slots
alone; the working state is never touched; two single-chain runs pooled into a 2-chain sampler give the bits of the 2-chain batch
run; every refusal comes with its message; the covariate blocks exist once covariates were set.
Shape: 13 curves of 5 .. 40 points, cubic splines with P = 8, K = 3, n_eigen = 2, T = 12."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["nu", "chi", "Z", "pi", "alpha_3", "delta", "A", "sigma_sq", "gamma", "Phi", "loglik", "tau"]
COV_NAMES = ["eta", "xi", "tau_eta", "gamma_xi", "delta_xi", "A_xi"]
STATE = ["nu", "Phi", "chi", "Z", "delta", "A", "gamma", "pi", "tau", "alpha_3", "sigma_sq", "loglik"]
K, M, T, N = 3, 2, 12, 13
IK, BK = [200.0, 400.0, 600.0, 800.0], [0.0, 990.0]


def data(seed=21, n=N):
    rng = np.random.default_rng(seed)
    lens = [5, 40] + [int(v) for v in rng.integers(6, 40, size=n - 2)]
    ts = [np.sort(rng.uniform(0.0, 990.0, size=m)) for m in lens]
    ys = [np.sin(t / 150.0 + rng.uniform(0, 3)) * rng.uniform(0.5, 3) + 0.1 * rng.standard_normal(len(t)) for t in ts]
    return ts, ys


def make(ts, ys, n_chains, T_=T):
    import bayesfmmm_amd as bf
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=3, tot_mcmc_iters=T_)
    return bf.Sampler(cfg, ys, ts, IK, BK, n_chains=n_chains)


def run(smp, ids, seed=9, mask=None):
    import bayesfmmm_amd as bf
    for q, cid in enumerate(ids):
        smp.select_chain(q)
        smp.init_state(1, seed, chain=cid)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM if mask is None else mask, smp.T, seed=seed, chain=ids[0])


def chains_of(smp, names=NAMES):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_chain(nm) for nm in names})
    smp.select_chain(0)
    return out


def states_of(smp):
    out = []
    for q in range(smp.n_chains):
        smp.select_chain(q)
        out.append({nm: smp.get_state(nm) for nm in STATE})
    smp.select_chain(0)
    return out


def same(a, b, label=""):
    """bit for bit, through dicts, lists, arrays and scalars"""
    if isinstance(a, dict):
        assert set(a) == set(b), label
        for k in a:
            same(a[k], b[k], f"{label}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), label
        for j, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{label}[{j}]")
    elif a is None or b is None:
        assert a is None and b is None, label
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape, label
        assert np.array_equal(x, y, equal_nan=True), label


@pytest.fixture(scope="module")
def pair():
    """A ran two chains; B is fresh and holds A's chains through get_chain -> set_chain"""
    ts, ys = data()
    A = make(ts, ys, 2)
    run(A, [0, 1])
    B = make(ts, ys, 2)
    run_state = states_of(B)
    chA = chains_of(A)
    for q in range(2):
        assert B.load_chain(chA[q], chain=q) == T
    yield A, B, chA, run_state, (ts, ys)
    A.close()
    B.close()


def test_round_trip_is_bitwise_and_leaves_the_state(pair):
    A, B, chA, state0, _ = pair
    same(chains_of(B), chA, "chains")
    same(states_of(B), state0, "working state")
    assert B.lib.bfmmm_selected_chain(B.h) == 0


def test_summaries_agree_bitwise(pair):
    A, B, _, _, _ = pair
    E = A.get_basis()[1][::5]
    for label, call in (("diagnostics sigma_sq", lambda s: s.diagnostics("sigma_sq")), ("diagnostics tau", lambda s: s.diagnostics("tau")),
                        ("curve_bands", lambda s: s.curve_bands(E)), ("similarity", lambda s: s.similarity()), ("loo", lambda s: s.loo()),
                        ("align", lambda s: s.align())):
        same(call(A), call(B), label)


def test_window_write_touches_its_slots_alone(pair):
    _, _, chA, _, (ts, ys) = pair
    Cw = make(ts, ys, 2)
    before = chains_of(Cw)
    state0 = states_of(Cw)
    for nm in NAMES:
        v = chA[1][nm]
        assert Cw.set_chain(nm, v[5:8] if nm == "tau" else v[..., 5:8], first_slot=5, chain=1) == 3
    after = chains_of(Cw)
    same(after[0], before[0], "the other chain")
    for nm in NAMES:
        sl = (lambda a, lo, hi: a[lo:hi]) if nm == "tau" else (lambda a, lo, hi: a[..., lo:hi])
        same(sl(after[1][nm], 5, 8), sl(chA[1][nm], 5, 8), nm)
        same(sl(after[1][nm], 0, 5), sl(before[1][nm], 0, 5), nm + " below")
        same(sl(after[1][nm], 8, T), sl(before[1][nm], 8, T), nm + " above")
    same(states_of(Cw), state0, "working state")
    Cw.close()


def test_pooling_single_chain_runs_gives_the_batch_bits(pair):
    A, _, chA, _, (ts, ys) = pair
    pool = make(ts, ys, 2)
    for q in range(2):
        solo = make(ts, ys, 1)
        run(solo, [q])
        ch = chains_of(solo)[0]
        same(ch, chA[q], f"stand-alone chain {q}")      # the header's promise, which the pooling rests on
        pool.load_chain(ch, chain=q)
        solo.close()
    same(pool.diagnostics("sigma_sq"), A.diagnostics("sigma_sq"), "diagnostics")
    same(pool.similarity(), A.similarity(), "similarity")
    pool.close()


def test_refusals(pair):
    from bayesfmmm_amd import _lib
    _, _, chA, _, (ts, ys) = pair
    s = make(ts, ys, 1)
    before = chains_of(s)[0]
    lib, dp = s.lib, lambda a: a.ctypes.data_as(_lib.c_double_p)
    v = np.ones(T)
    with pytest.raises(_lib.BfmmmError, match="bfmmm_set_chain: 'h' is null"):
        _lib.check(lib.bfmmm_set_chain(None, b"sigma_sq", 0, T, dp(v), T))
    with pytest.raises(_lib.BfmmmError, match="bfmmm_set_chain: 'name' is null"):
        _lib.check(lib.bfmmm_set_chain(s.h, None, 0, T, dp(v), T))
    with pytest.raises(_lib.BfmmmError, match="bfmmm_set_chain: 'values' is null"):
        _lib.check(lib.bfmmm_set_chain(s.h, b"sigma_sq", 0, T, None, T))
    with pytest.raises(_lib.BfmmmError, match="bfmmm_set_chain: unknown name 'bogus'"):
        s.set_chain("bogus", v)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_set_chain\(sigma_sq\): 'first_slot' out of range"):
        s.set_chain("sigma_sq", v[:1], first_slot=T)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_set_chain\(sigma_sq\): 'first_slot' out of range"):
        s.set_chain("sigma_sq", v[:1], first_slot=-1)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_set_chain\(sigma_sq\): 'n_slots' out of range"):
        s.set_chain("sigma_sq", v, first_slot=1)
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_set_chain\(sigma_sq\): 'n_slots' out of range"):
        _lib.check(lib.bfmmm_set_chain(s.h, b"sigma_sq", 0, 0, dp(v), 0))
    with pytest.raises(_lib.BfmmmError, match=rf"bfmmm_set_chain\(Z\): 'count' must be {N * K * 4} \({N * K} entries x 4 slots\), got {N * K * 4 - 1}"):
        _lib.check(lib.bfmmm_set_chain(s.h, b"Z", 0, 4, dp(np.ones(N * K * 4)), N * K * 4 - 1))
    Z = np.array(chA[0]["Z"][..., :4])
    Z[7, 1, 2] = np.nan
    with pytest.raises(_lib.BfmmmError, match=rf"bfmmm_set_chain\(Z\): value at slot 5, entry {7 + N * 1} is not finite"):
        s.set_chain("Z", Z, first_slot=3)
    tau = np.ones((4, K))
    tau[3, 2] = np.inf
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_set_chain\(tau\): value at slot 4, entry 2 is not finite"):
        s.set_chain("tau", tau, first_slot=1)
    sg = np.ones(5)
    sg[2] = 0.0
    with pytest.raises(_lib.BfmmmError, match=r"bfmmm_set_chain\(sigma_sq\): value at slot 2, entry 0 is not positive"):
        s.set_chain("sigma_sq", sg)
    sg[2] = -1.0
    with pytest.raises(_lib.BfmmmError, match="is not positive"):
        s.set_chain("sigma_sq", sg)
    # nothing was written by a refused call; no simplex check on Z
    same(chains_of(s)[0], before, "slots after the refused calls")
    s.set_chain("Z", 3.0 * np.abs(chA[0]["Z"]) - 1.0)
    # the Python layer: shapes, and arrays that disagree on the number of draws
    with pytest.raises(ValueError, match="values must be shaped"):
        s.set_chain("Z", np.ones((N, K + 1, 2)))
    with pytest.raises(ValueError, match="disagree on the number of draws"):
        s.load_chain({"sigma_sq": np.ones(3), "tau": np.ones((4, K))})
    s.close()


def test_covariate_blocks_exist_once_covariates_were_set():
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    S = bf.sampler
    ts, ys = data()
    X = np.random.default_rng(3).standard_normal((N, 2))
    A = make(ts, ys, 2)
    A.set_covariates(X, covariance_adj=True)
    run(A, [0, 1], mask=S.SWEEP_WARM | S.COV_MEAN | S.COV_XI)
    chA = chains_of(A, NAMES + COV_NAMES)
    B = make(ts, ys, 2)
    one = np.ones(4)
    for nm in COV_NAMES:      # (through the library: without covariates the Python layer has no shape for them either)
        with pytest.raises(_lib.BfmmmError, match=f"bfmmm_set_chain: unknown name '{nm}'"):
            _lib.check(B.lib.bfmmm_set_chain(B.h, nm.encode(), 0, 1, one.ctypes.data_as(_lib.c_double_p), one.size))
    B.set_covariates(X, covariance_adj=True)
    for q in range(2):
        B.load_chain(chA[q], chain=q)
    same(chains_of(B, NAMES + COV_NAMES), chA, "chains with covariates")
    same(B.curve_loglik(), A.curve_loglik(), "curve_loglik with covariates")
    A.close()
    B.close()
