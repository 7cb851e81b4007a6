"""Leave-block-out PSIS cross-validation within curves on the device (k_loo_blocks, bfmmm_chain_loo_blocks): the four
traces of Sampler.loo_blocks against explicit Gaussian conditioning on the dense n_i x n_i covariance (tests/loo_blocks_ref.dense,
fed the get_chain copies), every block and row; the pooled outputs against psis_ref / expect run on the device's own traces;
singletons against loo_pointwise and whole-curve blocks against curve_loglik on the same sampler; the three spellings bit for bit;
bit invariance under chunking, sub-lists, reversal, slot ranges and tracing; label and sign invariance; the argument checks.  The
tolerances are loo_blocks_ref.GPU_TOL_*: ten times the floors the two forms impose on each other (tests/test_loo_blocks_ref.py),
not figures taken from the kernel."""
import ctypes as C
import re

import numpy as np
import pytest

import curve_ll_ref as CL
import loo_blocks_ref as R
import loo_pointwise_ref as LP
import psis_ref
from test_gpu_loo_pointwise import EDGE_LENS, LOO_ARRAYS, TRACES, _chains, _lens, _spline_sampler

pytestmark = pytest.mark.gpu

ROW_KEYS = ("pit", "mean", "sd")
ROW_TRACES = ("pit_trace", "mean_trace", "var_trace")


def _check(smp, Y, B, blocks, first, S, X=None, covariance_adj=False, label=""):
    """the traces against `dense`, every block and row; the pooled outputs against the restatements run on the device's traces"""
    from bayesfmmm_amd import api
    res = smp.loo_blocks(blocks=blocks, first_slot=first, n_slots=S, trace=True)
    bc, off, obs = res["block_curve"], res["offsets"], res["obs"]
    nb, N, Cn = len(blocks), int(off[-1]), smp.n_chains
    assert [int(i) for i in bc] == [int(i) for i, _ in blocks]
    np.testing.assert_array_equal(obs, np.concatenate([np.array(list(ix)) for _, ix in blocks]))
    np.testing.assert_array_equal(res["block_size"], np.diff(off))
    assert res["loglik_trace"].shape == (nb, Cn, S)
    for k in ROW_TRACES:
        assert res[k].shape == (N, Cn, S), k
    l, pit, m, v, z = R.dense_traces(Y, B, _chains(smp, X is not None), first, S, bc, off, obs, X, covariance_adj)
    assert np.all(np.isfinite(l)) and np.all(v > 0), label
    errs = {"l": (R.rel_diff(res["loglik_trace"], l), R.GPU_TOL_L), "Phi(z)": (np.abs(res["pit_trace"] - pit), R.GPU_TOL_PIT),
            "m": (R.rel_diff(res["mean_trace"], m), R.GPU_TOL_M), "sqrt v": (R.rel_diff(np.sqrt(res["var_trace"]), np.sqrt(v)), R.GPU_TOL_SD)}
    for k, (e, tol) in errs.items():
        print(f"{label}: worst |device - dense| of {k} = {e.max():.3e} (tolerance {tol:.1e}) over {e.size} values")
    for k, (e, tol) in errs.items():
        assert e.max() <= tol, (label, k, float(e.max()), np.unravel_index(np.argmax(e), e.shape))
    # pooled: PSIS of the blocks and the expectations of the rows under their block's weights, from the device's own traces
    ll = res["loglik_trace"].reshape(nb, Cn * S)
    ref = psis_ref.psis_loo(ll)
    scale = max(1.0, float(np.max(np.abs(ref["lppd"]))))
    for k in LOO_ARRAYS:
        assert res[k].shape == (nb,), k
        if k != "pareto_k":
            np.testing.assert_allclose(res[k], ref[k], rtol=1e-8, atol=1e-8 * scale, err_msg=k)
    kg, kr = res["pareto_k"], ref["pareto_k"]
    np.testing.assert_array_equal(np.isinf(kg), np.isinf(kr))
    np.testing.assert_allclose(kg[np.isfinite(kr)], kr[np.isfinite(kr)], rtol=0, atol=1e-6)
    blk = np.repeat(np.arange(nb), np.diff(off))
    mt, second = res["mean_trace"].reshape(N, -1), (res["mean_trace"] ** 2 + res["var_trace"]).reshape(N, -1)
    e = np.array([LP.expect(ll[blk[r]], np.vstack([res["pit_trace"].reshape(N, -1)[r], mt[r], second[r]])) for r in range(N)])
    np.testing.assert_allclose(res["pit"], e[:, 0], rtol=1e-8, atol=1e-8)
    assert np.all(np.abs(res["mean"] - e[:, 1]) <= 1e-8 * np.abs(e[:, 1]) + 1e-8 * np.max(np.abs(mt), axis=1))
    sd_ref = np.sqrt(np.maximum(0.0, e[:, 2] - e[:, 1] ** 2))
    assert np.all(sd_ref > 0)
    assert np.all(np.abs(res["sd"] - sd_ref) <= 1e-8 * (e[:, 2] + 2.0 * e[:, 1] ** 2) / (2.0 * sd_ref) + 1e-8 * sd_ref)
    assert np.all((res["pit"] >= 0) & (res["pit"] <= 1))
    # totals over the blocks and sums per distinct curve, in order of first appearance
    tot = api.loo_totals({k: res[k] for k in LOO_ARRAYS}, Cn * S)
    for k, val in tot.items():
        if k not in LOO_ARRAYS:
            assert res[k] == val or (np.isnan(res[k]) and np.isnan(val)), k
    first_seen = list(dict.fromkeys(int(i) for i in bc))
    np.testing.assert_array_equal(res["curve_index"], first_seen)
    np.testing.assert_array_equal(res["curve_elpd_loo"], [res["pointwise_elpd_loo"][bc == i].sum() for i in first_seen])
    return res


def _with_len(lens, m):
    return [i for i, v in enumerate(lens) if v == m][0]


def _edge_blocks(lens):
    """the block list of the issue: every size at a boundary, a tile filled to exactly 64 rows by several blocks, a block that
    would make 65 rows, whole-curve blocks, a scattered one, one in decreasing order, two overlapping, curves at two places"""
    c130, c65, c64, c63, c17, c1 = (_with_len(lens, m) for m in (130, 65, 64, 63, 17, 1))
    short = [i for i, v in enumerate(lens) if 3 <= v <= 12][:2]
    return [(c130, range(0, 1)), (c130, [5, 6]), (c130, range(10, 25)), (c130, range(30, 46)), (c130, range(50, 67)),
            (c130, range(70, 83)),                                  # 1 + 2 + 15 + 16 + 17 + 13 = 64 rows: the tile is full
            (c130, range(0, 63)), (c130, [100, 101]),               # 63 + 2 = 65: the second opens the next tile
            (c130, range(66, 130)),                                 # 64 rows, a tile of its own
            (c64, range(64)), (c1, [0]),                            # whole curves
            (c130, range(0, 130, 3)),                               # scattered; the curve again, after two others
            (c65, range(40, 20, -1)), (c65, range(25, 45)),         # decreasing order; overlapping the one before
            (c63, range(3, 20)), (c17, range(17)), (short[0], range(lens[short[0]])), (short[1], [1, 0]),
            (c63, range(50, 63))]                                   # the 63-point curve at a second, non-adjacent place


@pytest.fixture(scope="module")
def batch():
    """P = 12, K = 3, M = 2, four chains of 30 slots, 40 ragged curves with every edge length"""
    lens = _lens(40, EDGE_LENS, 1)
    smp, ys = _spline_sampler(lens, 3, 8, 3, 2, 30, 4, seed=11)
    yield smp, ys, lens
    smp.close()


def test_edge_blocks_match_dense(batch):
    smp, ys, lens = batch
    blocks = _edge_blocks(lens)
    sizes = [len(list(ix)) for _, ix in blocks]
    assert smp.P == 12 and {1, 2, 15, 16, 17, 63, 64} <= set(sizes) and sum(sizes[:6]) == 64 and sizes[6] + sizes[7] == 65
    _check(smp, ys, smp.get_basis(), blocks, 22, 8, label="P=12 K=3 M=2 C=4")


def _sized_blocks(lens, sizes, seed):
    """one contiguous block of every size, on the first curve long enough, at a random place; then every third point of the
    longest curve and the first curve whole (its first 64 observations where it is longer)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in sizes:
        i = [j for j, v in enumerate(lens) if v >= s][0]
        st = int(rng.integers(0, lens[i] - s + 1))
        out.append((i, range(st, st + s)))
    i = int(np.argmax(lens))
    return out + [(i, range(1, lens[i], 3)), (0, range(min(lens[0], 64)))]


@pytest.mark.parametrize("K,M,degree,n_knots,edge,sizes", [
    (2, 16, 2, 37, [1, 2, 17, 65], [1, 17, 64]),      # P = 40: ten k-steps; M + 1 = 17: the second column tile
    (2, 1, 3, 8, [1, 16, 64], [1, 16, 5, 64]),        # M = 1
])
def test_shapes_match_dense(K, M, degree, n_knots, edge, sizes):
    lens = _lens(12, edge, 2)
    smp, ys = _spline_sampler(lens, degree, n_knots, K, M, 8, 1, seed=7)
    _check(smp, ys, smp.get_basis(), _sized_blocks(lens, sizes, 1), 2, 6, label=f"P={smp.P} K={K} M={M} C=1")
    smp.close()


@pytest.mark.parametrize("covariance_adj", [True, False])
def test_covariates_match_dense(covariance_adj):
    lens = _lens(12, [1, 17, 65], 3)
    X = np.random.default_rng(2).standard_normal((len(lens), 2))
    smp, ys = _spline_sampler(lens, 3, 8, 3, 2, 8, 2, seed=5, X=X, covariance_adj=covariance_adj)
    _check(smp, ys, smp.get_basis(), _sized_blocks(lens, [1, 17, 40], 2), 3, 5, X=X, covariance_adj=covariance_adj,
           label=f"D=2 cov_adj={covariance_adj}")
    smp.close()


def test_tensor_product_basis_matches_dense():
    """a create_from_basis handle: the basis rows are gathered from the handle's host copy, chunk by chunk"""
    import bayesfmmm_amd as bf
    from test_gpu_tensor import simulate_tensor
    K, M, T, NCH = 2, 2, 8, 2
    sim = simulate_tensor(10, K, M, [2, 2], [2, 2], seed=311, n_pts=90)       # 25 basis functions, band 12; 45 to 90 points a curve
    lens = [len(y) for y in sim["y"]]
    assert max(lens) > 64
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=2, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, sim["y"], basis=sim["B"], band=sim["band"], penalty=sim["Pmat"], penalty_band=sim["pen_band"], n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 5, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=5)
    blocks = _sized_blocks(lens, [1, 30, 40, 64], 3) + [(3, range(lens[3] - 1, lens[3] - 21, -1)), (9, [0, 7, 2])]
    one = _check(smp, sim["y"], sim["B"], blocks, 2, 6, label=f"tensor basis P={sim['P']} band={sim['band']}")
    few = smp.loo_blocks(blocks=blocks, first_slot=2, n_slots=6, trace=True, max_workspace_bytes=_tile_budget(smp, blocks, 2, 6, 2))
    for k in LOO_ARRAYS + TRACES + ROW_KEYS:
        assert one[k].tobytes() == few[k].tobytes(), k
    smp.close()


def test_multivariate_blocks_of_coordinates_match_dense():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(4)
    n, P, K, M, T, NCH = 30, 10, 3, 2, 10, 2
    Y = rng.standard_normal((n, P))
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, Y, n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 17, chain=q)
    smp.run(bf.SWEEP_WARM, T, seed=17)
    blocks = [(i, [int(v) for v in rng.permutation(P)[:1 + i % P]]) for i in range(n)] + [(2, range(P)), (2, [9, 0])]
    res = _check(smp, list(Y), None, blocks, 4, 6, label="multivariate")
    assert res["pit"].shape == (sum(len(ix) for _, ix in blocks),)
    smp.close()


def test_singletons_match_loo_pointwise(batch):
    smp, ys, lens = batch
    first, S = 3, 9
    pw = smp.loo_pointwise(first_slot=first, n_slots=S, trace=True)
    bl = smp.loo_blocks(block_size=1, first_slot=first, n_slots=S, trace=True)
    assert bl["loglik_trace"].shape == pw["loglik_trace"].shape
    np.testing.assert_array_equal(bl["offsets"], np.arange(sum(lens) + 1))
    z_tol = LP.GPU_TOL_PIT
    errs = {"l": (R.rel_diff(bl["loglik_trace"], pw["loglik_trace"]), LP.GPU_TOL_L), "Phi(z)": (np.abs(bl["pit_trace"] - pw["pit_trace"]), z_tol),
            "m": (R.rel_diff(bl["mean_trace"], pw["mean_trace"]), LP.GPU_TOL_M),
            "sqrt v": (R.rel_diff(np.sqrt(bl["var_trace"]), np.sqrt(pw["var_trace"])), LP.GPU_TOL_SD)}
    for k, (e, tol) in errs.items():
        print(f"singletons against loo_pointwise: worst difference of {k} = {e.max():.3e} (tolerance {tol:.1e})")
    for k, (e, tol) in errs.items():
        assert e.max() <= tol, k


def test_whole_curve_blocks_match_curve_loglik(batch):
    smp, ys, lens = batch
    first, S = 3, 9
    sel = [i for i, v in enumerate(lens) if v <= 64]
    assert {1, 2, 15, 16, 17, 63, 64} <= {lens[i] for i in sel}
    res = smp.loo_blocks(blocks=[(i, range(lens[i])) for i in sel], first_slot=first, n_slots=S, trace=True)
    cl = smp.curve_loglik(first_slot=first, n_slots=S)
    e = R.rel_diff(res["loglik_trace"], cl[sel])
    print(f"whole-curve blocks against curve_loglik: worst relative difference {e.max():.3e} (tolerance {CL.GPU_TOL + R.GPU_TOL_L:.1e})")
    assert e.max() <= CL.GPU_TOL + R.GPU_TOL_L


def test_spellings_agree_bit_for_bit(batch):
    smp, ys, lens = batch
    first, S = 7, 6
    keys = LOO_ARRAYS + TRACES + ROW_KEYS + ("offsets", "block_curve", "obs", "curve_elpd_loo", "curve_index")
    curves = [35, 3, 22, 35]
    a = smp.loo_blocks(block_size=10, curves=curves, first_slot=first, n_slots=S, trace=True)
    spelled = [(i, range(j, min(j + 10, lens[i]))) for i in curves for j in range(0, lens[i], 10)]
    b = smp.loo_blocks(blocks=spelled, first_slot=first, n_slots=S, trace=True)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    long_ = [i for i, v in enumerate(lens) if v > 5]
    a = smp.loo_blocks(horizon=5, curves=long_, first_slot=first, n_slots=S, trace=True)
    b = smp.loo_blocks(blocks=[(i, range(lens[i] - 5, lens[i])) for i in long_], first_slot=first, n_slots=S, trace=True)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    with pytest.raises(ValueError, match="not more than the horizon"):
        smp.loo_blocks(horizon=5, first_slot=first, n_slots=S)


def _tile_budget(smp, blocks, first, S, tiles):
    """max_workspace_bytes for chunks of `tiles` row tiles, from the plan the refusal of a one-byte budget states"""
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' below") as ei:
        smp.loo_blocks(blocks=blocks, first_slot=first, n_slots=S, max_workspace_bytes=1)
    shared, per = (int(v) for v in re.search(r"\((\d+) shared by all tiles \+ (\d+) per tile\)", str(ei.value)).groups())
    return shared + tiles * per


def _rows_of(off, ks):
    return np.concatenate([np.arange(off[k], off[k + 1]) for k in ks])


def test_bit_invariance(batch):
    smp, ys, lens = batch
    first, S = 5, 21
    blocks = _edge_blocks(lens)
    nb = len(blocks)
    one = smp.loo_blocks(blocks=blocks, first_slot=first, n_slots=S, trace=True)
    again = smp.loo_blocks(blocks=blocks, first_slot=first, n_slots=S, trace=True)
    few = smp.loo_blocks(blocks=blocks, first_slot=first, n_slots=S, trace=True, max_workspace_bytes=_tile_budget(smp, blocks, first, S, 3))
    keys = LOO_ARRAYS + TRACES + ROW_KEYS + ("curve_elpd_loo",)
    for k in keys:
        assert one[k].tobytes() == again[k].tobytes(), k
        assert one[k].tobytes() == few[k].tobytes(), k
    assert one["elpd_loo"] == few["elpd_loo"] and one["n_khat_above"] == few["n_khat_above"]
    # without the traces the same values
    plain = smp.loo_blocks(blocks=blocks, first_slot=first, n_slots=S)
    assert not any(k in plain for k in TRACES)
    for k in LOO_ARRAYS + ROW_KEYS:
        assert one[k].tobytes() == plain[k].tobytes(), k
    # a sub-list and the list reversed: other tiles, other neighbours; the blocks keep their bits, the rows permute
    off = one["offsets"]
    for ks in (list(range(1, nb, 2)), list(range(nb - 1, -1, -1))):
        sub = smp.loo_blocks(blocks=[blocks[k] for k in ks], first_slot=first, n_slots=S, trace=True)
        rows = _rows_of(off, ks)
        for k in LOO_ARRAYS + ("loglik_trace",):
            assert sub[k].tobytes() == np.ascontiguousarray(one[k][ks]).tobytes(), k
        for k in ROW_KEYS + ROW_TRACES + ("obs",):
            assert sub[k].tobytes() == np.ascontiguousarray(one[k][rows]).tobytes(), k
    # another slot range, hence another grid and other staging batches
    other = smp.loo_blocks(blocks=blocks, first_slot=first + 3, n_slots=10, trace=True)
    for k in TRACES:
        assert other[k].tobytes() == np.ascontiguousarray(one[k][:, :, 3:13]).tobytes(), k
    # the timers of the call
    ms, cnt = C.c_double(0), C.c_int64(0)
    for name in (b"loo_blocks", b"loo_blocks_psis"):
        assert smp.lib.bfmmm_get_timing(smp.h, name, C.byref(ms), C.byref(cnt)) == 0
        assert ms.value > 0 and cnt.value >= 1, name


def test_label_and_sign_invariance():
    import bayesfmmm_amd as bf
    from simdata import simulate_functional
    from test_gpu_chain_batch import _states, make_sampler_batch
    S = bf.sampler
    sim = simulate_functional(n=20, M=2, sigma_sq=0.01, seed=36, ragged=True)
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
    np.testing.assert_array_equal(b.get_chain("nu")[:, :, 0], a.get_chain("nu")[perm, :, 0])
    assert not np.array_equal(b.get_chain("nu")[:, :, 0], a.get_chain("nu")[:, :, 0])
    ra, rb = a.loo_blocks(block_size=4, first_slot=0, n_slots=1, trace=True), b.loo_blocks(block_size=4, first_slot=0, n_slots=1, trace=True)
    e = R.rel_diff(rb["loglik_trace"], ra["loglik_trace"])
    print(f"label permutation: worst relative difference of l {e.max():.3e}")
    assert e.max() <= R.GPU_TOL_L
    assert R.rel_diff(rb["mean_trace"], ra["mean_trace"]).max() <= R.GPU_TOL_M
    # against the dense form too, so that agreement is not two wrong answers
    l, pit, m, v, z = R.dense_traces(sim["y"], a.get_basis(), _chains(a), 0, 1, ra["block_curve"], ra["offsets"], ra["obs"])
    assert R.rel_diff(ra["loglik_trace"], l).max() <= R.GPU_TOL_L
    # the sign of one (Phi_.m, chi_.m) pair
    fst = dict(pst)
    fst["Phi"] = np.array(pst["Phi"], copy=True)
    fst["Phi"][:, :, 1] *= -1.0
    fst["chi"] = np.array(pst["chi"], copy=True)
    fst["chi"][:, 1] *= -1.0
    b.set_state(**fst)
    b.run(S.U_LOGLIK, 1, first_iter=1, seed=1)
    np.testing.assert_array_equal(b.get_chain("Phi")[:, :, 1, 1], -b.get_chain("Phi")[:, :, 1, 0])
    rf = b.loo_blocks(block_size=4, first_slot=1, n_slots=1, trace=True)
    e = R.rel_diff(rf["loglik_trace"], rb["loglik_trace"])
    print(f"eigen-sign flip: worst relative difference of l {e.max():.3e}")
    assert e.max() <= R.GPU_TOL_L
    assert R.rel_diff(rf["mean_trace"], rb["mean_trace"]).max() <= R.GPU_TOL_M
    a.close()
    b.close()


def test_argument_checks(batch):
    from bayesfmmm_amd import _lib
    smp, ys, lens = batch
    T = smp.T
    call = smp.loo_blocks
    with pytest.raises(_lib.BfmmmError, match="bfmmm_chain_loo_blocks: 'first_slot'"):
        call(block_size=5, first_slot=T)
    with pytest.raises(_lib.BfmmmError, match="'first_slot'"):
        call(block_size=5, first_slot=-1, n_slots=4)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        call(block_size=5, first_slot=2, n_slots=T - 1)
    with pytest.raises(_lib.BfmmmError, match="'n_slots'"):
        call(block_size=5, n_slots=0)
    with pytest.raises(_lib.BfmmmError, match="'max_workspace_bytes' must not be negative"):
        call(block_size=5, max_workspace_bytes=-1)
    with pytest.raises(_lib.BfmmmError, match=r"'max_workspace_bytes' below .*shared by all tiles \+ \d+ per tile"):
        call(block_size=5, max_workspace_bytes=64)
    c130 = _with_len(lens, 130)
    for kw, msg in (({}, "exactly one"), ({"block_size": 5, "horizon": 2}, "exactly one"), ({"blocks": [(0, [0])], "curves": [0]}, "'curves'"),
                    ({"blocks": [(c130, range(65))]}, "65 observations"), ({"blocks": [(c130, [])]}, "0 observations"),
                    ({"blocks": [(c130, [1, 1])]}, "repeats"), ({"blocks": [(c130, [130])]}, "an index outside"),
                    ({"blocks": [(smp.n, [0])]}, "curve"), ({"horizon": 20}, "not more than the horizon"),
                    ({"block_size": 3, "curves": [0, smp.n]}, "'curves'")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    smp.REFINE_TRACE_BYTES = 1000                          # on the instance: the class keeps its cap
    try:
        with pytest.raises(ValueError, match="REFINE_TRACE_BYTES"):
            call(block_size=5, trace=True)
    finally:
        del smp.REFINE_TRACE_BYTES
    # straight at the C entry
    lib = smp.lib
    i32, i64 = C.POINTER(C.c_int32), _lib.c_int64_p
    outs = [np.zeros(8) for _ in range(9)]
    p = [o.ctypes.data_as(_lib.c_double_p) for o in outs]

    def err(curve, offsets, obs, nb=None, ptrs=p, h=smp.h, caps=(8, 8), slots=(0, 4), nulls=()):
        bc, bo, bx = np.array(curve, dtype=np.int32), np.array(offsets, dtype=np.int64), np.array(obs, dtype=np.int32)
        lists = [bc.ctypes.data_as(i32), bo.ctypes.data_as(i64), bx.ctypes.data_as(i32)]
        for j in nulls:
            lists[j] = None
        rc = lib.bfmmm_chain_loo_blocks(h, *lists, len(bc) if nb is None else nb, slots[0], slots[1], 0, *ptrs, None, None, None, None, *caps)
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    good = ([c130, c130], [0, 2, 3], [4, 5, 9])
    assert lib.bfmmm_chain_loo_blocks(smp.h, np.array(good[0], dtype=np.int32).ctypes.data_as(i32), np.array(good[1], dtype=np.int64).ctypes.data_as(i64),
                                      np.array(good[2], dtype=np.int32).ctypes.data_as(i32), 2, 0, 4, 0, *p, None, None, None, None, 2, 3) == 0
    assert "bfmmm_chain_loo_blocks: 'h' is null" in err(*good, h=None)
    for j, nm in enumerate(("block_curve", "block_offsets", "block_obs")):
        assert f"'{nm}' is null" in err(*good, nulls=(j,))
    assert "'pit' is null" in err(*good, ptrs=p[:6] + [None] + p[7:])
    assert "'lppd' is null" in err(*good, ptrs=[None] + p[1:])
    assert "'n_blocks' must be at least 1" in err(*good, nb=0)
    assert "'block_offsets'[0] must be 0" in err(good[0], [1, 2, 3], good[2])
    assert "block 1 is empty" in err(good[0], [0, 2, 2], good[2])
    assert "block 1 is empty" in err(good[0], [0, 2, 1], good[2])
    assert "block 0 has 65 observations, above 64" in err([c130], [0, 65], list(range(65)), caps=(8, 80))
    assert f"'block_curve'[1] = {smp.n} outside 0 .. {smp.n - 1}" in err([c130, smp.n], good[1], good[2])
    assert "'block_curve'[0] = -1" in err([-1, c130], good[1], good[2])
    assert "'block_obs'[2] = 130 outside 0 .. 129" in err(good[0], good[1], [4, 5, 130])
    assert "'block_obs'[0] = -1 outside" in err(good[0], good[1], [-1, 5, 9])
    assert "'block_obs'[1] = 4 is repeated in block 0" in err(good[0], good[1], [4, 4, 9])
    assert "'block_capacity' below 2" in err(*good, caps=(1, 8))
    assert "'row_capacity' below 3" in err(*good, caps=(8, 2))
    assert "'first_slot' out of range" in err(*good, slots=(T, 1))
    assert "'n_slots' out of range" in err(*good, slots=(0, T + 1))
    # the same observation in two blocks is no repeat
    assert lib.bfmmm_chain_loo_blocks(smp.h, np.array(good[0], dtype=np.int32).ctypes.data_as(i32), np.array(good[1], dtype=np.int64).ctypes.data_as(i64),
                                      np.array([4, 5, 4], dtype=np.int32).ctypes.data_as(i32), 2, 0, 4, 0, *p, None, None, None, None, 2, 3) == 0
