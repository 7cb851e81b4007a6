"""The pair-Gram contraction, entry by entry, on every route the run driver can take (pg_route in bfmmm_capi.hip,
pg_route_decide and launch_pair_gram in kernels_pair_gram.hip):

  1 general     k_pair_gram<false,false>, general body + k_pg_reduce      one chain, outside pg_solo_fits or solo switched off
  2 solo        the same kernel, pg_solo_g in the G workgroups            one chain inside pg_solo_fits
  3 batch       k_pair_gram<true,false>                                   2-3 chains with RT >= 8, or covariates
  4 grouped     k_pair_gram<true,true>                                    2-3 chains, RT < 8
  5 packed      k_pair_gram_pack + k_pg_reduce_pack                       >= 4 chains, or n > 16384
  6 multivariate (one column tile, the reduction spreads the sum over P columns)
  7 covariates  (the s part against s~_i = s_i - G_i o_i, per chain)

Every case pushes a generic state per chain, runs ONE iteration with a mask that runs the contraction and leaves Z and chi
alone, asserts through bfmmm_debug_get("pg_route") that the run took the route, slice length and slice count the case was
written for, and compares H and tvec of EVERY chain with the longdouble restatement of pair_gram_ref.py under its derived
bound |x - x_ref| <= (n + 8) 2^-53 S_abs per entry (entries without terms exactly 0.0).  The band copy H2 that k_factor and
the sweep read is checked bit for bit against H (both reduction kernels write it).  Routes documented to sum in the same
order are additionally compared bit for bit on H and tvec themselves."""
import numpy as np
import pytest

import pair_gram_ref as R

pytestmark = pytest.mark.gpu

BW = 3          # cubic splines
GENERAL, SOLO, BATCH, GROUPED, PACKED = 0, 1, 2, 3, -1
BODY_NAME = {GENERAL: "general", SOLO: "solo", BATCH: "batch", GROUPED: "grouped batch", PACKED: "packed"}


class Case:
    def __init__(self, name, n, K, M, P, route, KS, NKS, nch=1, G=None, md1=False, mv=False, D=0, solo=True):
        self.name, self.n, self.K, self.M, self.P, self.nch = name, n, K, M, P, nch
        self.route, self.KS, self.NKS = route, KS, NKS
        self.G = G if G is not None else (0 if route == PACKED else 1)
        self.md1, self.mv, self.D, self.solo = md1, mv, D, solo
        self.MD = 1 if md1 else M + 1


# (the slice geometry written next to a case is what the case was designed for; the device's own report must agree)
CASES = [
    # ---- route 2: one chain, single-chain body -- curve counts around a 16-curve chunk, every slice count of the reduction
    Case("solo_n5", 5, 2, 1, 30, SOLO, 16, 1),
    Case("solo_n16", 16, 2, 1, 30, SOLO, 16, 1),
    Case("solo_n17_oddP31", 17, 3, 6, 31, SOLO, 32, 1),                 # LG = 124: partial last column tile / 32-column pair
    Case("solo_n70", 70, 3, 3, 8, SOLO, 32, 3),
    Case("solo_nks4", 64, 3, 3, 8, SOLO, 16, 4),
    Case("solo_nks5", 80, 3, 3, 8, SOLO, 16, 5),
    Case("solo_nks7", 112, 3, 3, 8, SOLO, 16, 7),
    Case("solo_nks8", 128, 3, 3, 8, SOLO, 16, 8),
    Case("solo_nks32", 512, 3, 2, 20, SOLO, 16, 32),
    Case("solo_nks33", 528, 3, 2, 20, SOLO, 16, 33),
    Case("solo_nks36", 576, 3, 2, 20, SOLO, 16, 36),
    Case("solo_slice_multiple", 4224, 3, 6, 30, SOLO, 176, 24),
    Case("solo_slice_plus1", 4225, 3, 6, 30, SOLO, 176, 25),
    Case("solo_4133_rt29", 4096 + 37, 4, 8, 32, SOLO, 128, 33),         # K = 4, M = 8, P = 32: every solo limit at once, RT = 29
    Case("solo_r18_P32", 90, 3, 1, 32, SOLO, 32, 3),                    # R = 18: two rows beyond a row tile
    Case("solo_md1", 1000, 3, 6, 30, SOLO, 48, 21, md1=True),
    Case("solo_slice256", 6400, 2, 1, 30, SOLO, 256, 25),               # the solo limit from inside
    # ---- route 1: one chain, general body
    Case("general_slice272", 6401, 2, 1, 30, GENERAL, 272, 24),         # ... and from outside
    Case("general_K8_M16", 40, 8, 16, 12, GENERAL, 32, 2),              # RT = 345
    Case("general_K5_M8_P33", 64, 5, 8, 33, GENERAL, 16, 4),
    Case("general_P64", 200, 2, 6, 64, GENERAL, 32, 7),
    Case("general_M16_rt58", 300, 3, 16, 30, GENERAL, 32, 10),          # RT > 32
    Case("general_R784", 100, 7, 6, 8, GENERAL, 32, 4),                 # R = 16 * 49: no padding rows
    Case("general_R225", 100, 5, 4, 9, GENERAL, 32, 4),                 # R = 16 * 14 + 1: one row in the last tile, odd P
    Case("general_solo_off_n70", 70, 3, 3, 8, GENERAL, 32, 3, solo=False),
    Case("general_solo_off_4133", 4096 + 37, 3, 6, 30, GENERAL, 176, 24, solo=False),
    # ---- route 3: 2-3 chains, RT >= 8
    Case("batch2", 1000, 3, 6, 30, BATCH, 48, 21, nch=2),
    Case("batch3_oddP31", 4096 + 37, 3, 6, 31, BATCH, 176, 24, nch=3),
    # ---- route 4: 2-3 chains, RT < 8
    Case("grouped3_md1", 1000, 3, 6, 30, GROUPED, 48, 21, nch=3, G=3, md1=True),
    Case("grouped2_M1", 1000, 2, 1, 30, GROUPED, 48, 21, nch=2, G=2),
    Case("grouped2_n17", 17, 2, 1, 30, GROUPED, 32, 1, nch=2, G=2),
    # ---- route 5: >= 4 chains at the plain geometry; long curve sets (one chain, four chains)
    Case("packed4", 1000, 3, 6, 30, PACKED, 48, 21, nch=4),
    Case("packed4_oddP31", 1000, 3, 6, 31, PACKED, 48, 21, nch=4),
    Case("packed5_n70", 70, 3, 3, 8, PACKED, 32, 3, nch=5),             # sub-batches of 3 and 2 chains
    Case("packed8_md1", 1000, 3, 6, 30, PACKED, 48, 21, nch=8, md1=True),
    Case("packed4_nks4", 64, 3, 3, 8, PACKED, 16, 4, nch=4),
    Case("packed4_nks5", 80, 3, 3, 8, PACKED, 16, 5, nch=4),
    Case("packed4_nks7", 112, 3, 3, 8, PACKED, 16, 7, nch=4),
    Case("packed4_nks8", 128, 3, 3, 8, PACKED, 16, 8, nch=4),
    Case("packed4_nks32", 512, 3, 2, 20, PACKED, 16, 32, nch=4),
    Case("packed4_nks33", 528, 3, 2, 20, PACKED, 16, 33, nch=4),
    Case("packed4_nks36", 576, 3, 2, 20, PACKED, 16, 36, nch=4),
    Case("packed4_n5", 5, 2, 1, 30, PACKED, 16, 1, nch=4),
    Case("packed4_rt29", 300, 4, 8, 32, PACKED, 32, 10, nch=4),
    Case("packed_long1", 20000, 3, 6, 30, PACKED, 160, 125),
    Case("packed_long1_tail", 16384 + 37, 2, 1, 8, PACKED, 144, 115),
    Case("packed_long4", 20000, 2, 1, 32, PACKED, 160, 125, nch=4),
    # ---- route 6: multivariate
    Case("mv_n70", 70, 3, 2, 11, GENERAL, 32, 3, mv=True),
    Case("mv_n1000_P40", 1000, 4, 3, 40, GENERAL, 32, 32, mv=True),
    Case("mv_batch2", 300, 3, 2, 11, GROUPED, 32, 10, nch=2, G=2, mv=True),
    # ---- route 7: covariates (one chain: general body; chains: route 3, one chain per group)
    Case("cov_n70", 70, 3, 2, 10, GENERAL, 32, 3, D=2),
    Case("cov_n1000", 1000, 3, 6, 30, GENERAL, 48, 21, D=3),
    Case("cov_batch2_small_rt", 300, 2, 1, 9, BATCH, 32, 10, nch=2, D=2),
    Case("cov_batch3", 1000, 3, 6, 30, BATCH, 48, 21, nch=3, D=2),
]
BY_NAME = {c.name: c for c in CASES}

_data = {}


def functional_data(n, P, seed=1):
    """ragged curves on random grids (every G_i different), 5 - 11 observations each: small to build at any n"""
    key = (n, P, seed)
    if key not in _data:
        rng = np.random.default_rng(1000 * seed + P)
        ni = rng.integers(5, 12, size=n)
        off = np.concatenate([[0], np.cumsum(ni)])
        cid = np.repeat(np.arange(n), ni)
        t = rng.uniform(0.0, 1.0, size=off[-1])
        t = t[np.lexsort((t, cid))]
        y = rng.standard_normal(off[-1]) * 2.0
        _data.clear()         # (one set at a time: the long sets are the big ones)
        _data[key] = ([y[off[i]:off[i + 1]] for i in range(n)], [t[off[i]:off[i + 1]] for i in range(n)],
                      np.linspace(0.0, 1.0, P - BW - 1 + 2)[1:-1], np.array([0.0, 1.0]))
    return _data[key]


def chain_state(c, q):
    """a generic state of chain q: Z on the simplex but not uniform, chi of mixed sign and scale, different per chain"""
    rng = np.random.default_rng(7919 * (q + 1) + c.n)
    n, K, M, P = c.n, c.K, c.M, c.P
    Z = rng.dirichlet(np.full(K, 0.6 + 0.5 * q), size=n)
    Z = np.clip(Z, 1e-9, None)
    Z /= Z.sum(axis=1, keepdims=True)
    chi = rng.standard_normal((n, M)) * rng.choice([0.03, 1.0, 6.0], size=(n, 1))
    st = dict(nu=rng.standard_normal((K, P)), Phi=0.3 * rng.standard_normal((K, P, M)), chi=chi, Z=Z,
              pi=rng.dirichlet(np.full(K, 5.0)), alpha_3=np.array([3.5]), delta=rng.gamma(2.0, 1.0, size=(K, M)),
              A=rng.gamma(2.0, 1.0, size=(K, 2)), gamma=rng.gamma(2.0, 0.7, size=(K, P, M)), tau=rng.gamma(3.0, 0.5, size=K),
              sigma_sq=np.array([0.05]))
    if c.D:
        D = c.D
        st.update(eta=rng.standard_normal((P, D, K)), xi=0.4 * rng.standard_normal((P, D, M, K)),
                  tau_eta=rng.gamma(3.0, 0.5, size=(K, D)), gamma_xi=rng.gamma(2.0, 0.7, size=(P, D, M, K)),
                  delta_xi=rng.gamma(2.0, 1.0, size=(K, M, D)), A_xi=rng.gamma(2.0, 1.0, size=(K, 2, D)))
    return st


def make_sampler(c, nch):
    import bayesfmmm_amd as bf
    if c.mv:
        Y = np.random.default_rng(c.n + c.P).standard_normal((c.n, c.P)) * 2.0
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=c.K, n_eigen=c.M, tot_mcmc_iters=2)
        smp = bf.Sampler(cfg, Y, n_chains=nch)
    else:
        y, t, ik, bk = functional_data(c.n, c.P)
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=BW, tot_mcmc_iters=2)
        smp = bf.Sampler(cfg, y, t, ik, bk, n_chains=nch)
    X = None
    if c.D:
        X = np.random.default_rng(c.n + 17).standard_normal((c.n, c.D))
        smp.set_covariates(X, True)
    return smp, X


def expected_h2(H, P, bw, mv):
    """the piece-major band copy (h2_index, sweep_helpers.hpp) that belongs to H: entry k of row p is G(p, p + k - BW)"""
    Rr = H.shape[0]
    W = 2 * bw + 2
    idx = lambda p, k: (((k >> 1) * P + p) << 1) + (k & 1)
    out = np.zeros((Rr, P * W))
    for d in range(bw + 1):
        for p in range(P):
            out[:, idx(p, bw + d)] = H[:, d * P + p]
            if d > 0 and p + d < P:
                out[:, idx(p + d, bw - d)] = H[:, d * P + p]
    return out


def run_case(c, chains=None, solo=None):
    """one iteration of the contraction for case c; returns per chain (H, tvec) after checking route, entries and H2.
    chains: the chain indices (of the case's batch) to run -- a subset runs those chains' states as a batch of its own."""
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    chains = list(range(c.nch)) if chains is None else chains
    solo = c.solo if solo is None else solo
    lib.bfmmm_set_solo_pair_gram(1 if solo else 0)
    try:
        smp, X = make_sampler(c, len(chains))
        states = [chain_state(c, q) for q in chains]
        for k, st in enumerate(states):
            smp.select_chain(k)
            smp.set_state(**st)
        smp.run(bf.sampler.U_SIGMA, 1, seed=3, phi_chi_zero=c.md1)      # pair-Gram + reduce; Z and chi stay
    finally:
        lib.bfmmm_set_solo_pair_gram(1)
    route = smp.debug("pg_route", 8)
    d = smp.dims()
    assert (d["n"], d["K"], d["P"], d["MD"]) == (c.n, c.K, c.P, c.MD)
    bw = d["BW"]
    LG, P, Rr, A = d["LG"], c.P, d["R"], d["A"]
    rec = smp.debug("rec", c.n * d["LREC"] + 8).reshape(c.n, d["LREC"])
    Gc, s = R.split_records(rec, LG, P)
    out = []
    for k, st in enumerate(states):
        smp.select_chain(k)
        H = smp.debug("H", Rr * LG + 8).reshape(Rr, LG)
        tv = smp.debug("tvec", A * P + 8).reshape(A, P)
        H2 = smp.debug("H2", Rr * P * (2 * bw + 2) + 8).reshape(Rr, P * (2 * bw + 2))
        # the state the contraction read is the state that was pushed
        assert np.array_equal(smp.get_state("Z"), st["Z"]) and np.array_equal(smp.get_state("chi"), st["chi"])
        extra = 0
        if c.D:
            o, oa = R.cov_offset(st["Z"], st["chi"], X, st["eta"], st["xi"], c.MD)
            stl, sabs = R.stil_ref(Gc, s, o, oa, P, bw)
            ref = R.pair_gram_ref(Gc, stl, st["Z"], st["chi"], c.MD, s_abs=sabs)
            extra = c.K * c.D * c.MD + 2 * bw + 8
        else:
            ref = R.pair_gram_ref(Gc, s, st["Z"], st["chi"], c.MD, mv=c.mv)
        label = BODY_NAME[int(route[3])] + (" multivariate" if c.mv else "") + (" covariates" if c.D else "")
        where = f"{label} [{c.name}, chain {chains[k]} in a batch of {len(chains)}, KS {int(route[1])}, NKS {int(route[2])}]"
        r = R.assert_pair_gram(where, H, tv, ref, extra_t=extra)
        print(f"{where}: worst error / bound = {r:.3g}")
        assert np.array_equal(H2, expected_h2(H, P, bw, c.mv)), f"{where}: H2 is not the band copy of H"
        out.append((H, tv))
    smp.close()
    return route, out


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_entries_on_route(name):
    c = BY_NAME[name]
    route, _ = run_case(c)
    got = dict(packed=int(route[0]), KS=int(route[1]), NKS=int(route[2]), body=int(route[3]), G=int(route[4]))
    want = dict(packed=int(c.route == PACKED), KS=c.KS, NKS=c.NKS, body=c.route, G=c.G)
    assert got == want, f"{name}: the run did not take the route the case was written for"


def test_case_list_reaches_every_route_and_slice_count():
    # (each case asserts its own row against the device's report: this is the list's coverage)
    fun = [c for c in CASES if not c.mv and not c.D]
    assert {c.route for c in fun} == {GENERAL, SOLO, BATCH, GROUPED, PACKED}
    assert any(c.mv for c in CASES) and any(c.D and c.nch == 1 for c in CASES) and any(c.D and c.nch > 1 for c in CASES)
    assert any(c.route == PACKED and c.nch >= 4 and c.n <= 16384 for c in CASES)
    assert any(c.route == PACKED and c.nch == 1 and c.n > 16384 for c in CASES)
    assert any(c.route == PACKED and c.nch == 4 and c.n > 16384 for c in CASES)
    for red in (lambda c: c.route != PACKED, lambda c: c.route == PACKED):        # k_pg_reduce, k_pg_reduce_pack
        assert {1, 3, 4, 5, 7, 8, 32, 33, 36} <= {c.NKS for c in CASES if red(c)}
    assert {16, 256} <= {c.KS for c in CASES if c.route == SOLO} and any(c.KS == 272 and c.route == GENERAL for c in CASES)


@pytest.mark.parametrize("name", ["solo_n5", "solo_n17_oddP31", "solo_n70", "solo_nks33", "solo_slice_plus1", "solo_4133_rt29",
                                  "solo_md1", "solo_slice256"])
def test_solo_body_equals_general_body_on_H_and_t(name):
    # the same canonical order (slice, k-step, pair-weight product): bit-equal arrays, each ALSO checked against the reference
    c = BY_NAME[name]
    r1, a = run_case(c, solo=True)
    r0, b = run_case(c, solo=False)
    assert int(r1[3]) == SOLO and int(r0[3]) == GENERAL and tuple(r1[1:3]) == tuple(r0[1:3])
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1])


@pytest.mark.parametrize("name", ["batch2", "grouped3_md1", "grouped2_n17", "packed4", "packed4_oddP31", "packed5_n70",
                                  "packed4_nks33", "packed4_rt29", "packed8_md1"])
def test_chain_alone_equals_chain_in_batch_on_H_and_t(name):
    # equal slice geometry (the plain geometry depends on the shape alone): a chain sums as it does alone
    c = BY_NAME[name]
    rb, batch = run_case(c)
    for q in sorted({0, c.nch // 2, c.nch - 1}):
        ra, alone = run_case(c, chains=[q])
        assert int(ra[0]) == 0 and tuple(ra[1:3]) == tuple(rb[1:3]), "slice geometry differs: not comparable"
        assert np.array_equal(alone[0][0], batch[q][0]), f"{name}: H of chain {q} differs from the chain alone"
        assert np.array_equal(alone[0][1], batch[q][1]), f"{name}: tvec of chain {q} differs from the chain alone"
