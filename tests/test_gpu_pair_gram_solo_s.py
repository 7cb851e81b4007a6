"""The tail of the single-chain pair-Gram launch: the s-part workgroup's own body (pg_solo_s) and the
deferred log-likelihood in an extra workgroup of its own, against the general s-part body and the log-likelihood in front of
pi / alpha_3 (bfmmm_set_solo_pair_gram_tail(0)).  Same data, start state and seed, one chain, three iterations: H, H2 and t of the
last contraction (bfmmm_debug_get) and every chain slot of loglik, pi, alpha_3, delta, A, gamma, tau BIT-identical -- both bodies
keep the canonical summation order (slice, k-step, the product Z_j chit_m of the same two raw weights), and the scalar jobs
only moved between workgroups of one launch, so no tolerance applies.

Shapes: the seven of test_gpu_pair_gram_solo.py; n = 2500 (112-curve slices, a partial last slice of 36 curves: a partial last
16-curve chunk in the new body); and the fallbacks, asserted through the last entry of "pg_route": n = 40 (two slices: the grid
has two extra workgroups, so the log-likelihood stays with pi / alpha_3) and n = 20 < KS = 32 (a single slice: neither the
deferred delta / A / gamma / tau job nor the log-likelihood has a workgroup to move to)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN_NAMES = ["loglik", "pi", "alpha_3", "delta", "A", "gamma", "tau"]
DEBUG_NAMES = ["H", "H2", "tvec"]
PG_SOLO_S, PG_SOLO_LL = 4, 8      # flags of the "tail" entry of pg_route (include/bfmmm.h)
T = 3


def _run(n, K, M, tail):
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import _lib
    from bench import make_config2
    lib = _lib.load()
    w = make_config2(n=n, n_i=100, K=K, M=M)
    lib.bfmmm_set_solo_pair_gram_tail(tail)
    try:
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=w["K"], n_eigen=w["M"], basis_degree=3, tot_mcmc_iters=T)
        smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"])
        smp.set_state(**w["state"])
        smp.run(bf.sampler.SWEEP_WARM, T, first_iter=0, seed=11)
        out = {nm: np.array(smp.get_chain(nm), copy=True) for nm in CHAIN_NAMES}
        out.update({nm: smp.debug(nm) for nm in DEBUG_NAMES})
        route = smp.debug("pg_route", 8)
        smp.close()
    finally:
        lib.bfmmm_set_solo_pair_gram_tail(1)
    return route, out


# (n, K, M, slices, tail flags the run must take with the switch on)
CASES = [(4096, 3, 6, 24, PG_SOLO_S | PG_SOLO_LL), (4096 + 37, 3, 6, 24, PG_SOLO_S | PG_SOLO_LL), (200, 3, 6, 7, PG_SOLO_S | PG_SOLO_LL),
         (1000, 2, 1, None, PG_SOLO_S | PG_SOLO_LL), (1000, 4, 8, None, PG_SOLO_S | PG_SOLO_LL), (200, 2, 8, None, PG_SOLO_S | PG_SOLO_LL),
         (4096 + 37, 4, 1, None, PG_SOLO_S | PG_SOLO_LL), (2500, 3, 6, 23, PG_SOLO_S | PG_SOLO_LL),
         (40, 3, 6, 2, PG_SOLO_S), (20, 3, 6, 1, PG_SOLO_S)]


@pytest.mark.parametrize("n,K,M,nks,tail", CASES)
def test_tail_bodies_equal_general_bodies_bitwise(n, K, M, nks, tail):
    r1, new = _run(n, K, M, 1)
    r0, old = _run(n, K, M, 0)
    print(f"n={n} K={K} M={M}: pg_route on {r1.tolist()} off {r0.tolist()}")
    # both runs: one chain, unpacked, the single-chain body of the G workgroups, the same slices
    assert len(r1) == 6 and len(r0) == 6
    assert r1[0] == 0 and r1[3] == 1 and list(r1[:5]) == list(r0[:5])
    if nks is not None:
        assert int(r1[2]) == nks
    if n == 20:
        assert n < int(r1[1])          # a single slice longer than the curve set
    if n == 2500:
        assert 0 < n % int(r1[1]) and (n % int(r1[1])) % 16 != 0      # partial last slice, partial last chunk
    assert int(r1[5]) == tail, "the run did not take the bodies (or the fallback) the case was written for"
    assert int(r0[5]) == 0
    for nm in DEBUG_NAMES + CHAIN_NAMES:
        assert new[nm].size > 0 and np.all(np.isfinite(new[nm])), nm
        assert new[nm].tobytes() == old[nm].tobytes(), f"n={n} K={K} M={M} {nm}: not bit-identical"
    # the chain moved (three iterations, not a copy of the start state), and the log-likelihood slots were all written
    assert not np.array_equal(new["tau"][..., 0], new["tau"][..., -1])
    assert np.all(new["loglik"] != 0.0)
