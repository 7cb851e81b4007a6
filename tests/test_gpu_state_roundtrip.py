"""bfmmm_set_state / bfmmm_get_state: every name set_state accepts comes back byte for byte on either chain of a batch, nu and
Phi land in theta where DESIGN.md says (theta[(k (M + 1) + m') P + p], m' = 0: nu, m' = m + 1: Phi), and wrong counts, short
buffers, unknown names and null arguments give their messages."""
import numpy as np
import pytest

from tiny_sampler import K, M, N, NCH, P, make_tiny

pytestmark = pytest.mark.gpu

BASE = ["nu", "Phi", "chi", "Z", "pi", "alpha_3", "delta", "A", "gamma", "tau", "sigma_sq"]
COV = ["eta", "xi", "tau_eta", "gamma_xi", "delta_xi", "A_xi"]


def _shapes(D):
    """the reference's shapes (column-major)"""
    return {"nu": (K, P), "Phi": (K, P, M), "chi": (N, M), "Z": (N, K), "pi": (K,), "alpha_3": (1,), "delta": (K, M), "A": (K, 2),
            "gamma": (K, P, M), "tau": (K,), "sigma_sq": (1,), "eta": (P, D, K), "xi": (P, D, M, K), "tau_eta": (K, D),
            "gamma_xi": (P, D, M, K), "delta_xi": (K, M, D), "A_xi": (K, 2, D)}


def _values(names, shapes, q):
    """distinct values everywhere: a transposed index, another array or another chain cannot give the same bytes"""
    return {nm: (np.arange(int(np.prod(shapes[nm])), dtype=np.float64) + 0.5 + 1000.0 * j + 100000.0 * q).reshape(shapes[nm], order="F")
            for j, nm in enumerate(names)}


@pytest.mark.parametrize("D,covariance_adj", [(0, False), (2, False), (2, True)])
def test_every_name_round_trips_on_both_chains(D, covariance_adj):
    smp = make_tiny(D=D, covariance_adj=covariance_adj)
    names = BASE + (COV if D else [])
    shapes = _shapes(D)
    want = [_values(names, shapes, q) for q in range(NCH)]
    for q in range(NCH):
        smp.select_chain(q)
        for nm in names:
            smp.set_state(**{nm: want[q][nm]})
    for q in reversed(range(NCH)):
        smp.select_chain(q)
        for nm in names:
            got = smp.get_state(nm)
            assert got.shape == shapes[nm], (q, nm)
            assert got.tobytes(order="F") == want[q][nm].tobytes(order="F"), (q, nm)
        th = np.zeros((K, M + 1, P))
        th[:, 0, :] = want[q]["nu"]
        for m in range(M):
            th[:, m + 1, :] = want[q]["Phi"][:, :, m]
        assert smp.debug("theta", 64).tobytes() == th.tobytes(), q
    smp.close()


def test_messages():
    from bayesfmmm_amd import _lib
    smp = make_tiny()
    lib = smp.lib
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(_lib.c_double_p)

    def msg(rc):
        assert rc != 0
        return lib.bfmmm_last_error().decode()

    sizes = {nm: int(np.prod(s)) for nm, s in _shapes(0).items() if nm in BASE}
    for nm, cnt in sizes.items():
        for bad in (cnt - 1, cnt + 1):
            assert msg(lib.bfmmm_set_state(smp.h, nm.encode(), p, bad)) == f"bfmmm_set_state({nm}): wrong element count"
        assert msg(lib.bfmmm_get_state(smp.h, nm.encode(), p, cnt - 1)) == f"bfmmm_get_state({nm}): buffer too small"
        assert lib.bfmmm_get_state(smp.h, nm.encode(), p, cnt + 1) == 0
    for nm, cnt in (("loglik", 1), ("status", 1), ("stamps", 64)):      # read-only
        assert msg(lib.bfmmm_get_state(smp.h, nm.encode(), p, cnt - 1)) == f"bfmmm_get_state({nm}): buffer too small"
        assert lib.bfmmm_get_state(smp.h, nm.encode(), p, cnt) == 0
        assert msg(lib.bfmmm_set_state(smp.h, nm.encode(), p, cnt)) == f"bfmmm_set_state: unknown name '{nm}'"
    for nm in ["nope"] + COV:      # the covariate arrays do not exist before bfmmm_set_covariates
        assert msg(lib.bfmmm_set_state(smp.h, nm.encode(), p, 1)) == f"bfmmm_set_state: unknown name '{nm}'"
        assert msg(lib.bfmmm_get_state(smp.h, nm.encode(), p, 4096)) == f"bfmmm_get_state: unknown name '{nm}'"
    for args in ((None, b"nu", p), (smp.h, None, p), (smp.h, b"nu", None)):
        assert msg(lib.bfmmm_set_state(*args, K * P)) == "bfmmm_set_state: null argument"
        assert msg(lib.bfmmm_get_state(*args, K * P)) == "bfmmm_get_state: null argument"
    smp.close()
    cov = make_tiny(D=2)
    for nm in COV:
        cnt = int(np.prod(_shapes(2)[nm]))
        assert msg(lib.bfmmm_set_state(cov.h, nm.encode(), p, cnt + 1)) == f"bfmmm_set_state({nm}): wrong element count"
        assert msg(lib.bfmmm_get_state(cov.h, nm.encode(), p, cnt - 1)) == f"bfmmm_get_state({nm}): buffer too small"
    cov.close()
