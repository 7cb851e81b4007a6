"""CPU-side checks of the cluster covariance surfaces: the built library exports bfmmm_chain_cluster_cov_bands
with the prototype the ctypes table declares, include/bfmmm.h declares it, a null handle is refused by name and Sampler has
cluster_cov_bands (no compute calls)."""
import ctypes as C
import os
import re

NAME = "bfmmm_chain_cluster_cov_bands"


def _args():
    from bayesfmmm_amd import _lib
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    # (h, perm, E1, G1, E2, G2, diagonal, pairs, n_pairs, x, first_slot, n_slots, probs, nq, alpha, max_workspace_bytes, mean, sd,
    #  quant, crit, lower, upper, trace, capacity)
    return [C.c_void_p, ip, dp, C.c_int, dp, C.c_int, C.c_int, ip, C.c_int, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int64,
            dp, dp, dp, dp, dp, dp, dp, C.c_int64]


def test_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and argtypes == _args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", hdr)
    assert decl, "include/bfmmm.h does not declare " + NAME
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(_args())
    names = [re.split(r"[ *]", p)[-1] for p in params]
    assert names == ["h", "perm", "E1", "G1", "E2", "G2", "diagonal", "pairs", "n_pairs", "x", "first_slot", "n_slots", "probs", "nq",
                     "alpha", "max_workspace_bytes", "mean", "sd", "quant", "crit", "lower", "upper", "trace", "capacity"]
    # the timers of the call are documented with bfmmm_get_timing
    for t in ("cluster_cov_project", "cluster_cov", "cluster_cov_maxdev"):
        assert '"' + t + '"' in hdr, t


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert lib.bfmmm_chain_cluster_cov_bands(None, None, None, 1, None, 0, 0, None, 0, None, 0, 1, None, 0, 0.05, 0, *([None] * 7), 0) != 0
    assert "bfmmm_chain_cluster_cov_bands: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_the_method():
    import inspect
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.cluster_cov_bands)
    assert list(sig.parameters)[1:] == ["E", "perm", "E2", "pairs", "x", "diagonal", "probs", "simultaneous", "trace", "first_slot",
                                        "n_slots", "max_workspace_bytes"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["E2"], d["pairs"], d["x"], d["diagonal"], d["simultaneous"], d["trace"]) == (None, None, None, False, None, False)
    assert d["probs"] == (0.025, 0.5, 0.975) and d["first_slot"] == 0 and d["n_slots"] is None and d["max_workspace_bytes"] == 0
