"""CPU-side checks of the marginal PSIS-LOO over curves: the built library exports bfmmm_chain_loo_marginal with the
prototype the ctypes table declares, include/bfmmm.h declares it with its parameter names and documents its timers, the checks that
need no device refuse by name and Sampler has loo_marginal with the documented defaults (no compute calls)."""
import ctypes as C
import inspect
import os
import re

NAME = "bfmmm_chain_loo_marginal"
PARAMS = ["h", "first_slot", "n_slots", "n_samples", "n_stages", "seed", "refine", "ess_floor", "refine_samples", "refine_stages",
          "max_workspace_bytes", "lppd", "elpd_loo", "p_loo", "pareto_k", "elpd_waic", "p_waic", "ess_mean", "ess_min", "n_refined",
          "n_below", "lpd_trace", "ess_trace", "ess_trace_first", "refined_index", "refine_prop", "refine_samples_out", "n_ref",
          "capacity", "ref_capacity"]


def _args():
    from bayesfmmm_amd import _lib
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    return [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int64] + [dp] * 8 + \
        [ip, ip, dp, dp, dp, ip, dp, dp, _lib.c_int64_p, C.c_int64, C.c_int64]


def test_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and argtypes == _args() and len(argtypes) == len(PARAMS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", hdr)
    assert decl, "include/bfmmm.h does not declare " + NAME
    params = [p.strip() for p in decl.group(1).split(",")]
    assert [re.split(r"[ *]", p)[-1] for p in params] == PARAMS
    assert '"loo_marginal"' in hdr and '"loo_marginal_psis"' in hdr


def test_null_pointers_are_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    args = [None, 0, 1, 1, 1, 1, 1, 10.0, 4, 2, 0] + [None] * 17 + [0, 0]
    assert len(args) == len(PARAMS)
    assert lib.bfmmm_chain_loo_marginal(*args) != 0
    assert "bfmmm_chain_loo_marginal: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_the_method():
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.loo_marginal)
    assert list(sig.parameters)[1:] == ["first_slot", "n_slots", "n_samples", "n_stages", "seed", "refine", "ess_floor", "refine_samples",
                                        "refine_stages", "trace", "max_workspace_bytes"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["first_slot"], d["n_slots"], d["n_samples"], d["n_stages"], d["seed"]) == (0, None, 256, 3, 1)
    assert (d["refine"], d["ess_floor"], d["refine_samples"], d["refine_stages"], d["trace"], d["max_workspace_bytes"]) == \
        (True, 10.0, None, 2, False, 0)
