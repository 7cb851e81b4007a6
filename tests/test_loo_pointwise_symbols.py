"""CPU-side checks of the observation-level PSIS-LOO: the built library exports bfmmm_chain_loo_pointwise and
bfmmm_post_psis_expect with the prototypes the ctypes tables declare, the headers declare them with their parameter names and
document the timers, the checks that need no device refuse by name, and Sampler.loo_pointwise and api.psis_expect have the
documented signatures (no compute calls)."""
import ctypes as C
import inspect
import os
import re

NAME = "bfmmm_chain_loo_pointwise"
PARAMS = ["h", "curves", "n_curves", "first_slot", "n_slots", "max_workspace_bytes", "lppd", "elpd_loo", "p_loo", "pareto_k", "elpd_waic",
          "p_waic", "pit", "mean", "sd", "loglik_trace", "pit_trace", "mean_trace", "var_trace", "capacity"]
POST = "bfmmm_post_psis_expect"
POST_PARAMS = ["ll", "h", "n", "S", "n_aux", "device", "lppd", "elpd_loo", "p_loo", "pareto_k", "elpd_waic", "p_waic", "expect"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, name):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert decl, f"include/{header} does not declare {name}"
    return hdr, [re.split(r"[ *]", p.strip())[-1] for p in decl.group(1).split(",")]


def test_library_exports_the_entry_points():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib, api
    lib = _lib.load()
    dp = _lib.c_double_p
    assert hasattr(lib, NAME) and hasattr(lib, POST)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int64] + [dp] * 13 + [C.c_int64]
    hdr, params = _declared("bfmmm.h", NAME)
    assert params == PARAMS and len(argtypes) == len(PARAMS)
    assert '"loo_pointwise"' in hdr and '"loo_pointwise_psis"' in hdr
    restype, argtypes = api.POST_SYMBOLS[POST]
    assert restype is C.c_int
    assert argtypes == [api.c_double_p, api.c_double_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [api.c_double_p] * 7
    _, params = _declared("bfmmm_post.h", POST)
    assert params == POST_PARAMS and len(argtypes) == len(POST_PARAMS)


def test_null_pointers_are_refused_by_name():
    """the argument checks run before any device is touched"""
    import numpy as np
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib, api
    lib = _lib.load()
    args = [None, None, 0, 0, 1, 0] + [None] * 13 + [0]
    assert len(args) == len(PARAMS)
    assert lib.bfmmm_chain_loo_pointwise(*args) != 0
    assert "bfmmm_chain_loo_pointwise: 'h' is null" in lib.bfmmm_last_error().decode()
    post = api._lib_entry()
    z = np.zeros(4)
    p = z.ctypes.data_as(api.c_double_p)
    for missing, name in ((0, "ll"), (1, "h"), (9, "pareto_k"), (12, "expect")):
        a = [p, p, 2, 2, 1, 0] + [p] * 7
        a[missing] = None
        assert post.bfmmm_post_psis_expect(*a) != 0
        assert f"bfmmm_post_psis_expect: '{name}' is null" in post.bfmmm_entry_last_error().decode()
    assert post.bfmmm_post_psis_expect(p, p, 2, 2, 0, 0, *[p] * 7) != 0
    assert "bfmmm_post_psis_expect: bad dimensions" in post.bfmmm_entry_last_error().decode()


def test_python_signatures():
    from bayesfmmm_amd import api
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.loo_pointwise)
    assert list(sig.parameters)[1:] == ["curves", "first_slot", "n_slots", "trace", "max_workspace_bytes"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["curves"], d["first_slot"], d["n_slots"], d["trace"], d["max_workspace_bytes"]) == (None, 0, None, False, 0)
    sig = inspect.signature(api.psis_expect)
    assert list(sig.parameters) == ["ll", "h", "device"] and sig.parameters["device"].default == 0
    assert list(inspect.signature(api.psis_loo).parameters) == ["ll", "device"]
