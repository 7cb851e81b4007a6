"""CPU-side checks of the leave-block-out cross-validation: the built library exports bfmmm_chain_loo_blocks with the
prototype the ctypes table declares, the header declares it with its parameter names and documents the timers, the checks that
need no device refuse by name, and Sampler.loo_blocks and sampler.block_plan have the documented signatures (no compute calls)."""
import ctypes as C
import inspect
import os
import re

NAME = "bfmmm_chain_loo_blocks"
PARAMS = ["h", "block_curve", "block_offsets", "block_obs", "n_blocks", "first_slot", "n_slots", "max_workspace_bytes", "lppd", "elpd_loo",
          "p_loo", "pareto_k", "elpd_waic", "p_waic", "pit", "mean", "sd", "loglik_trace", "pit_trace", "mean_trace", "var_trace",
          "block_capacity", "row_capacity"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, name):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert decl, f"include/{header} does not declare {name}"
    return hdr, [re.split(r"[ *]", p.strip())[-1] for p in decl.group(1).split(",")]


def test_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    dp = _lib.c_double_p
    assert hasattr(lib, NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.POINTER(C.c_int32), _lib.c_int64_p, C.POINTER(C.c_int32), C.c_int64, C.c_int, C.c_int, C.c_int64] + \
        [dp] * 13 + [C.c_int64, C.c_int64]
    hdr, params = _declared("bfmmm.h", NAME)
    assert params == PARAMS and len(argtypes) == len(PARAMS)
    assert '"loo_blocks"' in hdr and '"loo_blocks_psis"' in hdr
    # the pointwise call keeps its prototype beside it
    assert _lib.SYMBOLS["bfmmm_chain_loo_pointwise"][1] == [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int64] + \
        [dp] * 13 + [C.c_int64]


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    args = [None, None, None, None, 1, 0, 1, 0] + [None] * 13 + [0, 0]
    assert len(args) == len(PARAMS)
    assert lib.bfmmm_chain_loo_blocks(*args) != 0
    assert "bfmmm_chain_loo_blocks: 'h' is null" in lib.bfmmm_last_error().decode()


def test_python_signatures():
    from bayesfmmm_amd import sampler
    sig = inspect.signature(sampler.Sampler.loo_blocks)
    assert list(sig.parameters)[1:] == ["blocks", "block_size", "horizon", "curves", "first_slot", "n_slots", "trace", "max_workspace_bytes"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert d == {"blocks": None, "block_size": None, "horizon": None, "curves": None, "first_slot": 0, "n_slots": None, "trace": False,
                 "max_workspace_bytes": 0}
    sig = inspect.signature(sampler.block_plan)
    assert list(sig.parameters) == ["ni", "blocks", "block_size", "horizon", "curves"]
    assert all(sig.parameters[k].default is None for k in list(sig.parameters)[1:])
    # loo_pointwise is unchanged
    sig = inspect.signature(sampler.Sampler.loo_pointwise)
    assert list(sig.parameters)[1:] == ["curves", "first_slot", "n_slots", "trace", "max_workspace_bytes"]
