"""CPU-side checks of the fitted function of held-out curves: the built library exports bfmmm_chain_predict_fit with
the prototype the ctypes table declares, include/bfmmm.h declares it with its parameter names and documents its timer, a null handle
is refused by name and Sampler has predict_fit with the documented defaults (no compute calls)."""
import ctypes as C
import inspect
import os
import re

NAME = "bfmmm_chain_predict_fit"
PARAMS = ["h", "y", "t", "B", "offsets", "n_new", "X", "perm", "first_slot", "n_slots", "n_samples", "n_stages", "seed", "zs",
          "E", "G", "noise", "probs", "nq", "max_workspace_bytes", "lpd", "z_mean", "z_sd", "ess_mean", "ess_min", "fit_mean", "fit_sd",
          "fit_q", "lpd_trace", "z_trace", "ess_trace", "prop_trace", "samples", "mean_trace", "var_trace", "path_trace", "path_index",
          "path_u", "path_xi", "capacity"]


def _args():
    from bayesfmmm_amd import _lib
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    return [C.c_void_p, dp, dp, dp, _lib.c_int64_p, C.c_int, dp, ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, dp,
            dp, C.c_int, C.c_int, dp, C.c_int, C.c_int64] + [dp] * 16 + [ip, dp, dp, C.c_int64]


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
    assert '"predict_fit"' in hdr


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    args = [None, None, None, None, None, 1, None, None, 0, 1, 1, 1, 1, None, None, 1, 0, None, 0, 0] + [None] * 19 + [0]
    assert len(args) == len(PARAMS)
    assert lib.bfmmm_chain_predict_fit(*args) != 0
    assert "bfmmm_chain_predict_fit: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_the_method():
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.predict_fit)
    assert list(sig.parameters)[1:] == ["Y_new", "E", "time_new", "basis_new", "X_new", "perm", "probs", "noise", "n_samples", "n_stages",
                                        "seed", "trace", "z_samples", "first_slot", "n_slots", "max_workspace_bytes"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["time_new"], d["basis_new"], d["X_new"], d["perm"], d["z_samples"]) == (None, None, None, None, None)
    assert (d["probs"], d["noise"], d["n_samples"], d["n_stages"], d["seed"], d["trace"]) == ((0.025, 0.5, 0.975), False, 256, 3, 1, False)
    assert d["first_slot"] == 0 and d["n_slots"] is None and d["max_workspace_bytes"] == 0
