"""CPU-side checks of the cluster eigenvalues and eigenfunctions: the built library exports
bfmmm_chain_cluster_eigen with the prototype the ctypes table declares, include/bfmmm.h declares it with its parameter names and
documents its three timers, a null handle is refused by name and Sampler has cluster_eigen (no compute calls)."""
import ctypes as C
import inspect
import os
import re

NAME = "bfmmm_chain_cluster_eigen"
PARAMS = ["h", "perm", "E", "G", "w", "x", "n_functions", "ref", "first_slot", "n_slots", "probs", "nq", "max_workspace_bytes",
          "val_diag", "val_quant", "pve_mean", "pve_sd", "pve_quant", "tot_mean", "tot_sd", "tot_quant", "fn_mean", "fn_sd", "fn_quant",
          "val_trace", "fn_trace", "max_sweeps", "capacity"]


def _args():
    from bayesfmmm_amd import _lib
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    return [C.c_void_p, ip, dp, C.c_int, dp, dp, C.c_int, dp, C.c_int, C.c_int, dp, C.c_int, C.c_int64] + [dp] * 13 + [ip, C.c_int64]


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
    # the switch between the two forms of S_k
    assert hasattr(lib, "bfmmm_set_cluster_eig_form") and _lib.SYMBOLS["bfmmm_set_cluster_eig_form"] == (None, [C.c_int])
    assert re.search(r"\bvoid bfmmm_set_cluster_eig_form\(int form\);", hdr)
    # the timers of the call are documented with bfmmm_get_timing
    for t in ("cluster_eig_gram", "cluster_eig", "cluster_eig_values"):
        assert '"' + t + '"' in hdr, t


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert lib.bfmmm_chain_cluster_eigen(None, None, None, 1, None, None, 0, None, 0, 1, None, 0, 0, *([None] * 13), None, 0) != 0
    assert "bfmmm_chain_cluster_eigen: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_the_method():
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.cluster_eigen)
    assert list(sig.parameters)[1:] == ["E", "perm", "weights", "n_functions", "x", "ref", "probs", "trace", "first_slot", "n_slots",
                                        "max_workspace_bytes"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["weights"], d["n_functions"], d["x"], d["ref"], d["trace"]) == (None, None, None, "mean", False)
    assert d["probs"] == (0.025, 0.5, 0.975) and d["first_slot"] == 0 and d["n_slots"] is None and d["max_workspace_bytes"] == 0
