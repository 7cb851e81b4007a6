"""CPU-side checks of the label alignment: the built library exports bfmmm_chain_align,
bfmmm_chain_aligned_summary and bfmmm_chain_cluster_mean_bands with the prototypes the ctypes table declares, and Sampler has
align, aligned_summary and cluster_mean_bands (no compute calls)."""
import ctypes as C
import os
import re


def test_library_exports_the_alignment_entry_points():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    want = {
        "bfmmm_chain_align": [C.c_void_p, dp, C.c_int, C.c_int, ip, dp, C.c_int64],
        "bfmmm_chain_aligned_summary": [C.c_void_p, C.c_char_p, ip, C.c_int, C.c_int, dp, C.c_int, C.c_int64] + [dp] * 8 + [C.c_int64],
        "bfmmm_chain_cluster_mean_bands": [C.c_void_p, ip, dp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int64, dp, dp, dp, C.c_int64],
    }
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    for name, args in want.items():
        assert hasattr(lib, name), name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and argtypes == args, name
        # the header's declaration has as many parameters
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == len(args), name


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert lib.bfmmm_chain_align(None, None, 0, 1, None, None, 0) != 0
    assert "bfmmm_chain_align: 'h' is null" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_aligned_summary(None, b"Z", None, 0, 1, None, 0, 0, *([None] * 8), 0) != 0
    assert "bfmmm_chain_aligned_summary: 'h' is null" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_cluster_mean_bands(None, None, None, 1, 0, 1, None, 0, 0, None, None, None, 0) != 0
    assert "bfmmm_chain_cluster_mean_bands: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_the_alignment_methods():
    import inspect
    from bayesfmmm_amd.sampler import Sampler
    assert list(inspect.signature(Sampler.align).parameters)[1:] == ["pivot", "first_slot", "n_slots", "max_workspace_bytes"]
    assert list(inspect.signature(Sampler.aligned_summary).parameters)[1:] == ["name", "perm", "probs", "first_slot", "n_slots",
                                                                               "max_workspace_bytes"]
    assert list(inspect.signature(Sampler.cluster_mean_bands).parameters)[1:] == ["E", "perm", "probs", "first_slot", "n_slots",
                                                                                  "max_workspace_bytes"]
    assert inspect.signature(Sampler.aligned_summary).parameters["probs"].default == (0.025, 0.5, 0.975)
