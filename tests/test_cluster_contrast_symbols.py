"""CPU-side checks of the contrast call: the built library exports bfmmm_chain_cluster_contrast_bands with the prototype
the ctypes table declares and the header's argument count, its timers are named in the header, it refuses a null handle by name, and
Sampler.cluster_contrast_bands has the documented signature (no compute calls)."""
import ctypes as C
import os
import re

import pytest

NAME = "bfmmm_chain_cluster_contrast_bands"


def _want():
    from bayesfmmm_amd import _lib
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    return [C.c_void_p, dp, dp, C.c_int, dp, dp, C.c_int, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int64, dp, dp, dp, ip, dp, dp, dp,
            ip, dp, dp, dp, dp, C.c_int64]


def test_library_exports_the_entry_point():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    assert hasattr(lib, NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and argtypes == _want()
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", hdr)
    assert decl and len(decl.group(1).split(",")) == len(_want())
    for nm in ("contrast_coef", "contrast_values", "contrast_norm"):
        assert '"' + nm + '"' in hdr, nm
    assert hdr.index('"contrast_coef"') > hdr.index('"rescale_project"')


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert lib.bfmmm_chain_cluster_contrast_bands(None, None, None, 1, None, None, 1, None, 0, 1, None, 0, 0.05, 0, *([None] * 12), 0) != 0
    assert NAME + ": 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_the_method():
    import inspect
    from bayesfmmm_amd import sampler
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.cluster_contrast_bands)
    assert list(sig.parameters)[1:] == ["E", "contrasts", "perm", "rescale", "weights", "probs", "simultaneous", "trace", "first_slot", "n_slots",
                                        "max_workspace_bytes"]
    dflt = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert dflt == dict(contrasts="pairwise", perm=None, rescale=None, weights=None, probs=(0.025, 0.5, 0.975), simultaneous=None, trace=False,
                        first_slot=0, n_slots=None, max_workspace_bytes=0)
    assert callable(sampler.contrast_plan)
    # refused before any device call
    with pytest.raises(ValueError, match="exactly one of 'perm' and 'rescale'"):
        Sampler.cluster_contrast_bands(None, None)
    with pytest.raises(ValueError, match="exactly one of 'perm' and 'rescale'"):
        Sampler.cluster_contrast_bands(None, None, perm=[0], rescale={})
