"""CPU-side checks of the rescale step: the built library exports bfmmm_chain_rescale,
bfmmm_chain_rescaled_summary, bfmmm_chain_cluster_mean_bands_rescaled and bfmmm_chain_cluster_cov_bands_rescaled with the prototypes
the ctypes table declares, they refuse a null handle by name, Sampler has rescale, and aligned_summary, cluster_mean_bands and
cluster_cov_bands take the keyword-only rescale= (cluster_mean_bands also x=) while inspect.signature shows their own parameters (no
compute calls)."""
import ctypes as C
import os
import re

import pytest


def _want():
    from bayesfmmm_amd import _lib
    dp, ip, lp = _lib.c_double_p, C.POINTER(C.c_int32), _lib.c_int64_p
    return {
        "bfmmm_chain_rescale": [C.c_void_p, ip, dp, C.c_int, C.c_int, dp, dp, ip, dp, dp, lp, C.c_int64],
        "bfmmm_chain_rescaled_summary": [C.c_void_p, C.c_char_p, dp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_int64] + [dp] * 8 + [C.c_int64],
        "bfmmm_chain_cluster_mean_bands_rescaled": [C.c_void_p, dp, dp, C.c_int, dp, C.c_int, C.c_int, dp, C.c_int, C.c_int64, dp, dp, dp,
                                                    C.c_int64],
        "bfmmm_chain_cluster_cov_bands_rescaled": [C.c_void_p, dp, dp, C.c_int, dp, C.c_int, C.c_int, ip, C.c_int, dp, C.c_int, C.c_int, dp,
                                                   C.c_int, C.c_double, C.c_int64] + [dp] * 7 + [C.c_int64],
    }


def test_library_exports_the_rescale_entry_points():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    for name, args in _want().items():
        assert hasattr(lib, name), name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and argtypes == args, name
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl and len(decl.group(1).split(",")) == len(args), name
    # the covariance call differs from its sibling in the second argument alone
    assert _lib.SYMBOLS["bfmmm_chain_cluster_cov_bands_rescaled"][1][2:] == _lib.SYMBOLS["bfmmm_chain_cluster_cov_bands"][1][2:]
    for nm in ("rescale_transform", "rescale_gather", "rescale_project"):
        assert '"' + nm + '"' in hdr, nm


def test_null_handle_is_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert lib.bfmmm_chain_rescale(None, None, None, 0, 1, None, None, None, None, None, None, 0) != 0
    assert "bfmmm_chain_rescale: 'h' is null" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_rescaled_summary(None, b"Z", None, None, 0, 1, None, 0, 0, *([None] * 8), 0) != 0
    assert "bfmmm_chain_rescaled_summary: 'h' is null" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_cluster_mean_bands_rescaled(None, None, None, 1, None, 0, 1, None, 0, 0, None, None, None, 0) != 0
    assert "bfmmm_chain_cluster_mean_bands_rescaled: 'h' is null" in lib.bfmmm_last_error().decode()
    assert lib.bfmmm_chain_cluster_cov_bands_rescaled(None, None, None, 1, None, 0, 0, None, 0, None, 0, 1, None, 0, 0.05, 0, *([None] * 7), 0) != 0
    assert "bfmmm_chain_cluster_cov_bands_rescaled: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_has_rescale_and_the_keyword():
    import inspect
    from bayesfmmm_amd.sampler import Sampler
    par = lambda f: list(inspect.signature(f).parameters)[1:]
    assert par(Sampler.rescale) == ["perm", "transform", "first_slot", "n_slots"]
    # the keyword comes from a wrapper: the methods show their own parameters, and the wrapper takes rescale= (and x=)
    assert par(Sampler.aligned_summary) == ["name", "perm", "probs", "first_slot", "n_slots", "max_workspace_bytes"]
    assert par(Sampler.cluster_mean_bands) == ["E", "perm", "probs", "first_slot", "n_slots", "max_workspace_bytes"]
    for f in (Sampler.aligned_summary, Sampler.cluster_mean_bands, Sampler.cluster_cov_bands):
        kwonly = inspect.signature(f, follow_wrapped=False).parameters
        assert kwonly["rescale"].kind is inspect.Parameter.KEYWORD_ONLY and kwonly["rescale"].default is None, f.__name__
        assert "rescale=None" in f.__doc__, f.__name__
    for nm in ("rescaled_summary", "cluster_mean_bands_rescaled", "cluster_cov_bands_rescaled"):
        assert not hasattr(Sampler, nm), nm
    assert "x=None" in Sampler.cluster_mean_bands.__doc__ and "x = 0" in Sampler.cluster_mean_bands.__doc__
    assert "out of scope" in Sampler.cluster_eigen.__doc__
    # refused before any device call: x without rescale
    with pytest.raises(ValueError, match="'x' is honoured only with rescale="):
        Sampler.cluster_mean_bands(None, None, None, x=[0.0])
