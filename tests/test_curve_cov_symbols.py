"""CPU-side checks of the pooled per-curve covariance surfaces: the built library exports
bfmmm_chain_curve_cov, the ctypes table carries it and Sampler has curve_cov (no compute calls)."""


def test_library_exports_curve_cov():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "bfmmm_chain_curve_cov")
    assert "bfmmm_chain_curve_cov" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["bfmmm_chain_curve_cov"]
    assert len(argtypes) == 15


def test_sampler_has_curve_cov():
    import inspect
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.curve_cov)
    assert list(sig.parameters)[1:] == ["E", "E2", "curves", "sd", "per_chain", "diagonal", "first_slot", "n_slots", "max_workspace_bytes"]
