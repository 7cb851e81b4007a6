"""CPU-side checks of the simultaneous bands of the pooled per-curve fits: the built library exports
bfmmm_chain_curve_bands_sim, the ctypes table carries it and Sampler has curve_bands_simultaneous (no compute calls)."""


def test_library_exports_curve_bands_sim():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "bfmmm_chain_curve_bands_sim")
    assert "bfmmm_chain_curve_bands_sim" in _lib.SYMBOLS
    restype, argtypes = _lib.SYMBOLS["bfmmm_chain_curve_bands_sim"]
    assert len(argtypes) == 16


def test_sampler_has_curve_bands_simultaneous():
    import inspect
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(Sampler.curve_bands_simultaneous)
    assert list(sig.parameters)[1:] == ["E", "which", "alpha", "curves", "first_slot", "n_slots", "max_workspace_bytes"]
    assert sig.parameters["which"].default == "fit" and sig.parameters["alpha"].default == 0.05
    # curve_bands keeps its signature
    assert list(inspect.signature(Sampler.curve_bands).parameters)[1:] == ["E", "which", "probs", "curves", "first_slot", "n_slots",
                                                                           "max_workspace_bytes"]
