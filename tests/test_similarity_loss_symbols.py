"""The least-squares draw of the clustering through every layer, without computing anything: the built library
exports bfmmm_chain_similarity_loss and bfmmm_get_slot, include/bfmmm.h declares them, _lib.SYMBOLS carries them with 9 and 5
arguments, and Sampler has similarity_loss, get_slot and representative_draw with the documented signatures."""
import inspect
import os
import re


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:]


def test_symbols_and_signatures():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    from bayesfmmm_amd.sampler import Sampler
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    declared = set(re.findall(r"\b(bfmmm_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name, nargs in (("bfmmm_chain_similarity_loss", 9), ("bfmmm_get_slot", 5)):
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), name
    for nm in ("similarity_loss", "similarity_loss_reduce"):
        assert f'"{nm}"' in hdr, nm
    E = inspect.Parameter.empty
    assert _sig(Sampler.similarity_loss) == [("first_slot", 0), ("n_slots", None), ("diagnostics", True), ("max_workspace_bytes", 0)]
    assert _sig(Sampler.get_slot) == [("name", E), ("slot", E), ("chain", None)]
    assert _sig(Sampler.representative_draw) == [("names", ("Z",)), ("first_slot", 0), ("n_slots", None), ("max_workspace_bytes", 0)]
