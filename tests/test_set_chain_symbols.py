"""Loading chains into the chain slots and the slot log-likelihood through every layer, without computing
anything: the built library exports bfmmm_set_chain and bfmmm_chain_slot_loglik, include/bfmmm.h declares them, _lib.SYMBOLS
carries them with 6 and 8 arguments, Sampler has set_chain, load_chain and slot_loglik and api has read_batches and open_batches
with the documented signatures, and the header names the two timers."""
import inspect
import os
import re


def _sig(fn, skip=1):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind != p.VAR_KEYWORD][skip:]


def test_symbols_and_signatures():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib, api
    from bayesfmmm_amd.sampler import Sampler
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    declared = set(re.findall(r"\b(bfmmm_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name, nargs in (("bfmmm_set_chain", 6), ("bfmmm_chain_slot_loglik", 8)):
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), name
    for nm in ("slot_loglik", "slot_loglik_reduce"):
        assert f'"{nm}"' in hdr, nm
    E = inspect.Parameter.empty
    assert _sig(Sampler.set_chain) == [("name", E), ("values", E), ("first_slot", 0), ("chain", None)]
    assert _sig(Sampler.load_chain) == [("arrays", E), ("first_slot", 0), ("chain", None)]
    assert _sig(Sampler.slot_loglik) == [("first_slot", 0), ("n_slots", None), ("store", False), ("per_curve", False), ("max_workspace_bytes", 0)]
    assert _sig(Sampler.get_chain) == [("name", E), ("n_slots", None)]      # what set_chain mirrors
    assert _sig(api.read_batches, 0) == [("dir", E), ("n_files", E), ("X", False), ("cov_adj", False), ("drop_unassigned", False)]
    assert _sig(api.open_batches, 0) == [("dirs", E), ("n_files", E), ("Y", E), ("time", None), ("basis_degree", None), ("boundary_knots", None),
                                         ("internal_knots", None), ("X", None), ("cov_adj", False), ("drop_unassigned", False), ("device", 0)]
    assert any(p.kind == p.VAR_KEYWORD and p.name == "cfg_kw" for p in inspect.signature(api.open_batches).parameters.values())
