"""CPU-side checks of the Laplace mixture proposal: the built library exports bfmmm_chain_predict_laplace and
bfmmm_chain_loo_marginal_laplace with the prototypes the ctypes table declares, include/bfmmm.h declares them with their parameter
names and documents their timers, the checks that need no device refuse by name, and Sampler.predict and Sampler.loo_marginal take
`proposal` with the default "dirichlet" (no compute calls)."""
import ctypes as C
import inspect
import os
import re

PREDICT = "bfmmm_chain_predict_laplace"
PREDICT_PARAMS = ["h", "y", "t", "B", "offsets", "n_new", "X", "perm", "first_slot", "n_slots", "n_samples", "seed", "max_workspace_bytes",
                  "lpd", "z_mean", "z_sd", "ess_mean", "ess_min", "lpd_trace", "z_trace", "ess_trace", "n_modes", "components",
                  "eta_samples", "capacity"]
LOO = "bfmmm_chain_loo_marginal_laplace"
LOO_PARAMS = ["h", "first_slot", "n_slots", "n_samples", "seed", "ess_floor", "max_workspace_bytes", "lppd", "elpd_loo", "p_loo", "pareto_k",
              "elpd_waic", "p_waic", "ess_mean", "ess_min", "n_below", "lpd_trace", "ess_trace", "n_modes", "components", "eta_samples",
              "capacity"]


def _args():
    from bayesfmmm_amd import _lib
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    pred = [C.c_void_p, dp, dp, dp, _lib.c_int64_p, C.c_int, dp, ip, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int64] + [dp] * 8 + \
        [ip, dp, dp, C.c_int64]
    loo = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_int64] + [dp] * 8 + [ip, dp, dp, ip, dp, dp, C.c_int64]
    return {PREDICT: pred, LOO: loo}


def test_library_exports_the_entry_points():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bfmmm.h")).read()
    for name, names in ((PREDICT, PREDICT_PARAMS), (LOO, LOO_PARAMS)):
        assert hasattr(lib, name)
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and argtypes == _args()[name] and len(argtypes) == len(names)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl, "include/bfmmm.h does not declare " + name
        assert [re.split(r"[ *]", p.strip())[-1] for p in decl.group(1).split(",")] == names
    assert '"predict_laplace"' in hdr and '"loo_marginal_laplace"' in hdr


def test_null_pointers_are_refused_by_name():
    """the argument checks run before any device is touched"""
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib
    lib = _lib.load()
    args = [None] * 5 + [1, None, None, 0, 1, 8, 1, 0] + [None] * 11 + [1]
    assert len(args) == len(PREDICT_PARAMS)
    assert lib.bfmmm_chain_predict_laplace(*args) != 0
    assert "bfmmm_chain_predict_laplace: 'h' is null" in lib.bfmmm_last_error().decode()
    args = [None, 0, 1, 8, 1, 10.0, 0] + [None] * 14 + [0]
    assert len(args) == len(LOO_PARAMS)
    assert lib.bfmmm_chain_loo_marginal_laplace(*args) != 0
    assert "bfmmm_chain_loo_marginal_laplace: 'h' is null" in lib.bfmmm_last_error().decode()


def test_sampler_takes_the_proposal():
    from bayesfmmm_amd.sampler import Sampler
    import pytest
    for fn in (Sampler.predict, Sampler.loo_marginal):
        # the option is keyword-only and sits in front of the method, whose own parameters and defaults stay what they were
        p = inspect.signature(fn, follow_wrapped=False).parameters["proposal"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "dirichlet"
        assert "proposal" not in inspect.signature(fn).parameters
    assert inspect.signature(Sampler.loo_marginal).parameters["refine"].default is True
    assert not hasattr(Sampler.predict_fit, "__wrapped__")

    class Fake:
        """stands in for a sampler: the option's checks run before anything touches the device"""
        predict, loo_marginal = Sampler.predict, Sampler.loo_marginal

        def _predict_laplace(self, **kw):
            return ("predict", kw)

        def _loo_marginal_laplace(self, **kw):
            return ("loo", kw)

    f = Fake()
    with pytest.raises(ValueError, match="predict: 'n_stages' has no meaning with proposal='laplace'"):
        f.predict([], n_stages=2, proposal="laplace")
    with pytest.raises(ValueError, match="predict: 'z_samples' has no meaning"):
        f.predict([], z_samples=[1.0], proposal="laplace")
    with pytest.raises(ValueError, match="loo_marginal: 'refine' has no meaning"):
        f.loo_marginal(refine=True, proposal="laplace")
    with pytest.raises(ValueError, match="loo_marginal: 'refine_samples' has no meaning"):
        f.loo_marginal(refine_samples=8, proposal="laplace")
    with pytest.raises(ValueError, match="proposal must be 'dirichlet' or 'laplace'"):
        f.loo_marginal(proposal="gauss")
    # the defaults given explicitly, and refine=False, pass; what has no meaning there is not handed on
    name, kw = f.predict([1], [2], n_samples=8, n_stages=3, proposal="laplace")
    assert name == "predict" and kw == dict(Y_new=[1], time_new=[2], basis_new=None, X_new=None, perm=None, n_samples=8, seed=1, trace=False,
                                            first_slot=0, n_slots=None, max_workspace_bytes=0)
    name, kw = f.loo_marginal(2, refine=False, ess_floor=5.0, proposal="laplace")
    assert name == "loo" and kw == dict(first_slot=2, n_slots=None, n_samples=256, seed=1, ess_floor=5.0, trace=False, max_workspace_bytes=0)
