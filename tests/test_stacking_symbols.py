"""CPU-side checks of stacking and of the chain-by-chain PSIS-LOO: the built library exports bfmmm_post_stacking and
bfmmm_chain_loo_by_chain with the prototypes the ctypes tables declare, the headers declare them with their parameter names, the
checks that need no device refuse by name, and the Python entry points have the documented signatures (no compute calls)."""
import ctypes as C
import inspect
import os
import re

POST = "bfmmm_post_stacking"
POST_PARAMS = ["lpd", "n", "Q", "device", "init", "max_iter", "check_every", "tol", "weights", "pointwise", "objective", "gap", "n_iter",
               "converged"]
NAME = "bfmmm_chain_loo_by_chain"
PARAMS = ["h", "unit", "curves", "n_curves", "first_slot", "n_slots", "max_workspace_bytes", "lppd", "elpd_loo", "p_loo", "pareto_k",
          "elpd_waic", "p_waic", "capacity"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, name):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert decl, f"include/{header} does not declare {name}"
    return [re.split(r"[ *]", p.strip())[-1] for p in decl.group(1).split(",")]


def test_library_exports_the_entry_points():
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib, api
    lib = _lib.load()
    dp = _lib.c_double_p
    assert hasattr(lib, NAME) and hasattr(lib, POST) and hasattr(lib, "bfmmm_post_stacking_geometry")
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int64] + [dp] * 6 + [C.c_int64]
    assert _declared("bfmmm.h", NAME) == PARAMS and len(argtypes) == len(PARAMS)
    restype, argtypes = api.POST_SYMBOLS[POST]
    ip = C.POINTER(C.c_int)
    assert restype is C.c_int
    assert argtypes == [api.c_double_p, C.c_int64, C.c_int, C.c_int, api.c_double_p, C.c_int, C.c_int, C.c_double] + [api.c_double_p] * 4 + [ip, ip]
    assert _declared("bfmmm_post.h", POST) == POST_PARAMS and len(argtypes) == len(POST_PARAMS)
    threads, groups = api.stacking_geometry()
    assert threads % 64 == 0 and threads >= 64 and groups >= 1


def test_arguments_are_refused_by_name_before_a_device_is_touched():
    import numpy as np
    import __graft_entry__ as g
    g.build()
    from bayesfmmm_amd import _lib, api
    lib = _lib.load()
    args = [None, 1, None, 0, 0, 1, 0] + [None] * 6 + [0]
    assert len(args) == len(PARAMS)
    assert lib.bfmmm_chain_loo_by_chain(*args) != 0
    assert "bfmmm_chain_loo_by_chain: 'h' is null" in lib.bfmmm_last_error().decode()
    post = api._lib_entry()
    z = np.zeros(8)
    p = z.ctypes.data_as(api.c_double_p)
    it, cv = C.c_int(0), C.c_int(0)

    def call(**kw):
        a = dict(lpd=p, n=4, Q=2, device=0, init=None, max_iter=10, check_every=2, tol=1e-8, weights=p, pointwise=p, objective=p, gap=p,
                 n_iter=C.byref(it), converged=C.byref(cv))
        a.update(kw)
        assert post.bfmmm_post_stacking(*[a[k] for k in POST_PARAMS]) != 0
        return post.bfmmm_entry_last_error().decode()

    for name in ("lpd", "weights", "pointwise", "objective", "gap", "n_iter", "converged"):
        assert f"bfmmm_post_stacking: '{name}' is null" in call(**{name: None})
    assert "'n' must be at least 1" in call(n=0)
    assert "at most 64 candidates" in call(Q=65) and "'Q' must lie in 1 .. 64" in call(Q=0)
    assert "'max_iter' must be at least 1" in call(max_iter=0)
    assert "'check_every' must be at least 1" in call(check_every=0)
    assert "'tol' must be finite and not negative" in call(tol=-1.0)
    assert "'tol' must be finite and not negative" in call(tol=float("nan"))
    for init, what in (([0.5, 0.6], "add to 1.1"), ([1.0, 0.0], r"'init'[1]"), ([1.5, -0.5], r"'init'[1]"), ([float("nan"), 1.0], r"'init'[0]")):
        w = np.array(init)
        assert what in call(init=w.ctypes.data_as(api.c_double_p)), init


def test_python_signatures():
    from bayesfmmm_amd import api
    from bayesfmmm_amd.sampler import Sampler
    sig = inspect.signature(api.stacking)
    assert list(sig.parameters) == ["lpd", "init", "max_iter", "check_every", "tol", "device"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, 10000, 16, 1e-8, 0]
    assert list(inspect.signature(api.stack_models).parameters) == ["results", "names", "kw"]
    sig = inspect.signature(Sampler.loo_by_chain)
    assert list(sig.parameters)[1:] == ["unit", "curves", "first_slot", "n_slots", "max_workspace_bytes"]
    assert [p.default for p in sig.parameters.values()][1:] == ["observation", None, 0, None, 0]
    assert list(inspect.signature(Sampler.chain_stacking).parameters)[1:6] == ["unit", "curves", "first_slot", "n_slots", "max_workspace_bytes"]


def test_stack_models_refuses_unequal_lengths_and_compares_on_the_host():
    """the compare table is host arithmetic: against the long-double restatement without a device"""
    import numpy as np
    import pytest
    import stacking_ref as R
    from bayesfmmm_amd import api
    with pytest.raises(ValueError, match="same units"):
        api.stack_models([np.zeros(4), {"pointwise_elpd_loo": np.zeros(5)}])
    L = -1.0 + np.random.default_rng(3).standard_normal((50, 3)) * [0.5, 1.0, 0.7]
    tab, ref = api.compare_table(L), R.compare_table(L)
    assert tab["best"] == ref["best"]
    for k in ("elpd", "se", "elpd_diff", "se_diff", "pseudo_bma"):
        np.testing.assert_allclose(tab[k], ref[k].astype(float), rtol=1e-12, atol=0)
