"""The reference's R entry points for the functional model, over the C ABI of include/bfmmm_entry.h.

Function names, argument names, defaults and returned names follow
`BFMMM_Nu_Z_multiple_try`, `BFMMM_Theta_est` and `BFMMM_warm_start` of src/UserFunctions.cpp
(:166, :684, :1341; R wrappers R/RcppExports.R:1604, 1791, 2018).  Results are dicts of numpy arrays in
the reference's shapes (Fortran order); lists of per-curve vectors stay Python lists.

Extra keyword arguments that the reference does not have: `seed` (the reference uses R's global
RNG), `device`, `max_concurrent` (multi-try chains run concurrently on one GPU) and, for the
multi-GPU multi-try, `group` (a torch.distributed process group: chains are dealt round-robin to
the ranks, scores are all-gathered and the winning chain is broadcast; see parallel.py).
"""
import ctypes as C

import numpy as np

from . import _lib

c_double_p = _lib.c_double_p
c_int64_p = _lib.c_int64_p


class EntryArgs(C.Structure):
    """Mirror of `bfmmm_entry_args` (include/bfmmm_entry.h)."""
    _fields_ = [("n_funct", C.c_int32), ("y", c_double_p), ("t", c_double_p), ("offsets", c_int64_p),
                ("tot_mcmc_iters", C.c_int32), ("n_try", C.c_int32), ("K", C.c_int32), ("basis_degree", C.c_int32),
                ("n_eigen", C.c_int32), ("n_internal_knots", C.c_int32), ("boundary_knots", c_double_p),
                ("internal_knots", c_double_p), ("c", c_double_p), ("burnin_prop", C.c_double),
                ("b", C.c_double), ("nu_1", C.c_double), ("alpha1l", C.c_double), ("alpha2l", C.c_double),
                ("beta1l", C.c_double), ("beta2l", C.c_double), ("a_Z_PM", C.c_double), ("a_pi_PM", C.c_double),
                ("var_alpha3", C.c_double), ("var_epsilon1", C.c_double), ("var_epsilon2", C.c_double),
                ("alpha_nu", C.c_double), ("beta_nu", C.c_double), ("alpha_eta", C.c_double), ("beta_eta", C.c_double),
                ("alpha_0", C.c_double), ("beta_0", C.c_double), ("thinning_num", C.c_double), ("beta_N_t", C.c_double),
                ("N_t", C.c_int32), ("n_temp_trans", C.c_int32), ("r_stored_iters", C.c_int32),
                ("seed", C.c_uint64), ("device", C.c_int32), ("chain_offset", C.c_int32), ("chain_stride", C.c_int32),
                ("max_concurrent", C.c_int32), ("model", C.c_int32), ("P", C.c_int32),
                ("X", c_double_p), ("D", C.c_int32), ("covariance_adj", C.c_int32), ("dir", C.c_char_p),
                ("dim", C.c_int32), ("basis_degree_hd", C.POINTER(C.c_int32)), ("n_internal_hd", C.POINTER(C.c_int32)),
                ("progress_every", C.c_int32), ("progress_cb", C.c_void_p), ("progress_user", C.c_void_p),
                ("devices", C.POINTER(C.c_int32)), ("n_devices", C.c_int32)]


ENTRY_SYMBOLS = {
    "bfmmm_result_create": (C.c_void_p, []),
    "bfmmm_result_free": (None, [C.c_void_p]),
    "bfmmm_result_set": (C.c_int, [C.c_void_p, C.c_char_p, c_double_p, C.c_int64, c_int64_p, C.c_int]),
    "bfmmm_result_get": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(c_double_p), c_int64_p, C.POINTER(c_int64_p),
                                   C.POINTER(C.c_int)]),
    "bfmmm_result_count": (C.c_int, [C.c_void_p]),
    "bfmmm_result_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "bfmmm_entry_defaults": (None, [C.POINTER(EntryArgs), C.c_int]),
    "bfmmm_BFMMM_Nu_Z_multiple_try": (C.c_int, [C.POINTER(EntryArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_BFMMM_Theta_est": (C.c_int, [C.POINTER(EntryArgs), C.c_void_p, C.POINTER(C.c_void_p)]),
    "bfmmm_BFMMM_warm_start": (C.c_int, [C.POINTER(EntryArgs), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bfmmm_BMVMMM_Nu_Z_multiple_try": (C.c_int, [C.POINTER(EntryArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_BMVMMM_Theta_est": (C.c_int, [C.POINTER(EntryArgs), C.c_void_p, C.POINTER(C.c_void_p)]),
    "bfmmm_BMVMMM_warm_start": (C.c_int, [C.POINTER(EntryArgs), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bfmmm_BHDFMMM_Nu_Z_multiple_try": (C.c_int, [C.POINTER(EntryArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_BHDFMMM_Theta_est": (C.c_int, [C.POINTER(EntryArgs), C.c_void_p, C.POINTER(C.c_void_p)]),
    "bfmmm_BHDFMMM_warm_start": (C.c_int, [C.POINTER(EntryArgs), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "bfmmm_arma_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "bfmmm_arma_read_field": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "bfmmm_arma_write_ascii": (C.c_int, [C.c_char_p, c_double_p, c_int64_p, C.c_int]),
    "bfmmm_arma_write_field": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int64, C.c_int64]),
    "bfmmm_tensor_bspline": (C.c_int, [C.c_int, C.c_int, c_double_p, C.POINTER(C.c_int), c_double_p, C.POINTER(C.c_int),
                                       c_double_p, c_double_p]),
    "bfmmm_tensor_penalty": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p]),
    "bfmmm_entry_last_error": (C.c_char_p, []),
}

_bound = False


class PostInput(C.Structure):
    """bfmmm_post_input of include/bfmmm_post.h."""
    _fields_ = [("n", C.c_int32), ("K", C.c_int32), ("P", C.c_int32), ("M", C.c_int32), ("D", C.c_int32),
                ("offsets", c_int64_p), ("y", c_double_p), ("B", c_double_p), ("X", c_double_p), ("T", C.c_int32),
                ("nu", c_double_p), ("Phi", c_double_p), ("Z", c_double_p), ("chi", c_double_p), ("sigma", c_double_p),
                ("eta", c_double_p), ("xi", c_double_p), ("device", C.c_int32), ("identity_basis", C.c_int32)]


class PostArgs(C.Structure):
    """bfmmm_post_args of include/bfmmm_post.h."""
    _fields_ = [("dir", C.c_char_p), ("n_files", C.c_int32), ("basis_degree", C.c_int32), ("n_internal_knots", C.c_int32),
                ("boundary_knots", c_double_p), ("internal_knots", c_double_p), ("n_funct", C.c_int32),
                ("t", c_double_p), ("y", c_double_p), ("offsets", c_int64_p), ("burnin_prop", C.c_double),
                ("X", c_double_p), ("D", C.c_int32), ("cov_adj", C.c_int32), ("device", C.c_int32), ("P", C.c_int32)]


class CiArgs(C.Structure):
    """bfmmm_ci_args of include/bfmmm_post.h."""
    _fields_ = [("dir", C.c_char_p), ("n_files", C.c_int32), ("time", c_double_p), ("n_time", C.c_int32),
                ("basis_degree", C.c_int32), ("n_internal_knots", C.c_int32), ("boundary_knots", c_double_p),
                ("internal_knots", c_double_p), ("k", C.c_int32), ("alpha", C.c_double), ("rescale", C.c_int32),
                ("simultaneous", C.c_int32), ("burnin_prop", C.c_double), ("X", c_double_p), ("n_x", C.c_int32), ("D", C.c_int32),
                ("trans_mats", c_double_p), ("device", C.c_int32), ("time2", c_double_p), ("n_time2", C.c_int32),
                ("l", C.c_int32), ("m", C.c_int32), ("dim", C.c_int32), ("basis_degree_hd", C.POINTER(C.c_int32)),
                ("n_internal_hd", C.POINTER(C.c_int32))]


POST_SYMBOLS = {
    "bfmmm_post_col_quantiles": (C.c_int, [c_double_p, C.c_int32, C.c_int32, c_double_p, C.c_int32, C.c_int32, c_double_p]),
    "bfmmm_post_bands": (C.c_int, [c_double_p, C.c_int32, C.c_int32, c_double_p, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                   c_double_p, c_double_p, c_double_p, c_double_p]),
    "bfmmm_post_cov_bands": (C.c_int, [c_double_p, c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p, C.c_int32,
                                       C.c_double, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p]),
    "bfmmm_FCovCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_HDFCovCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_MVCovCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_MVMeanCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_HDFMeanCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_ci_defaults": (None, [C.POINTER(CiArgs)]),
    "bfmmm_SigmaCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_ZCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_FMeanCI": (C.c_int, [C.POINTER(CiArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_post_pointwise": (C.c_int, [C.POINTER(PostInput), C.c_int32, c_double_p, c_double_p, c_double_p]),
    "bfmmm_post_pointwise_joint": (C.c_int, [C.POINTER(PostInput), C.c_int32, c_double_p, c_double_p, c_double_p]),
    "bfmmm_post_cpo": (C.c_int, [C.POINTER(PostInput), C.c_int32, c_double_p]),
    "bfmmm_post_curve_loglik": (C.c_int, [C.POINTER(PostInput), C.c_int32, c_double_p]),
    "bfmmm_post_psis": (C.c_int, [c_double_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p,
                                  c_double_p, c_double_p]),
    "bfmmm_post_psis_expect": (C.c_int, [c_double_p, c_double_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [c_double_p] * 7),
    "bfmmm_post_stacking": (C.c_int, [c_double_p, C.c_int64, C.c_int, C.c_int, c_double_p, C.c_int, C.c_int, C.c_double, c_double_p,
                                      c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bfmmm_post_stacking_geometry": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bfmmm_FLOO": (C.c_int, [C.POINTER(PostArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_post_diagnostics": (C.c_int, [c_double_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p,
                                         c_double_p, c_double_p, c_double_p, c_double_p]),
    "bfmmm_MVLOO": (C.c_int, [C.POINTER(PostArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_ConditionalPredictiveOrdinates": (C.c_int, [C.POINTER(PostArgs), C.c_int32, C.POINTER(C.c_void_p)]),
    "bfmmm_post_last_kernel_ms": (C.c_double, []),
    "bfmmm_FSamplePaths": (C.c_int, [C.POINTER(PostArgs), C.c_double, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "bfmmm_post_sample_paths": (C.c_int, [C.POINTER(PostInput), C.c_int32, C.c_uint64, c_double_p, c_double_p]),
    "bfmmm_post_table_bands": (C.c_int, [c_double_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p]),
    "bfmmm_MVLLik": (C.c_int, [C.POINTER(PostArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_MVDIC": (C.c_int, [C.POINTER(PostArgs), c_double_p]),
    "bfmmm_MVAIC": (C.c_int, [C.POINTER(PostArgs), c_double_p]),
    "bfmmm_MVBIC": (C.c_int, [C.POINTER(PostArgs), c_double_p]),
    "bfmmm_post_defaults": (None, [C.POINTER(PostArgs)]),
    "bfmmm_FLLik": (C.c_int, [C.POINTER(PostArgs), C.POINTER(C.c_void_p)]),
    "bfmmm_FDIC": (C.c_int, [C.POINTER(PostArgs), c_double_p]),
    "bfmmm_FAIC": (C.c_int, [C.POINTER(PostArgs), c_double_p]),
    "bfmmm_FBIC": (C.c_int, [C.POINTER(PostArgs), c_double_p]),
}


def _lib_entry():
    global _bound
    lib = _lib.load()
    if not _bound:
        for name, (res, args) in list(ENTRY_SYMBOLS.items()) + list(POST_SYMBOLS.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return lib


def _check(rc):
    if rc != 0:
        raise _lib.BfmmmError(_lib_entry().bfmmm_entry_last_error().decode())


def _set_kw(owner, a, kw):
    """remaining keyword arguments are fields of bfmmm_entry_args; `devices` (a list of GPU indices) selects the
    multi-GPU multi-try of include/bfmmm_entry.h"""
    devices = kw.pop("devices", None)
    if devices is not None:
        owner.devices = (C.c_int32 * len(devices))(*[int(x) for x in devices])
        a.devices, a.n_devices = owner.devices, len(devices)
    for k, v in kw.items():
        if not hasattr(a, k):
            raise TypeError(f"unexpected argument '{k}'")
        setattr(a, k, v)


class _ArgsMV:
    """bfmmm_entry_args of the multivariate entry points: Y is the n x P matrix."""

    def __init__(self, entry, tot_mcmc_iters, K, Y, n_eigen, X, kw):
        lib = _lib_entry()
        self.a = EntryArgs()
        lib.bfmmm_entry_defaults(C.byref(self.a), entry)
        self.Y = np.asfortranarray(Y, dtype=np.float64)
        n, P = self.Y.shape
        a = self.a
        a.n_funct, a.P, a.tot_mcmc_iters, a.K, a.n_eigen = n, P, tot_mcmc_iters, K, n_eigen
        a.y = self.Y.ctypes.data_as(c_double_p)
        self.P, self.offsets = P, None
        if X is not None:        # UserFunctions.cpp:4582 / :5000 / :5545 (`X`, `covariance_adj`)
            self.X = np.asfortranarray(X, dtype=np.float64)
            if self.X.shape[0] != n:
                raise _lib.BfmmmError("'X' must be have 'n_funct' number of rows")
            a.X, a.D = self.X.ctypes.data_as(c_double_p), self.X.shape[1]
            a.covariance_adj = int(bool(kw.pop("covariance_adj", False)))
        else:
            kw.pop("covariance_adj", None)
        c = kw.pop("c", None)
        if c is not None:
            self.c = np.ascontiguousarray(c, dtype=np.float64)
            if self.c.size != K:
                raise _lib.BfmmmError("number of elements of the vector 'c' must be equal to K")
            a.c = self.c.ctypes.data_as(c_double_p)
        _set_kw(self, a, kw)


def _result_to_dict(lib, res, offsets, P):
    out = {}
    for i in range(lib.bfmmm_result_count(res)):
        name = lib.bfmmm_result_name(res, i)
        data, cnt, dims, nd = c_double_p(), C.c_int64(), c_int64_p(), C.c_int()
        _check(lib.bfmmm_result_get(res, name, C.byref(data), C.byref(cnt), C.byref(dims), C.byref(nd)))
        shape = tuple(dims[k] for k in range(nd.value))
        arr = np.ctypeslib.as_array(data, shape=(cnt.value,)).copy() if cnt.value > 0 else np.zeros(0)
        key = name.decode()
        if key in ("B", "B_obs") and offsets is not None:
            rows = arr.reshape(-1, P)
            out[key] = [rows[offsets[j]:offsets[j + 1]].copy() for j in range(len(offsets) - 1)]
        elif key in ("best_chain", "best_score"):
            out[key] = float(arr[0])
        else:
            out[key] = arr.reshape(shape, order="F")
    return out


def _dict_to_result(lib, d):
    res = C.c_void_p(lib.bfmmm_result_create())
    for key, val in d.items():
        if key in ("B", "B_obs", "best_chain", "best_score"):
            continue
        a = np.asfortranarray(np.asarray(val, dtype=np.float64))
        flat = np.ascontiguousarray(a.reshape(-1, order="F"))
        dims = (C.c_int64 * a.ndim)(*a.shape)
        _check(lib.bfmmm_result_set(res, key.encode(), flat.ctypes.data_as(c_double_p), flat.size, dims, a.ndim))
    return res


class _Args:
    """Owns the numpy buffers behind a bfmmm_entry_args."""

    def __init__(self, entry, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots,
                 internal_knots, X, kw):
        if len(Y) != n_funct or len(time) != n_funct:
            raise ValueError("'Y' and 'time' must have 'n_funct' elements")
        lib = _lib_entry()
        self.a = EntryArgs()
        lib.bfmmm_entry_defaults(C.byref(self.a), entry)
        self.offsets = np.zeros(n_funct + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum([len(v) for v in Y])
        self.y = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in Y]))
        self.t = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in time]))
        self.bk = np.ascontiguousarray(boundary_knots, dtype=np.float64)
        self.ik = np.ascontiguousarray(internal_knots, dtype=np.float64)
        a = self.a
        a.n_funct, a.tot_mcmc_iters, a.K, a.basis_degree, a.n_eigen = n_funct, tot_mcmc_iters, K, basis_degree, n_eigen
        a.n_internal_knots = len(self.ik)
        a.y, a.t = self.y.ctypes.data_as(c_double_p), self.t.ctypes.data_as(c_double_p)
        a.offsets = self.offsets.ctypes.data_as(c_int64_p)
        a.boundary_knots, a.internal_knots = self.bk.ctypes.data_as(c_double_p), self.ik.ctypes.data_as(c_double_p)
        self.P = len(self.ik) + basis_degree + 1
        if X is not None:
            self.X = np.asfortranarray(X, dtype=np.float64)
            if self.X.shape[0] != n_funct:
                raise _lib.BfmmmError("'X' must be have 'n_funct' number of rows")
            a.X, a.D = self.X.ctypes.data_as(c_double_p), self.X.shape[1]
            a.covariance_adj = int(bool(kw.pop("covariance_adj", False)))
        else:
            kw.pop("covariance_adj", None)
        c = kw.pop("c", None)
        if c is not None:
            self.c = np.ascontiguousarray(c, dtype=np.float64)
            if self.c.size != K:
                raise _lib.BfmmmError("number of elements of the vector 'c' must be equal to K")
            a.c = self.c.ctypes.data_as(c_double_p)
        _set_kw(self, a, kw)


def BFMMM_Nu_Z_multiple_try(tot_mcmc_iters, n_try, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots,
                            internal_knots, X=None, group=None, **kw):
    """src/UserFunctions.cpp:166.  Runs 1 + n_try independent chains of the (Z, pi, alpha_3, nu, tau, sigma^2)
    sweep and returns the chain with the largest mean log-likelihood over its last 99 draws."""
    lib = _lib_entry()
    args = _Args(0, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw)
    args.a.n_try = n_try
    if group is not None:
        from . import parallel
        return parallel.multi_try(lambda: _call1(lib.bfmmm_BFMMM_Nu_Z_multiple_try, args), args, group)
    return _call1(lib.bfmmm_BFMMM_Nu_Z_multiple_try, args)


PROGRESS_CB = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_double, C.c_void_p)


def set_progress(args, every, fn):
    """Attach a progress callback fn(iteration, loglik) -> truthy to abort (warm start; include/bfmmm_entry.h)."""
    args._cb = PROGRESS_CB(lambda it, ll, user: 1 if fn(it, ll) else 0)
    args.a.progress_every = int(every)
    args.a.progress_cb = C.cast(args._cb, C.c_void_p)


def _call1(fn, args, *prev):
    lib = _lib_entry()
    res = C.c_void_p()
    handles = [_dict_to_result(lib, p) for p in prev]
    try:
        _check(fn(C.byref(args.a), *handles, C.byref(res)))
        return _result_to_dict(lib, res, args.offsets, args.P)
    finally:
        for h in handles:
            lib.bfmmm_result_free(h)
        if res:
            lib.bfmmm_result_free(res)


def BFMMM_Theta_est(tot_mcmc_iters, n_try, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots,
                    multiple_try, X=None, burnin_prop=0.8, group=None, **kw):
    """src/UserFunctions.cpp:684.  Conditions on the posterior medians of Z and nu from stage 1 and samples
    (Phi, delta, A, gamma, tau, sigma^2, chi); best of 1 + n_try chains."""
    lib = _lib_entry()
    args = _Args(1, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw)
    args.a.n_try, args.a.burnin_prop = n_try, burnin_prop
    mt = {k: multiple_try[k] for k in ("Z", "nu") + (("eta",) if X is not None else ())}
    if group is not None:
        from . import parallel
        return parallel.multi_try(lambda: _call1(lib.bfmmm_BFMMM_Theta_est, args, mt), args, group)
    return _call1(lib.bfmmm_BFMMM_Theta_est, args, mt)


def BFMMM_warm_start(tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots,
                     multiple_try, theta_est, X=None, burnin_prop=0.8, dir=None, **kw):
    """src/UserFunctions.cpp:1341.  Full sampler started at the posterior medians of stages 1 and 2."""
    lib = _lib_entry()
    progress = kw.pop("progress", None)          # (every, fn(iteration, loglik) -> truthy to abort)
    args = _Args(2, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw)
    if progress is not None:
        set_progress(args, *progress)
    args.a.burnin_prop = burnin_prop
    if dir is not None:      # <dir>Nu<q>.txt, ... are written as the reference does (string concatenation: end it with "/")
        args.dir = str(dir).encode()
        args.a.dir = args.dir
    mt = {k: multiple_try[k] for k in ("Z", "nu", "pi", "alpha_3", "tau") + (("eta", "tau_eta") if X is not None else ())}
    te_names = ("delta", "gamma", "Phi", "A", "sigma_sq", "chi")
    if X is not None and args.a.covariance_adj:
        te_names += ("xi", "gamma_xi", "delta_xi", "A_xi")
    te = {k: theta_est[k] for k in te_names}
    return _call1(lib.bfmmm_BFMMM_warm_start, args, mt, te)


def BMVMMM_Nu_Z_multiple_try(tot_mcmc_iters, n_try, K, Y, n_eigen, X=None, group=None, **kw):
    """src/UserFunctions.cpp:4579 (multivariate model: Y is an n x P matrix, no basis)."""
    lib = _lib_entry()
    args = _ArgsMV(3, tot_mcmc_iters, K, Y, n_eigen, X, kw)
    args.a.n_try = n_try
    if group is not None:
        from . import parallel
        return parallel.multi_try(lambda: _call1(lib.bfmmm_BMVMMM_Nu_Z_multiple_try, args), args, group)
    return _call1(lib.bfmmm_BMVMMM_Nu_Z_multiple_try, args)


def BMVMMM_Theta_est(tot_mcmc_iters, n_try, K, Y, n_eigen, multiple_try, X=None, burnin_prop=0.8, group=None, **kw):
    """src/UserFunctions.cpp:4995."""
    lib = _lib_entry()
    args = _ArgsMV(4, tot_mcmc_iters, K, Y, n_eigen, X, kw)
    args.a.n_try, args.a.burnin_prop = n_try, burnin_prop
    mt = {k: multiple_try[k] for k in ("Z", "nu") + (("eta",) if X is not None else ())}
    if group is not None:
        from . import parallel
        return parallel.multi_try(lambda: _call1(lib.bfmmm_BMVMMM_Theta_est, args, mt), args, group)
    return _call1(lib.bfmmm_BMVMMM_Theta_est, args, mt)


def BMVMMM_warm_start(tot_mcmc_iters, K, Y, n_eigen, multiple_try, theta_est, X=None, burnin_prop=0.8, dir=None, **kw):
    """src/UserFunctions.cpp:5540."""
    lib = _lib_entry()
    args = _ArgsMV(5, tot_mcmc_iters, K, Y, n_eigen, X, kw)
    args.a.burnin_prop = burnin_prop
    if dir is not None:
        args.dir = str(dir).encode()
        args.a.dir = args.dir
    mt = {k: multiple_try[k] for k in ("Z", "nu", "pi", "alpha_3", "tau") + (("eta", "tau_eta") if X is not None else ())}
    te_names = ("delta", "gamma", "Phi", "A", "sigma_sq", "chi")
    if X is not None and args.a.covariance_adj:
        te_names += ("xi", "gamma_xi", "delta_xi", "A_xi")
    te = {k: theta_est[k] for k in te_names}
    return _call1(lib.bfmmm_BMVMMM_warm_start, args, mt, te)


# ---- readers / writers of the on-disk chain batches (src/UserFunctions.cpp:2157-2357) ---------------------------
def _read(fn, file):
    lib = _lib_entry()
    res = C.c_void_p()
    try:
        _check(fn(str(file).encode(), C.byref(res)))
        return _result_to_dict(lib, res, None, 0)
    finally:
        if res:
            lib.bfmmm_result_free(res)


def ReadVec(file):
    """src/UserFunctions.cpp:2158 (arma::vec::load): 1-d array."""
    return _read(_lib_entry().bfmmm_arma_read, file)["value"].reshape(-1, order="F")


def ReadMat(file):
    """src/UserFunctions.cpp:2205."""
    return _read(_lib_entry().bfmmm_arma_read, file)["value"]


def ReadCube(file):
    """src/UserFunctions.cpp:2253."""
    return _read(_lib_entry().bfmmm_arma_read, file)["value"]


def _read_field(file):
    d = _read(_lib_entry().bfmmm_arma_read_field, file)
    nr, nc = (int(x) for x in d["field_dims"])
    out = np.empty((nr, nc), dtype=object)
    for e in range(nr * nc):
        out[e % nr, e // nr] = d[str(e)]
    return out


def ReadFieldCube(file):
    """src/UserFunctions.cpp:2303: object array (n_rows, n_cols) of cubes."""
    return _read_field(file)


def ReadFieldMat(file):
    """src/UserFunctions.cpp:2351."""
    return _read_field(file)


def ReadFieldVec(file):
    """src/UserFunctions.cpp:2399: object array of 1-d arrays."""
    f = _read_field(file)
    for idx in np.ndindex(f.shape):
        f[idx] = f[idx].reshape(-1, order="F")
    return f


def write_arma_ascii(file, x):
    """`x.save(file, arma::arma_ascii)` for a vector (saved as an n x 1 matrix), matrix or cube."""
    a = np.asfortranarray(np.asarray(x, dtype=np.float64))
    if a.ndim == 1:
        a = a.reshape(-1, 1, order="F")
    flat = np.ascontiguousarray(a.reshape(-1, order="F"))
    dims = (C.c_int64 * a.ndim)(*a.shape)
    _check(_lib_entry().bfmmm_arma_write_ascii(str(file).encode(), flat.ctypes.data_as(c_double_p), dims, a.ndim))


def write_arma_field(file, field):
    """`field.save(file)` (arma_binary) for an object array (n_rows, n_cols) of matrices / cubes."""
    lib = _lib_entry()
    field = np.asarray(field, dtype=object)
    if field.ndim == 1:
        field = field.reshape(-1, 1)
    nr, nc = field.shape
    items = {}
    for e in range(nr * nc):
        v = np.asarray(field[e % nr, e // nr], dtype=np.float64)
        items[str(e)] = v.reshape(-1, 1) if v.ndim == 1 else v
    res = _dict_to_result(lib, items)
    try:
        _check(lib.bfmmm_arma_write_field(str(file).encode(), res, nr, nc))
    finally:
        lib.bfmmm_result_free(res)


# ---- the on-disk chain batches as chain slots of a Sampler ----------------------------------------------
# file name -> (get_chain name, kind): "cube" / "vec" / "mat" (draws along the last axis), "rows" (a draw a row: Tau), "field" (a
# field of one cube per draw), "fieldK" (a field of K cubes per draw: (draw, cluster)), "cube_head" / "field_head": containers of
# r_stored_iters entries of which only the first per_file are draws (save_batch in entry_points.cpp)
_BATCH_FILES = (("Nu", "nu", "cube", 0), ("Chi", "chi", "cube", 0), ("Z", "Z", "cube", 0), ("Sigma", "sigma_sq", "vec", 0),
                ("Phi", "Phi", "field", 0), ("Pi", "pi", "mat", 0), ("alpha_3", "alpha_3", "vec", 0), ("A", "A", "cube", 0),
                ("Delta", "delta", "cube", 0), ("Tau", "tau", "rows", 0), ("Gamma", "gamma", "field", 0),
                ("Eta", "eta", "field", 1), ("Tau_Eta", "tau_eta", "cube_head", 1),
                ("Xi", "xi", "fieldK", 2), ("Gamma_Xi", "gamma_xi", "fieldK", 2), ("Delta_Xi", "delta_xi", "field", 2),
                ("A_Xi", "A_xi", "field", 2))
_BATCH_REQUIRED = ("Nu", "Chi", "Z", "Sigma", "Phi")


def read_batches(dir, n_files, X=False, cov_adj=False, drop_unassigned=False):
    """The reference's on-disk chain batches `<dir><Name><q>.txt`, q < n_files (BFMMM_warm_start and its relatives with `dir=`), as
    arrays in Sampler.get_chain's layouts, concatenated over the files along the draws: a dict with "nu" (K, P, T), "chi"
    (n, M, T), "Z" (n, K, T), "sigma_sq" (T,), "Phi" (K, P, M, T) and, where the files exist, "pi", "alpha_3", "A", "delta", "tau"
    ((T, K)) and "gamma"; with X also "eta" and "tau_eta"; with cov_adj also "xi", "gamma_xi", "delta_xi" and "A_xi"; and
    "n_draws" = T.  What Sampler.load_chain takes.
    The covariate containers of a file hold r_stored_iters entries of which only the first per_file (the draws of Nu<q>.txt) are
    draws; the rest is dropped.  The first entry of alpha_3 in every file is the reference's unassigned 0.  The default keeps that
    draw, so that slot indices and `burnin_prop` mean what they mean for every file-route function (FLLik, ZCI, ...); predict and
    loo_marginal, which read alpha_3, must then start after it (first_slot >= 1, one file).  drop_unassigned=True leaves the first
    draw of every file out of every array instead."""
    import os
    if n_files <= 0:
        raise ValueError("'n_files' must be greater than 0")
    level = 2 if (X and cov_adj) else 1 if X else 0
    parts = {}
    per_file = []
    for q in range(int(n_files)):
        per = None
        for fname, key, kind, lvl in _BATCH_FILES:
            if lvl > level:
                continue
            path = os.path.join(str(dir), f"{fname}{q}.txt")
            if not os.path.exists(path):
                if fname in _BATCH_REQUIRED or key in parts:
                    raise FileNotFoundError(f"read_batches: '{path}' is missing")
                continue
            if q > 0 and key not in parts:
                raise FileNotFoundError(f"read_batches: '{fname}<q>.txt' exists for q = {q} but not for q = 0")
            if kind == "vec":
                a = ReadVec(path)
            elif kind in ("cube", "mat", "rows", "cube_head"):
                a = ReadCube(path)
            else:
                f = ReadFieldCube(path)
                if per is not None and f.shape[0] < per:
                    raise ValueError(f"'{fname}<q>.txt' holds fewer draws than 'Nu<q>.txt'")
                rows = range(f.shape[0] if per is None else per)
                if kind == "fieldK":
                    a = np.stack([np.stack([f[l, k] for k in range(f.shape[1])], axis=-1) for l in rows], axis=-1)
                else:
                    a = np.stack([f[l, 0] for l in rows], axis=-1)
            if fname == "Nu":
                per = a.shape[-1]
                per_file.append(per)
            if kind == "cube_head":
                a = a[..., :per]
            have = a.shape[0] if kind == "rows" else a.shape[-1]
            if have != per:
                raise ValueError(f"'{fname}{q}.txt' holds {have} draws, 'Nu{q}.txt' {per}")
            if q > 0:
                lead0 = parts[key][0].shape[1:] if kind == "rows" else parts[key][0].shape[:-1]
                lead = a.shape[1:] if kind == "rows" else a.shape[:-1]
                if lead != lead0:
                    raise ValueError(f"files '{fname}<q>.txt' differ in size")
            if drop_unassigned:
                a = a[1:] if kind == "rows" else a[..., 1:]
            parts.setdefault(key, []).append(a)
    out = {}
    for fname, key, kind, lvl in _BATCH_FILES:
        if key in parts:
            out[key] = np.asfortranarray(np.concatenate(parts[key], axis=0 if kind == "rows" else -1))
    out["n_draws"] = int(sum(per_file)) - (len(per_file) if drop_unassigned else 0)
    return out


def open_batches(dirs, n_files, Y, time=None, basis_degree=None, boundary_knots=None, internal_knots=None, X=None, cov_adj=False,
                 drop_unassigned=False, device=0, **cfg_kw):
    """A Sampler whose chain slots hold saved chains: `dirs` is one directory of on-disk batches (read_batches) or a list of them,
    one chain each.  K, n_eigen, P and the number of draws T are read off the files; the sampler is built over Y (and time with
    the spline basis; the multivariate model where time is None) with tot_mcmc_iters = T and n_chains = len(dirs), X is set where
    given, every chain is loaded into slots [0, T) and the "loglik" slots are filled by slot_loglik(store=True).  Every summary
    that reads chain slots (diagnostics, align, cluster_mean_bands, curve_bands, similarity, loo, predict, ...) then works on the
    saved draws.  cfg_kw: further fields of the configuration.  Files that disagree with each other, with Y or with the basis
    are refused."""
    from .sampler import MODEL_FUNCTIONAL, MODEL_MULTIVARIATE, Sampler, default_config
    if isinstance(dirs, (str, bytes)) or hasattr(dirs, "__fspath__"):
        dirs = [dirs]
    dirs = list(dirs)
    if not dirs:
        raise ValueError("open_batches: 'dirs' is empty")
    chains = [read_batches(d, n_files, X=X is not None, cov_adj=cov_adj, drop_unassigned=drop_unassigned) for d in dirs]
    c0 = chains[0]
    K, P, T = c0["nu"].shape
    n, M = c0["chi"].shape[:2]
    for d, c in zip(dirs[1:], chains[1:]):
        for key in c0:
            same = c[key] == c0[key] if key == "n_draws" else (key in c and c[key].shape == c0[key].shape)
            if not same:
                raise ValueError(f"open_batches: the files of '{d}' and of '{dirs[0]}' differ in '{key}'")
    if c0["Z"].shape[:2] != (n, K) or c0["Phi"].shape[:3] != (K, P, M):
        raise ValueError("open_batches: the files 'Nu', 'Chi', 'Z' and 'Phi' differ in size")
    mv = time is None
    n_y = np.shape(Y)[0] if mv else len(Y)
    if n_y != n:
        raise ValueError("The number of functions in 'Y' must be equal to the number of rows of the saved 'Z' draws")
    if X is not None:
        Xm = np.asarray(X, dtype=np.float64)
        if Xm.ndim != 2 or Xm.shape[0] != n or Xm.shape[1] != c0["eta"].shape[1]:
            raise ValueError("The number of columns in 'X' must be equal to the number of covariates in the model")
    if mv:
        if np.ndim(Y) != 2 or np.shape(Y)[1] != P:
            raise ValueError("the saved draws do not match the number of columns of 'Y'")
        cfg = default_config(model=MODEL_MULTIVARIATE, K=int(K), n_eigen=int(M), tot_mcmc_iters=int(T), **cfg_kw)
        s = Sampler(cfg, Y, device=device, n_chains=len(dirs))
    else:
        if basis_degree is None or boundary_knots is None or internal_knots is None:
            raise ValueError("open_batches: 'basis_degree', 'boundary_knots' and 'internal_knots' are needed with 'time'")
        if P != len(internal_knots) + int(basis_degree) + 1:
            raise ValueError("the saved draws do not match the basis ('basis_degree', 'internal_knots')")
        cfg = default_config(model=MODEL_FUNCTIONAL, K=int(K), n_eigen=int(M), basis_degree=int(basis_degree), tot_mcmc_iters=int(T), **cfg_kw)
        s = Sampler(cfg, Y, time, internal_knots, boundary_knots, device=device, n_chains=len(dirs))
    try:
        if X is not None:
            s.set_covariates(X, covariance_adj=cov_adj)
        for q, c in enumerate(chains):
            s.load_chain({k: v for k, v in c.items() if k != "n_draws"}, chain=q)
        s.slot_loglik(store=True)
    except Exception:
        s.close()
        raise
    return s


# ---- set-up pieces of the high-dimensional functional model (BSplines.h:18-120) -----------------------------------
def TensorBSpline(t, basis_degree, boundary_knots, internal_knots):
    """Tensor-product B-spline basis of the points t (n_pts x dim): n_pts x prod_l (len(internal_knots[l]) + degree[l] + 1)."""
    t = np.asfortranarray(np.asarray(t, dtype=np.float64))
    n_pts, dim = t.shape
    deg = (C.c_int * dim)(*[int(x) for x in basis_degree])
    nint = (C.c_int * dim)(*[len(k) for k in internal_knots])
    bk = np.ascontiguousarray(np.asarray(boundary_knots, dtype=np.float64).reshape(dim, 2))
    ik = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float64).reshape(-1) for k in internal_knots]) if dim else [])
    P = int(np.prod([len(k) + int(g) + 1 for k, g in zip(internal_knots, basis_degree)]))
    out = np.zeros((n_pts, P), order="F")
    _check(_lib_entry().bfmmm_tensor_bspline(n_pts, dim, t.ctypes.data_as(c_double_p), deg, bk.ctypes.data_as(c_double_p), nint,
                                             ik.ctypes.data_as(c_double_p), out.ctypes.data_as(c_double_p)))
    return out


def GetP(basis_degree, n_internal_knots):
    """Penalty matrix of the tensor-product basis (BSplines.h:74-120)."""
    dim = len(basis_degree)
    deg = (C.c_int * dim)(*[int(x) for x in basis_degree])
    nint = (C.c_int * dim)(*[int(x) for x in n_internal_knots])
    P = int(np.prod([int(k) + int(g) + 1 for k, g in zip(n_internal_knots, basis_degree)]))
    out = np.zeros((P, P), order="F")
    _check(_lib_entry().bfmmm_tensor_penalty(dim, deg, nint, out.ctypes.data_as(c_double_p)))
    return out


# ---- high-dimensional functional model (src/UserFunctions.cpp:2519, :3030, :3676) --------------------------------
class _ArgsHD:
    """bfmmm_entry_args of the BHDFMMM_* entry points: `time` is a list of n_i x dim matrices, `basis_degree` a vector,
    `boundary_knots` a dim x 2 matrix, `internal_knots` a list of vectors."""

    def __init__(self, entry, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw):
        if len(Y) != n_funct or len(time) != n_funct:
            raise ValueError("'Y' and 'time' must have 'n_funct' elements")
        lib = _lib_entry()
        self.a = EntryArgs()
        lib.bfmmm_entry_defaults(C.byref(self.a), entry)
        dim = len(basis_degree)
        tm = [np.asfortranarray(np.asarray(t, dtype=np.float64).reshape(len(y), -1)) for t, y in zip(time, Y)]
        if tm[0].shape[1] != dim:
            raise _lib.BfmmmError("number of elemnts in 'basis_degree' does not match number of columns in time matrix")
        self.offsets = np.zeros(n_funct + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum([len(v) for v in Y])
        self.y = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in Y]))
        self.t = np.ascontiguousarray(np.concatenate([t.reshape(-1, order="F") for t in tm]))
        self.bk = np.ascontiguousarray(np.asarray(boundary_knots, dtype=np.float64).reshape(dim, 2))
        self.ik = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float64).reshape(-1) for k in internal_knots]))
        self.deg = (C.c_int32 * dim)(*[int(x) for x in basis_degree])
        self.nint = (C.c_int32 * dim)(*[len(k) for k in internal_knots])
        a = self.a
        a.n_funct, a.tot_mcmc_iters, a.K, a.n_eigen, a.dim = n_funct, tot_mcmc_iters, K, n_eigen, dim
        a.basis_degree = max(int(x) for x in basis_degree)
        a.y, a.t = self.y.ctypes.data_as(c_double_p), self.t.ctypes.data_as(c_double_p)
        a.offsets = self.offsets.ctypes.data_as(c_int64_p)
        a.boundary_knots, a.internal_knots = self.bk.ctypes.data_as(c_double_p), self.ik.ctypes.data_as(c_double_p)
        a.basis_degree_hd, a.n_internal_hd = self.deg, self.nint
        self.P = int(np.prod([len(k) + int(g) + 1 for k, g in zip(internal_knots, basis_degree)]))
        if X is not None:        # UserFunctions.cpp:2531 / :3043 / :3689 (`X`, `covariance_adj`)
            self.X = np.asfortranarray(X, dtype=np.float64)
            if self.X.shape[0] != n_funct:
                raise _lib.BfmmmError("'X' must be have 'n_funct' number of rows")
            a.X, a.D = self.X.ctypes.data_as(c_double_p), self.X.shape[1]
            a.covariance_adj = int(bool(kw.pop("covariance_adj", False)))
        else:
            kw.pop("covariance_adj", None)
        c = kw.pop("c", None)
        if c is not None:
            self.c = np.ascontiguousarray(c, dtype=np.float64)
            if self.c.size != K:
                raise _lib.BfmmmError("number of elements of the vector 'c' must be equal to K")
            a.c = self.c.ctypes.data_as(c_double_p)
        _set_kw(self, a, kw)


def BHDFMMM_Nu_Z_multiple_try(tot_mcmc_iters, n_try, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots,
                              internal_knots, X=None, **kw):
    """src/UserFunctions.cpp:2519."""
    lib = _lib_entry()
    args = _ArgsHD(0, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw)
    args.a.n_try = n_try
    return _call1(lib.bfmmm_BHDFMMM_Nu_Z_multiple_try, args)


def BHDFMMM_Theta_est(tot_mcmc_iters, n_try, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots,
                      multiple_try, X=None, burnin_prop=0.8, **kw):
    """src/UserFunctions.cpp:3030."""
    lib = _lib_entry()
    args = _ArgsHD(1, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw)
    args.a.n_try, args.a.burnin_prop = n_try, burnin_prop
    mt = {k: multiple_try[k] for k in ("Z", "nu") + (("eta",) if X is not None else ())}
    return _call1(lib.bfmmm_BHDFMMM_Theta_est, args, mt)


def BHDFMMM_warm_start(tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots,
                       multiple_try, theta_est, X=None, burnin_prop=0.8, dir=None, **kw):
    """src/UserFunctions.cpp:3676."""
    lib = _lib_entry()
    args = _ArgsHD(2, tot_mcmc_iters, K, Y, time, n_funct, basis_degree, n_eigen, boundary_knots, internal_knots, X, kw)
    args.a.burnin_prop = burnin_prop
    if dir is not None:
        args.dir = str(dir).encode()
        args.a.dir = args.dir
    mt = {k: multiple_try[k] for k in ("Z", "nu", "pi", "alpha_3", "tau") + (("eta", "tau_eta") if X is not None else ())}
    te_names = ("delta", "gamma", "Phi", "A", "sigma_sq", "chi")
    if X is not None and args.a.covariance_adj:
        te_names += ("xi", "gamma_xi", "delta_xi", "A_xi")
    return _call1(lib.bfmmm_BHDFMMM_warm_start, args, mt, {k: theta_est[k] for k in te_names})


# ---- likelihood-based post-processing (src/PostProcessing.cpp:3660-5114; include/bfmmm_post.h) ----------------------
def _post_input(Y, B, nu, Phi, Z, chi, sigma, X=None, eta=None, xi=None, device=0):
    """bfmmm_post_input over in-memory draws in the reference's shapes; returns (struct, arrays to keep alive)."""
    n = len(Y)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for v in Y])
    y = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in Y]))
    Bm = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64) for b in B], axis=0))
    K, P, T = nu.shape
    M = chi.shape[1]
    keep = [off, y, Bm]

    def fa(x):
        a = np.asfortranarray(x, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(c_double_p)

    inp = PostInput()
    inp.n, inp.K, inp.P, inp.M, inp.T, inp.device = n, K, P, M, T, device
    inp.offsets, inp.y, inp.B = off.ctypes.data_as(c_int64_p), y.ctypes.data_as(c_double_p), Bm.ctypes.data_as(c_double_p)
    inp.nu, inp.Phi, inp.Z, inp.chi, inp.sigma = fa(nu), fa(Phi), fa(Z), fa(chi), fa(sigma)
    if X is not None:
        inp.X, inp.D = fa(X), np.asarray(X).shape[1]
        if eta is not None:
            inp.eta = fa(eta)
        if xi is not None:      # (P, D, M, K, T) in Fortran order is T x K cubes P x D x M
            inp.xi = fa(xi)
    return inp, keep


def post_pointwise(Y, B, nu, Phi, Z, chi, sigma, first_kept=0, X=None, eta=None, xi=None, device=0):
    """bfmmm_post_pointwise on in-memory draws in the reference's shapes: nu (K, P, T), Phi (K, P, M, T), Z (n, K, T),
    chi (n, M, T), sigma (T,), eta (P, D, K, T), xi (P, D, M, K, T).  Returns (llik (T,), mean_pdf, mean_fit) with the
    per-observation arrays as lists shaped like Y."""
    lib = _lib_entry()
    inp, keep = _post_input(Y, B, nu, Phi, Z, chi, sigma, X, eta, xi, device)
    off, y = keep[0], keep[1]
    n, T = len(Y), nu.shape[2]
    ll, pdf, fit = np.zeros(T), np.zeros(len(y)), np.zeros(len(y))
    _check(lib.bfmmm_post_pointwise(C.byref(inp), int(first_kept), ll.ctypes.data_as(c_double_p), pdf.ctypes.data_as(c_double_p),
                                    fit.ctypes.data_as(c_double_p)))
    split = lambda v: [v[off[i]:off[i + 1]].copy() for i in range(n)]
    return ll, split(pdf), split(fit)


class _PostArgs:
    def __init__(self, dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj, device=0):
        lib = _lib_entry()
        self.a = PostArgs()
        lib.bfmmm_post_defaults(C.byref(self.a))
        n = len(Y)
        self.off = np.zeros(n + 1, dtype=np.int64)
        self.off[1:] = np.cumsum([len(v) for v in Y])
        self.y = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in Y]))
        self.t = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in time]))
        self.bk = np.ascontiguousarray(boundary_knots, dtype=np.float64)
        self.ik = np.ascontiguousarray(internal_knots, dtype=np.float64)
        self.dir = str(dir).encode()
        a = self.a
        a.dir, a.n_files, a.basis_degree, a.n_internal_knots = self.dir, n_files, basis_degree, len(self.ik)
        a.boundary_knots, a.internal_knots = self.bk.ctypes.data_as(c_double_p), self.ik.ctypes.data_as(c_double_p)
        a.n_funct, a.t, a.y, a.offsets = n, self.t.ctypes.data_as(c_double_p), self.y.ctypes.data_as(c_double_p), self.off.ctypes.data_as(c_int64_p)
        if burnin_prop is not None:
            a.burnin_prop = burnin_prop
        if X is not None:
            self.X = np.asfortranarray(X, dtype=np.float64)
            a.X, a.D = self.X.ctypes.data_as(c_double_p), self.X.shape[1]
        a.cov_adj, a.device = int(bool(cov_adj)), device


def FLLik(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, X=None, cov_adj=False):
    """src/PostProcessing.cpp:4892: the log-likelihood of every saved draw."""
    lib = _lib_entry()
    args = _PostArgs(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, None, X, cov_adj)
    res = C.c_void_p()
    _check(lib.bfmmm_FLLik(C.byref(args.a), C.byref(res)))
    try:
        return _result_to_dict(lib, res, None, 0)["value"]
    finally:
        lib.bfmmm_result_free(res)


def FSamplePaths(dir, n_files, basis_degree, boundary_knots, internal_knots, time, alpha=0.05, burnin_prop=0.1, simultaneous=False,
                 X=None, cov_adj=False, seed=1):
    """src/PostProcessing.cpp:6599: posterior-predictive sample paths.  Returns lists over the curves: CI_Upper / CI_50 /
    CI_Lower (vectors of n_i), Path_trace / Mean_only_Path_trace (kept x n_i matrices).  `seed`: the keyed generator of the
    predictive noise (the reference draws it from R's stream)."""
    lib = _lib_entry()
    args = _PostArgs(dir, n_files, basis_degree, boundary_knots, internal_knots, time, [np.zeros(len(v)) for v in time],
                     burnin_prop, X, cov_adj)
    res = C.c_void_p()
    _check(lib.bfmmm_FSamplePaths(C.byref(args.a), float(alpha), int(bool(simultaneous)), int(seed), C.byref(res)))
    try:
        d = _result_to_dict(lib, res, None, 0)
    finally:
        lib.bfmmm_result_free(res)
    off = args.off
    out = {}
    for nm in ("CI_Upper", "CI_50", "CI_Lower"):
        v = d[nm].reshape(-1)
        out[nm] = [v[off[i]:off[i + 1]].copy() for i in range(len(off) - 1)]
    for nm in ("Path_trace", "Mean_only_Path_trace"):
        m = d[nm]
        out[nm] = [m[:, off[i]:off[i + 1]].copy() for i in range(len(off) - 1)]
    return out


def _post_scalar(name, dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj):
    lib = _lib_entry()
    args = _PostArgs(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj)
    out = C.c_double()
    _check(getattr(lib, name)(C.byref(args.a), C.cast(C.byref(out), c_double_p)))
    return out.value


def FDIC(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """src/PostProcessing.cpp:3660."""
    return _post_scalar("bfmmm_FDIC", dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj)


def FAIC(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """src/PostProcessing.cpp:4041."""
    return _post_scalar("bfmmm_FAIC", dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj)


def FBIC(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """src/PostProcessing.cpp:4458."""
    return _post_scalar("bfmmm_FBIC", dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj)


class _PostArgsMV:
    def __init__(self, dir, n_files, Y, burnin_prop, X, cov_adj, device=0):
        lib = _lib_entry()
        self.a = PostArgs()
        lib.bfmmm_post_defaults(C.byref(self.a))
        self.Y = np.asfortranarray(Y, dtype=np.float64)
        self.dir = str(dir).encode()
        a = self.a
        a.dir, a.n_files, a.n_funct, a.P = self.dir, n_files, self.Y.shape[0], self.Y.shape[1]
        a.y = self.Y.ctypes.data_as(c_double_p)
        if burnin_prop is not None:
            a.burnin_prop = burnin_prop
        if X is not None:
            self.X = np.asfortranarray(X, dtype=np.float64)
            a.X, a.D = self.X.ctypes.data_as(c_double_p), self.X.shape[1]
        a.cov_adj, a.device = int(bool(cov_adj)), device


def MVLLik(dir, n_files, Y, X=None, cov_adj=False):
    """src/PostProcessing.cpp:6099."""
    lib = _lib_entry()
    args = _PostArgsMV(dir, n_files, Y, None, X, cov_adj)
    res = C.c_void_p()
    _check(lib.bfmmm_MVLLik(C.byref(args.a), C.byref(res)))
    try:
        return _result_to_dict(lib, res, None, 0)["value"]
    finally:
        lib.bfmmm_result_free(res)


def _post_scalar_mv(name, dir, n_files, Y, burnin_prop, X, cov_adj):
    lib = _lib_entry()
    args = _PostArgsMV(dir, n_files, Y, burnin_prop, X, cov_adj)
    out = C.c_double()
    _check(getattr(lib, name)(C.byref(args.a), C.cast(C.byref(out), c_double_p)))
    return out.value


def MVDIC(dir, n_files, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """src/PostProcessing.cpp:5789."""
    return _post_scalar_mv("bfmmm_MVDIC", dir, n_files, Y, burnin_prop, X, cov_adj)


def MVAIC(dir, n_files, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """src/PostProcessing.cpp:5116."""
    return _post_scalar_mv("bfmmm_MVAIC", dir, n_files, Y, burnin_prop, X, cov_adj)


def MVBIC(dir, n_files, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """src/PostProcessing.cpp:5452."""
    return _post_scalar_mv("bfmmm_MVBIC", dir, n_files, Y, burnin_prop, X, cov_adj)


def ConditionalPredictiveOrdinates(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop=0.1, X=None,
                                   cov_adj=False, log_CPO=True):
    """src/PostProcessing.cpp:6339: (log) conditional predictive ordinate of every curve."""
    lib = _lib_entry()
    args = _PostArgs(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj)
    res = C.c_void_p()
    _check(lib.bfmmm_ConditionalPredictiveOrdinates(C.byref(args.a), int(bool(log_CPO)), C.byref(res)))
    try:
        return _result_to_dict(lib, res, None, 0)["value"]
    finally:
        lib.bfmmm_result_free(res)


# ---- PSIS-LOO and WAIC over curves (include/bfmmm_post.h) ------------------------------------------------
_LOO_SCALARS = ("elpd_loo", "se_elpd_loo", "p_loo", "se_p_loo", "looic", "se_looic", "elpd_waic", "se_elpd_waic", "p_waic",
                "se_p_waic", "waic", "se_waic", "khat_threshold", "n_khat_above")


def _loo_dict(d):
    out = {k: float(np.asarray(d[k]).reshape(-1)[0]) for k in _LOO_SCALARS}
    out["n_khat_above"] = int(out["n_khat_above"])
    for k in ("pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "lppd", "pointwise_elpd_waic", "pointwise_p_waic"):
        out[k] = np.asarray(d[k]).reshape(-1)
    return out


def _loo_call(fn, args):
    lib = _lib_entry()
    res = C.c_void_p()
    _check(fn(C.byref(args.a), C.byref(res)))
    try:
        return _loo_dict(_result_to_dict(lib, res, None, 0))
    finally:
        lib.bfmmm_result_free(res)


def FLOO(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """PSIS-LOO and WAIC over curves (leave one curve out, scores integrated out) on the draws t >= floor(burnin_prop T),
    the ones ConditionalPredictiveOrdinates uses; relative efficiency 1.  Returns a dict: the totals and their standard
    errors (floats), the number of curves with Pareto k above the threshold (int), the per-curve arrays."""
    args = _PostArgs(dir, n_files, basis_degree, boundary_knots, internal_knots, time, Y, burnin_prop, X, cov_adj)
    return _loo_call(_lib_entry().bfmmm_FLOO, args)


def MVLOO(dir, n_files, Y, burnin_prop=0.1, X=None, cov_adj=False):
    """FLOO for the multivariate model (the arguments of MVDIC); the log-density carries the full (P / 2) log 2 pi."""
    args = _PostArgsMV(dir, n_files, Y, burnin_prop, X, cov_adj)
    return _loo_call(_lib_entry().bfmmm_MVLOO, args)


def post_curve_loglik(Y, B, nu, Phi, Z, chi, sigma, first_kept=0, X=None, eta=None, xi=None, device=0):
    """bfmmm_post_curve_loglik on in-memory draws (the shapes of post_pointwise): the marginal log-density of every curve
    under every draw t >= first_kept, scores integrated out, as an (n, kept) array (row i = curve i; its memory is R's
    S x N column-major log_lik)."""
    lib = _lib_entry()
    inp, keep = _post_input(Y, B, nu, Phi, Z, chi, sigma, X, eta, xi, device)
    n, T = len(Y), nu.shape[2]
    out = np.zeros((n, T - int(first_kept)))
    _check(lib.bfmmm_post_curve_loglik(C.byref(inp), int(first_kept), out.ctypes.data_as(c_double_p)))
    return out


def _total_se(v):
    """sum in curve order and sqrt(n var_{n-1}) (NaN for one curve)"""
    s = 0.0
    for x in v:
        s += float(x)
    n = len(v)
    if n < 2:
        return s, float("nan")
    mean = s / n
    q = 0.0
    for x in v:
        q += (float(x) - mean) ** 2
    return s, float(np.sqrt(n * (q / (n - 1))))


def loo_totals(pointwise, S):
    """the totals of per-curve PSIS / WAIC values (keys as FLOO returns them) for S draws per curve"""
    e_loo, se_loo = _total_se(pointwise["pointwise_elpd_loo"])
    p_loo, se_ploo = _total_se(pointwise["pointwise_p_loo"])
    e_waic, se_ewaic = _total_se(pointwise["pointwise_elpd_waic"])
    p_waic, se_pwaic = _total_se(pointwise["pointwise_p_waic"])
    with np.errstate(divide="ignore"):
        thr = float(min(1.0 - 1.0 / np.log10(float(S)), 0.7))
    out = dict(elpd_loo=e_loo, se_elpd_loo=se_loo, p_loo=p_loo, se_p_loo=se_ploo, looic=-2 * e_loo, se_looic=2 * se_loo,
               elpd_waic=e_waic, se_elpd_waic=se_ewaic, p_waic=p_waic, se_p_waic=se_pwaic, waic=-2 * e_waic, se_waic=2 * se_ewaic,
               khat_threshold=thr, n_khat_above=int(np.sum(np.asarray(pointwise["pareto_k"]) > thr)))
    out.update(pointwise)
    return out


def psis_loo(ll, device=0):
    """PSIS-LOO and WAIC (relative efficiency 1) of any n x S pointwise log-likelihood matrix (row = unit left out,
    column = draw) on the device; the dict FLOO returns."""
    lib = _lib_entry()
    m = np.ascontiguousarray(ll, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError("'ll' must be an n x S matrix")
    n, S = m.shape
    outs = [np.zeros(n) for _ in range(6)]
    _check(lib.bfmmm_post_psis(m.ctypes.data_as(c_double_p), n, S, device, *[o.ctypes.data_as(c_double_p) for o in outs]))
    pw = dict(zip(("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic"), outs))
    return loo_totals(pw, S)


def psis_expect(ll, h, device=0):
    """`psis_loo(ll)`, bit for bit, and "expect": the expectation of every auxiliary matrix of h -- (n, S), or (n_aux, n, S) -- under
    each row's Pareto-smoothed weights, sum_t w_it h[a, i, t] / sum_t w_it, of shape h.shape[:-1] (bfmmm_post_psis_expect; DESIGN.md
    7q).  With h = exp(ll) the logarithm of "expect" is "pointwise_elpd_loo"."""
    lib = _lib_entry()
    m = np.ascontiguousarray(ll, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError("'ll' must be an n x S matrix")
    n, S = m.shape
    hm = np.ascontiguousarray(h, dtype=np.float64)
    if hm.ndim not in (2, 3) or hm.shape[-2:] != (n, S) or hm.shape[0] < 1:
        raise ValueError("'h' must be an n x S matrix, or n_aux of them, of the shape of 'll'")
    n_aux = 1 if hm.ndim == 2 else hm.shape[0]
    outs = [np.zeros(n) for _ in range(6)]
    expect = np.zeros((n_aux, n))
    _check(lib.bfmmm_post_psis_expect(m.ctypes.data_as(c_double_p), hm.ctypes.data_as(c_double_p), n, S, n_aux, device,
                                      *[o.ctypes.data_as(c_double_p) for o in outs], expect.ctypes.data_as(c_double_p)))
    pw = dict(zip(("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic"), outs))
    out = loo_totals(pw, S)
    out["expect"] = expect[0] if hm.ndim == 2 else expect
    return out


# ---- stacking of predictive distributions (include/bfmmm_post.h) ------------------------------------------
def stacking_geometry():
    """(threads, max_workgroups) of the stacking iteration: one grid-stride pass covers threads * max_workgroups units"""
    t, g = C.c_int32(0), C.c_int32(0)
    _lib_entry().bfmmm_post_stacking_geometry(C.byref(t), C.byref(g))
    return t.value, g.value


def stacking(lpd, init=None, max_iter=10000, check_every=16, tol=1e-8, device=0):
    """Stacking weights (Yao et al. 2018) of the Q candidates -- models, or chains (Yao et al. 2022) -- whose leave-one-out log
    predictive densities are the columns of the (n, Q) matrix `lpd`: the simplex weights that maximise the LOO log score of the
    mixture, sum_i log sum_q w_q exp(lpd[i, q]), by the EM fixed point on the device (bfmmm_post_stacking).  -inf is
    allowed; NaN, +inf and a unit that is -inf under every candidate are refused.  The loop stops at the first iterate, at a
    multiple of check_every, whose certificate "gap" is at most tol: the stacked elpd is then within n * gap nats of the optimum.
    tol=0 runs max_iter iterations.  `init`: Q positive weights that add to 1 (None: uniform).
    Returns "weights": (Q,), "pointwise": (n,) the stacked log density of every unit, "elpd" and "se_elpd": its total and standard
    error, "objective" (the total, as the device adds it), "gap", "n_iter" and "converged"."""
    lib = _lib_entry()
    m = np.asarray(lpd, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("'lpd' must be an n x Q matrix, units by candidates")
    n, Q = m.shape
    cm = np.ascontiguousarray(m.T)                      # candidate-major
    w0 = None
    if init is not None:
        w0 = np.ascontiguousarray(init, dtype=np.float64).reshape(-1)
        if w0.size != Q:
            raise ValueError(f"'init' must have {Q} entries, one per candidate")
    weights, pointwise = np.zeros(Q), np.zeros(n)
    obj, gap = C.c_double(0.0), C.c_double(0.0)
    n_iter, conv = C.c_int(0), C.c_int(0)
    _check(lib.bfmmm_post_stacking(cm.ctypes.data_as(c_double_p), n, Q, device, None if w0 is None else w0.ctypes.data_as(c_double_p),
                                   int(max_iter), int(check_every), float(tol), weights.ctypes.data_as(c_double_p),
                                   pointwise.ctypes.data_as(c_double_p), C.byref(obj), C.byref(gap), C.byref(n_iter), C.byref(conv)))
    elpd, se = _total_se(pointwise)
    return dict(weights=weights, pointwise=pointwise, elpd=elpd, se_elpd=se, objective=obj.value, gap=gap.value,
                n_iter=n_iter.value, converged=bool(conv.value))


def compare_table(L):
    """the comparison of the Q columns of the (n, Q) pointwise elpd matrix L, host arithmetic in unit order: "elpd" and "se" (Q,),
    "best" (the largest elpd, the first of equals), "elpd_diff" and "se_diff" against it from the paired differences over units,
    sqrt(n var_{n-1}(L[:, q] - L[:, best])) (0 and 0 for the best), and "pseudo_bma", the softmax of the totals"""
    n, Q = L.shape
    tot = [_total_se(L[:, q]) for q in range(Q)]
    elpd = np.array([t[0] for t in tot])
    best = int(np.argmax(elpd))
    diff = [(0.0, 0.0) if q == best else _total_se(L[:, q] - L[:, best]) for q in range(Q)]
    e = np.exp(elpd - elpd[best])
    return dict(elpd=elpd, se=np.array([t[1] for t in tot]), best=best, elpd_diff=np.array([d[0] for d in diff]),
                se_diff=np.array([d[1] for d in diff]), pseudo_bma=e / e.sum())


def stack_models(results, names=None, **kw):
    """Compares and stacks Q fits of the same data.  `results`: one entry per fit, the dict of loo_pointwise, loo_blocks, loo,
    loo_marginal or psis_loo (its "pointwise_elpd_loo" is read) or a plain (n,) array of log predictive densities, such as the "lpd"
    of `predict` over the folds of a K-fold split; all of one length.  Returns the dict of `stacking` (keywords go to it) and the
    compare table: "elpd", "se", "elpd_diff", "se_diff", "pseudo_bma": (Q,), "best" and "names" (default "model0", ...).  "elpd" is
    the candidates' here; the stacked total is "objective", its standard error "se_elpd".  Prefer "weights" to "pseudo_bma" and to
    picking "best" (Yao et al. 2018)."""
    cols = [np.asarray(r["pointwise_elpd_loo"] if isinstance(r, dict) else r, dtype=np.float64).reshape(-1) for r in results]
    if not cols:
        raise ValueError("stack_models: 'results' is empty")
    if any(c.size != cols[0].size for c in cols):
        raise ValueError(f"stack_models: the entries of 'results' must cover the same units, got lengths {[c.size for c in cols]}")
    names = [f"model{q}" for q in range(len(cols))] if names is None else list(names)
    if len(names) != len(cols):
        raise ValueError(f"stack_models: 'names' must have {len(cols)} entries")
    L = np.stack(cols, axis=1)
    out = stacking(L, **kw)
    out.update(compare_table(L))
    out["names"] = names
    return out


# ---- convergence diagnostics (include/bfmmm_post.h) -----------------------------------------------------
DIAG_STATS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")


def diagnostics(draws, device=0):
    """Split R-hat (rank-normalised, bulk and folded), bulk / tail ESS, ESS and MCSE of the mean, mean and sd of draws of
    shape (S, C) or (S, C, *shape) -- S draws of C chains -- on the device.  Returns a dict of the seven statistics, each of
    shape `shape`."""
    lib = _lib_entry()
    d = np.asarray(draws, dtype=np.float64)
    if d.ndim < 2:
        raise ValueError("'draws' must be (S, C) or (S, C, *shape)")
    S, C = d.shape[:2]
    shape = d.shape[2:]
    n_param = int(np.prod(shape, dtype=np.int64))
    rows = np.ascontiguousarray(d.reshape(S, C, n_param).transpose(2, 1, 0))      # x[s + S (c + C p)]
    outs = [np.zeros(n_param) for _ in DIAG_STATS]
    _check(lib.bfmmm_post_diagnostics(rows.ctypes.data_as(c_double_p), n_param, C, S, device,
                                      *[o.ctypes.data_as(c_double_p) for o in outs]))
    return {k: o.reshape(shape) for k, o in zip(DIAG_STATS, outs)}


# ---- credible intervals (src/PostProcessing.cpp:99, :3435, :3505) -------------------------------------------------------
def _ci_call(fn, a, keep):
    lib = _lib_entry()
    res = C.c_void_p()
    _check(fn(C.byref(a), C.byref(res)))
    try:
        return _result_to_dict(lib, res, None, 0)
    finally:
        lib.bfmmm_result_free(res)


def _ci_args(dir, n_files, alpha, burnin_prop):
    lib = _lib_entry()
    a = CiArgs()
    lib.bfmmm_ci_defaults(C.byref(a))
    keep = [str(dir).encode()]
    a.dir, a.n_files, a.alpha, a.burnin_prop = keep[0], n_files, alpha, burnin_prop
    return a, keep


def SigmaCI(dir, n_files, alpha=0.05, burnin_prop=0.1):
    """src/PostProcessing.cpp:3435 (CI_Lower is the median, as in the reference)."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    d = _ci_call(_lib_entry().bfmmm_SigmaCI, a, keep)
    return {k: float(v.reshape(-1)[0]) for k, v in d.items()}


def ZCI(dir, n_files, alpha=0.05, rescale=True, burnin_prop=0.1):
    """src/PostProcessing.cpp:3505."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    a.rescale = int(bool(rescale))
    return _ci_call(_lib_entry().bfmmm_ZCI, a, keep)


def FMeanCI(dir, n_files, time, basis_degree, boundary_knots, internal_knots, k, alpha=0.05, rescale=True, simultaneous=False,
            burnin_prop=0.1, X=None, trans_mats=None):
    """src/PostProcessing.cpp:99."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    t = np.ascontiguousarray(time, dtype=np.float64).reshape(-1)
    bk = np.ascontiguousarray(boundary_knots, dtype=np.float64)
    ik = np.ascontiguousarray(internal_knots, dtype=np.float64)
    keep += [t, bk, ik]
    a.time, a.n_time, a.basis_degree, a.n_internal_knots = t.ctypes.data_as(c_double_p), len(t), basis_degree, len(ik)
    a.boundary_knots, a.internal_knots = bk.ctypes.data_as(c_double_p), ik.ctypes.data_as(c_double_p)
    a.k, a.rescale, a.simultaneous = k, int(bool(rescale)), int(bool(simultaneous))
    if X is not None:
        Xf = np.asfortranarray(X, dtype=np.float64)
        keep.append(Xf)
        a.X, a.n_x, a.D = Xf.ctypes.data_as(c_double_p), Xf.shape[0], Xf.shape[1]
    if trans_mats is not None:
        tm = np.asfortranarray(trans_mats, dtype=np.float64)
        keep.append(tm)
        a.trans_mats = tm.ctypes.data_as(c_double_p)
    d = _ci_call(_lib_entry().bfmmm_FMeanCI, a, keep)
    if X is None:
        for nm in ("CI_Upper", "CI_50", "CI_Lower"):
            d[nm] = d[nm].reshape(-1)
    return d


def _cov_x(a, keep, X):
    if X is not None:
        Xf = np.asfortranarray(X, dtype=np.float64)
        keep.append(Xf)
        a.X, a.n_x, a.D = Xf.ctypes.data_as(c_double_p), Xf.shape[0], Xf.shape[1]


def FCovCI(dir, n_files, time1, time2, basis_degree, boundary_knots, internal_knots, l, m, alpha=0.05, rescale=True,
           simultaneous=False, burnin_prop=0.1, X=None, trans_mats=None):
    """src/PostProcessing.cpp:1781.  With X (n_x covariate settings: the covariate-dependent covariance) the bands are
    (n_time1, n_time2, n_x) and cov_trace (n_time1, n_time2, kept, n_x) -- the reference's list of n_x cubes."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    t1 = np.ascontiguousarray(time1, dtype=np.float64).reshape(-1)
    t2 = np.ascontiguousarray(time2, dtype=np.float64).reshape(-1)
    bk = np.ascontiguousarray(boundary_knots, dtype=np.float64)
    ik = np.ascontiguousarray(internal_knots, dtype=np.float64)
    keep += [t1, t2, bk, ik]
    a.time, a.n_time, a.time2, a.n_time2 = t1.ctypes.data_as(c_double_p), len(t1), t2.ctypes.data_as(c_double_p), len(t2)
    a.basis_degree, a.n_internal_knots = basis_degree, len(ik)
    a.boundary_knots, a.internal_knots = bk.ctypes.data_as(c_double_p), ik.ctypes.data_as(c_double_p)
    a.l, a.m, a.rescale, a.simultaneous = l, m, int(bool(rescale)), int(bool(simultaneous))
    _cov_x(a, keep, X)
    if trans_mats is not None:
        tm = np.asfortranarray(trans_mats, dtype=np.float64)
        keep.append(tm)
        a.trans_mats = tm.ctypes.data_as(c_double_p)
    return _ci_call(_lib_entry().bfmmm_FCovCI, a, keep)


def HDFCovCI(dir, n_files, time1, time2, basis_degree, boundary_knots, internal_knots, l, m, alpha=0.05, rescale=True,
             simultaneous=False, burnin_prop=0.1, X=None):
    """src/PostProcessing.cpp:2468: `time1`, `time2` n x dim matrices, `basis_degree` a vector, `boundary_knots` dim x 2,
    `internal_knots` a list.  (The reference evaluates both bases at time1: the surface is time1 x time1.)"""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    dim = len(basis_degree)
    t1 = np.asfortranarray(np.asarray(time1, dtype=np.float64).reshape(-1, dim))
    t2 = np.asfortranarray(np.asarray(time2, dtype=np.float64).reshape(-1, dim))
    bk = np.ascontiguousarray(np.asarray(boundary_knots, dtype=np.float64).reshape(dim, 2))
    ik = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in internal_knots]))
    deg = (C.c_int32 * dim)(*[int(x) for x in basis_degree])
    nint = (C.c_int32 * dim)(*[len(v) for v in internal_knots])
    keep += [t1, t2, bk, ik, deg, nint]
    a.time, a.n_time, a.time2, a.n_time2 = t1.ctypes.data_as(c_double_p), t1.shape[0], t2.ctypes.data_as(c_double_p), t2.shape[0]
    a.dim, a.basis_degree_hd, a.n_internal_hd = dim, deg, nint
    a.boundary_knots, a.internal_knots = bk.ctypes.data_as(c_double_p), ik.ctypes.data_as(c_double_p)
    a.l, a.m, a.rescale, a.simultaneous = l, m, int(bool(rescale)), int(bool(simultaneous))
    _cov_x(a, keep, X)
    return _ci_call(_lib_entry().bfmmm_HDFCovCI, a, keep)


def MVCovCI(dir, n_files, l, m, alpha=0.05, rescale=True, burnin_prop=0.1, X=None):
    """src/PostProcessing.cpp:3097 (multivariate model: P x P bands, pointwise)."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    a.l, a.m, a.rescale = l, m, int(bool(rescale))
    _cov_x(a, keep, X)
    return _ci_call(_lib_entry().bfmmm_MVCovCI, a, keep)


def MVMeanCI(dir, n_files, alpha=0.05, rescale=True, burnin_prop=0.1, X=None):
    """src/PostProcessing.cpp:1410.  With X the mean_trace is returned as (K, P, kept, n_x)."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    a.rescale = int(bool(rescale))
    if X is not None:
        Xf = np.asfortranarray(X, dtype=np.float64)
        keep.append(Xf)
        a.X, a.n_x, a.D = Xf.ctypes.data_as(c_double_p), Xf.shape[0], Xf.shape[1]
    d = _ci_call(_lib_entry().bfmmm_MVMeanCI, a, keep)
    if X is not None:
        K, P, tot = d["mean_trace"].shape
        d["mean_trace"] = d["mean_trace"].reshape((K, P, tot // Xf.shape[0], Xf.shape[0]), order="F")
    return d


def HDFMeanCI(dir, n_files, time, basis_degree, boundary_knots, internal_knots, k, alpha=0.05, rescale=True, simultaneous=False,
              burnin_prop=0.1, X=None, trans_mats=None):
    """src/PostProcessing.cpp:806: `time` n_time x dim, `basis_degree` a vector, `boundary_knots` dim x 2, `internal_knots` a list."""
    a, keep = _ci_args(dir, n_files, alpha, burnin_prop)
    dim = len(basis_degree)
    t = np.asfortranarray(np.asarray(time, dtype=np.float64).reshape(-1, dim))
    bk = np.ascontiguousarray(np.asarray(boundary_knots, dtype=np.float64).reshape(dim, 2))
    ik = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in internal_knots]))
    deg = (C.c_int32 * dim)(*[int(x) for x in basis_degree])
    nint = (C.c_int32 * dim)(*[len(v) for v in internal_knots])
    keep += [t, bk, ik, deg, nint]
    a.time, a.n_time, a.dim, a.basis_degree_hd, a.n_internal_hd = t.ctypes.data_as(c_double_p), t.shape[0], dim, deg, nint
    a.boundary_knots, a.internal_knots = bk.ctypes.data_as(c_double_p), ik.ctypes.data_as(c_double_p)
    a.k, a.rescale, a.simultaneous = k, int(bool(rescale)), int(bool(simultaneous))
    if X is not None:
        Xf = np.asfortranarray(X, dtype=np.float64)
        keep.append(Xf)
        a.X, a.n_x, a.D = Xf.ctypes.data_as(c_double_p), Xf.shape[0], Xf.shape[1]
    if trans_mats is not None:
        tm = np.asfortranarray(trans_mats, dtype=np.float64)
        keep.append(tm)
        a.trans_mats = tm.ctypes.data_as(c_double_p)
    d = _ci_call(_lib_entry().bfmmm_HDFMeanCI, a, keep)
    if X is None:
        for nm in ("CI_Upper", "CI_50", "CI_Lower"):
            d[nm] = d[nm].reshape(-1)
    return d
