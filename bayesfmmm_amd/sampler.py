"""Thin object wrapper over the C ABI (include/bfmmm.h): one `Sampler` = one `bfmmm_handle`.

All arrays cross the boundary in the reference's layouts (column-major, R/Armadillo order);
numpy arrays returned here are Fortran-ordered with the reference's shapes.
"""
import ctypes as C
import functools
import inspect

import numpy as np

from . import _lib

U_Z, U_PI, U_ALPHA3, U_PHI, U_DELTA, U_A, U_GAMMA, U_NU, U_TAU, U_SIGMA, U_CHI = (1 << i for i in range(11))
U_ETA, U_TAU_ETA, U_XI, U_DELTA_XI, U_A_XI, U_GAMMA_XI = (1 << i for i in range(11, 17))
U_LOGLIK = 1 << 17
COV_MEAN = U_ETA | U_TAU_ETA
COV_XI = U_XI | U_DELTA_XI | U_A_XI | U_GAMMA_XI
SWEEP_NU_Z = U_Z | U_PI | U_ALPHA3 | U_NU | U_TAU | U_SIGMA | U_LOGLIK
SWEEP_THETA = U_PHI | U_DELTA | U_A | U_GAMMA | U_TAU | U_SIGMA | U_CHI | U_LOGLIK
SWEEP_WARM = SWEEP_NU_Z | SWEEP_THETA

MODEL_FUNCTIONAL, MODEL_MULTIVARIATE = 0, 1

# One draw of every array of the model in the reference's shape: a letter per dimension, n, K, P, M, D of the sampler or 2.
DRAW_DIMS = {"nu": "KP", "Phi": "KPM", "chi": "nM", "Z": "nK", "pi": "K", "alpha_3": "", "delta": "KM", "A": "K2", "gamma": "KPM",
             "tau": "K", "sigma_sq": "", "loglik": "", "eta": "PDK", "xi": "PDMK", "gamma_xi": "PDMK", "tau_eta": "KD",
             "delta_xi": "KMD", "A_xi": "K2D"}
# what get_state also answers: diagnostic vectors of fixed length
STATE_ONLY = {"status": (1,), "stamps": (64,), "wgtrace": (3072,), "ztrace": (3 * 8192,), "zphase": (8 * 8192,), "fct": (8,)}
STAT_NAMES = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")
# the six arrays every PSIS call fills first, by their names in the dict of api.psis_loo
_PW_NAMES = ("lppd", "pointwise_elpd_loo", "pointwise_p_loo", "pareto_k", "pointwise_elpd_waic", "pointwise_p_waic")


def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _loo_dict(outs, draws):
    """the dict of api.psis_loo from the six pointwise arrays in front of outs, `draws` draws a row"""
    from . import api
    return api.loo_totals(dict(zip(_PW_NAMES, outs[:6])), draws)


def _opt(tr):
    """k -> the array tr[k] as a pointer, None where it was not asked for"""
    return lambda k: None if tr.get(k) is None else _dp(tr[k])


def _proposal_option(laplace, refused):
    """Gives a method the keyword-only option proposal="dirichlet" | "laplace" (DESIGN.md 7p).  "dirichlet", the default, calls the
    method as it is, with its own parameters and defaults, which are what inspect.signature shows.  "laplace" calls the method named
    `laplace` with the same arguments, once every parameter of refused = {name: test} that the caller gave, and whose value the test
    marks as without meaning there, has been refused by name: a wrapper sees which arguments were given, where the method itself
    could not tell a given refine=True from its default."""
    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(self, *args, proposal="dirichlet", **kw):
            if proposal == "dirichlet":
                return fn(self, *args, **kw)
            if proposal != "laplace":
                raise ValueError(f"{fn.__name__}: proposal must be 'dirichlet' or 'laplace', got {proposal!r}")
            b = sig.bind(self, *args, **kw)
            for name, without_meaning in refused.items():
                if name in b.arguments and without_meaning(b.arguments[name]):
                    raise ValueError(f"{fn.__name__}: '{name}' has no meaning with proposal='laplace' (one round, no sample table, no "
                                     f"refinement): leave it at its default")
            b.apply_defaults()
            return getattr(self, laplace)(**{k: v for k, v in b.arguments.items() if k != "self" and k not in refused})
        return call
    return deco


def _rescale_option(rescaled, with_x=False):
    """Gives a method that takes `perm` the keyword-only option rescale=None.  None, the default, calls the method as it
    is, with its own parameters and defaults, which are what inspect.signature shows.  With the dict `Sampler.rescale` returned for the
    same slots it calls the method named `rescaled` with the same arguments; perm may then be left out or None, and where it is given it
    must be the dict's.  with_x: the method also gains the keyword-only x=None, one covariate setting, honoured only with rescale and
    refused without it."""
    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(self, *args, rescale=None, **kw):
            if with_x and rescale is None and kw.get("x") is not None:
                raise ValueError(f"{fn.__name__}: 'x' is honoured only with rescale=: without it this is the mean function at x = 0")
            extra = {"x": kw.pop("x", None)} if with_x else {}
            if rescale is None:
                return fn(self, *args, **kw)
            b = sig.bind_partial(self, *args, **kw)
            b.apply_defaults()
            given = {k: v for k, v in b.arguments.items() if k != "self"}
            given.setdefault("perm", None)
            return getattr(self, rescaled)(rescale=rescale, **given, **extra)
        return call
    return deco


def _probs_arg(probs):
    return np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)


BLOCK_MAX = 64      # the most observations of a block of loo_blocks: a row tile of k_loo_blocks


def block_plan(ni, blocks=None, block_size=None, horizon=None, curves=None):
    """The flat block lists of Sampler.loo_blocks (bfmmm_chain_loo_blocks) from one of its three spellings, ni the observation
    counts of the curves: blocks, a sequence of (curve, indices within the curve) pairs; block_size=s, every selected curve cut
    into consecutive blocks of s observations (the last one shorter); horizon=h, one block a selected curve, its last h
    observations, which needs n_i > h.  curves (None: all, in order; repeats allowed) selects for the latter two.  Returns
    (block_curve int32 (n_blocks,), block_offsets int64 (n_blocks + 1,), block_obs int32 (N_rows,)) in the order of the result.
    ValueError: not exactly one spelling, curves with blocks, a curve or an index out of range, an empty block or one above
    BLOCK_MAX observations, an index repeated within a block, a curve too short for the horizon."""
    ni = np.asarray(ni, dtype=np.int64)
    n = len(ni)
    if sum(v is not None for v in (blocks, block_size, horizon)) != 1:
        raise ValueError("loo_blocks: exactly one of 'blocks', 'block_size' and 'horizon' must be given")
    pairs = []
    if blocks is not None:
        if curves is not None:
            raise ValueError("loo_blocks: 'curves' goes with 'block_size' or 'horizon', not with 'blocks'")
        for k, (i, idx) in enumerate(blocks):
            pairs.append((int(i), np.array(list(idx), dtype=np.int64).reshape(-1)))
            if not 0 <= pairs[-1][0] < n:
                raise ValueError(f"loo_blocks: block {k}: curve {pairs[-1][0]} outside 0 .. {n - 1}")
    else:
        sel = np.arange(n) if curves is None else np.asarray(curves, dtype=np.int64).reshape(-1)
        if sel.size and (sel.min() < 0 or sel.max() >= n):
            raise ValueError(f"loo_blocks: 'curves' must lie in 0 .. {n - 1}")
        # generated blocks are valid by construction: the lists are built curve by curve, not block by block
        cur, sizes, obs = [], [], []
        if block_size is not None:
            s = int(block_size)
            if not 1 <= s <= BLOCK_MAX:
                raise ValueError(f"loo_blocks: 'block_size' must lie in 1 .. {BLOCK_MAX}, got {s}")
            for i in sel:
                m = int(ni[i])
                nb = -(-m // s)
                if nb:
                    sz = np.full(nb, s, dtype=np.int64)
                    sz[-1] = m - s * (nb - 1)
                    cur.append(np.full(nb, i, dtype=np.int32)); sizes.append(sz); obs.append(np.arange(m, dtype=np.int32))
        else:
            hz = int(horizon)
            if not 1 <= hz <= BLOCK_MAX:
                raise ValueError(f"loo_blocks: 'horizon' must lie in 1 .. {BLOCK_MAX}, got {hz}")
            for i in sel:
                m = int(ni[i])
                if m <= hz:
                    raise ValueError(f"loo_blocks: curve {int(i)} has {m} observations, not more than the horizon {hz}")
                cur.append(np.full(1, i, dtype=np.int32)); sizes.append(np.full(1, hz, dtype=np.int64)); obs.append(np.arange(m - hz, m, dtype=np.int32))
        if not cur:
            raise ValueError("loo_blocks: no blocks")
        block_offsets = np.zeros(sum(len(c) for c in cur) + 1, dtype=np.int64)
        block_offsets[1:] = np.cumsum(np.concatenate(sizes))
        return np.concatenate(cur), block_offsets, np.concatenate(obs)
    if not pairs:
        raise ValueError("loo_blocks: no blocks")
    for k, (i, idx) in enumerate(pairs):
        if idx.size < 1 or idx.size > BLOCK_MAX:
            raise ValueError(f"loo_blocks: block {k} has {idx.size} observations, outside 1 .. {BLOCK_MAX}")
        if idx.min() < 0 or idx.max() >= ni[i]:
            raise ValueError(f"loo_blocks: block {k}: an index outside 0 .. {int(ni[i]) - 1} of curve {i}")
        if len(np.unique(idx)) != idx.size:
            raise ValueError(f"loo_blocks: block {k} repeats an index")
    block_curve = np.array([i for i, _ in pairs], dtype=np.int32)
    block_offsets = np.zeros(len(pairs) + 1, dtype=np.int64)
    block_offsets[1:] = np.cumsum([idx.size for _, idx in pairs])
    block_obs = np.concatenate([idx for _, idx in pairs]).astype(np.int32)
    return block_curve, block_offsets, block_obs


def contrast_plan(K, D, contrasts="pairwise"):
    """The weight arrays of Sampler.cluster_contrast_bands (bfmmm_chain_cluster_contrast_bands) from one of its
    spellings, for K clusters and D covariates: "pairwise", nu_k - nu_l for all k < l in the order (0, 1), (0, 2), .., (1, 2), ..;
    "effects", eta_kd for every k and d (r = k D + d; it requires covariates); a list of contrasts, each a list of terms (weight, k)
    or (weight, k, x), where a term with a D-vector x also adds weight x_d to the eta weight of (k, d), so that [(1, k, x), (-1, k, x')]
    is f_k(x) - f_k(x'); or a dict {"nu": (R, K), "eta": (R, K, D)} taken as is (either may be left out: zeros).  Returns (w_nu
    (R, K), w_eta (R, K, D) or None where D = 0).  ValueError: an unknown spelling, "effects" or an x without covariates, no contrast,
    a term of another length, a cluster outside 0 .. K - 1, an x of another length, arrays of another shape.  Contrasts whose weights
    are all zero or not finite, and more than 64 of them, are refused by the call itself."""
    K, D = int(K), int(D)
    name = "cluster_contrast_bands"
    if isinstance(contrasts, str):
        if contrasts == "pairwise":
            pairs = [(k, l) for k in range(K) for l in range(k + 1, K)]
            w_nu = np.zeros((len(pairs), K))
            for r, (k, l) in enumerate(pairs):
                w_nu[r, k], w_nu[r, l] = 1.0, -1.0
            w_eta = np.zeros((len(pairs), K, D))
        elif contrasts == "effects":
            if D < 1:
                raise ValueError(f"{name}: contrasts='effects' requires covariates")
            w_nu = np.zeros((K * D, K))
            w_eta = np.zeros((K * D, K, D))
            for k in range(K):
                for d in range(D):
                    w_eta[k * D + d, k, d] = 1.0
        else:
            raise ValueError(f"{name}: contrasts must be 'pairwise', 'effects', a list of contrasts or a dict, got {contrasts!r}")
    elif isinstance(contrasts, dict):
        if not contrasts or any(k not in ("nu", "eta") for k in contrasts):
            raise ValueError(f"{name}: a contrasts dict has the keys 'nu' and 'eta'")
        arrs = {k: np.array(v, dtype=np.float64) for k, v in contrasts.items()}
        R = next(iter(arrs.values())).shape[0] if next(iter(arrs.values())).ndim else -1
        w_nu = arrs.get("nu", np.zeros((max(R, 0), K)))
        if w_nu.shape != (R, K):
            raise ValueError(f"{name}: contrasts['nu'] must have shape (R, {K}), got {w_nu.shape}")
        if "eta" in arrs and D < 1:
            raise ValueError(f"{name}: contrasts['eta'] is given but the sampler has no covariates")
        w_eta = arrs.get("eta", np.zeros((R, K, D)))
        if w_eta.shape != (R, K, D):
            raise ValueError(f"{name}: contrasts['eta'] must have shape ({R}, {K}, {D}), got {w_eta.shape}")
    else:
        rows = [list(c) for c in contrasts]
        w_nu = np.zeros((len(rows), K))
        w_eta = np.zeros((len(rows), K, D))
        for r, terms in enumerate(rows):
            for term in terms:
                term = tuple(term)
                if len(term) not in (2, 3):
                    raise ValueError(f"{name}: contrast {r}: a term is (weight, k) or (weight, k, x), got {len(term)} entries")
                wgt, k = float(term[0]), int(term[1])
                if not 0 <= k < K:
                    raise ValueError(f"{name}: contrast {r}: cluster {k} outside 0 .. {K - 1}")
                w_nu[r, k] += wgt
                if len(term) == 3:
                    if D < 1:
                        raise ValueError(f"{name}: contrast {r}: a term has an x but the sampler has no covariates")
                    x = np.asarray(term[2], dtype=np.float64).reshape(-1)
                    if x.size != D:
                        raise ValueError(f"{name}: contrast {r}: x must have {D} entries, one per covariate, got {x.size}")
                    w_eta[r, k] += wgt * x
    if w_nu.shape[0] < 1:
        raise ValueError(f"{name}: no contrasts")
    return np.ascontiguousarray(w_nu), (np.ascontiguousarray(w_eta) if D > 0 else None)


def default_config(**kw):
    cfg = _lib.BfmmmConfig()
    _lib.load().bfmmm_config_defaults(C.byref(cfg))
    for k, v in kw.items():
        if k == "c":
            for i, x in enumerate(v):
                cfg.c[i] = float(x)
        else:
            setattr(cfg, k, v)
    return cfg


class Sampler:
    def __init__(self, cfg, Y, time=None, internal_knots=None, boundary_knots=None, device=0, basis=None, band=None,
                 penalty=None, penalty_band=None, n_chains=1):
        """Functional model: Y, time are lists of 1-D arrays (one per curve).
        Multivariate model: Y is an (n, P) matrix.
        Functional model over a caller-supplied basis (bfmmm_create_from_basis; the high-dimensional model's tensor-product
        basis): `basis` is a list of n_i x P matrices, `band` the half-bandwidth of B'B, `penalty` the P x P penalty of the
        nu prior and `penalty_band` its half-bandwidth.
        n_chains > 1: a chain batch (bfmmm_create_batch) -- `run` advances all chains in lockstep, `select_chain` picks the
        chain the state / chain accessors address."""
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = int(device)
        self.h = C.c_void_p()
        if basis is not None:
            self.offsets = np.zeros(len(Y) + 1, dtype=np.int64)
            self.offsets[1:] = np.cumsum([len(y) for y in Y])
            y = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in Y]))
            B = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64) for b in basis], axis=0))
            Pm = np.asfortranarray(penalty, dtype=np.float64)
            cfg.n_funct = len(Y)
            self.P = B.shape[1]
            _lib.check(self.lib.bfmmm_create_from_basis_batch(C.byref(cfg), device, _dp(y), _dp(B),
                                                              self.offsets.ctypes.data_as(_lib.c_int64_p), self.P, int(band),
                                                              _dp(Pm), int(penalty_band), int(n_chains), C.byref(self.h)))
        elif cfg.model == MODEL_FUNCTIONAL:
            self.offsets = np.zeros(len(Y) + 1, dtype=np.int64)
            self.offsets[1:] = np.cumsum([len(y) for y in Y])
            y = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in Y]))
            t = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in time]))
            ik = np.ascontiguousarray(internal_knots, dtype=np.float64)
            bk = np.ascontiguousarray(boundary_knots, dtype=np.float64)
            cfg.n_funct = len(Y)
            cfg.n_internal_knots = len(ik)
            self.P = len(ik) + cfg.basis_degree + 1
            _lib.check(self.lib.bfmmm_create_batch(C.byref(cfg), device, _dp(y), _dp(t),
                                                   self.offsets.ctypes.data_as(_lib.c_int64_p), _dp(ik), _dp(bk),
                                                   int(n_chains), C.byref(self.h)))
        else:
            Ym = np.asfortranarray(Y, dtype=np.float64)
            cfg.n_funct, cfg.P = Ym.shape
            self.P = cfg.P
            self.offsets = None
            _lib.check(self.lib.bfmmm_create_batch(C.byref(cfg), device, _dp(Ym), None, None, None, None, int(n_chains),
                                                   C.byref(self.h)))
        self.n, self.K, self.M, self.T = cfg.n_funct, cfg.K, cfg.n_eigen, cfg.tot_mcmc_iters
        self.D = 0
        self.n_chains = int(n_chains)

    def select_chain(self, q):
        """Chain of the batch that set_state / get_state / init_state / get_chain / debug address."""
        _lib.check(self.lib.bfmmm_select_chain(self.h, int(q)))

    def set_chain_id_stride(self, stride):
        """Chain q of the batch draws from RNG chain id `chain + q * stride` (default 1)."""
        _lib.check(self.lib.bfmmm_set_chain_id_stride(self.h, int(stride)))

    def set_covariates(self, X, covariance_adj=False):
        """X: (n, D) covariate matrix (the `X` argument of the reference's entry points)."""
        Xm = np.asfortranarray(X, dtype=np.float64)
        assert Xm.shape[0] == self.n
        _lib.check(self.lib.bfmmm_set_covariates(self.h, _dp(Xm), Xm.shape[1], int(covariance_adj)))
        self.D = Xm.shape[1]

    def close(self):
        if self.h:
            self.lib.bfmmm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- shapes of the reference's objects ----
    def _draw_shape(self, name):
        size = {"n": self.n, "K": self.K, "P": self.P, "M": self.M, "D": self.D, "2": 2}
        return tuple(size[c] for c in DRAW_DIMS[name])

    def _state_shape(self, name):
        return STATE_ONLY[name] if name in STATE_ONLY else self._draw_shape(name) or (1,)

    def _slots(self, first_slot, n_slots):
        return self.T - int(first_slot) if n_slots is None else int(n_slots)

    def _basis_arg(self, E, name):
        """E as a contiguous G x P matrix of rows in the sampler's basis"""
        Em = np.ascontiguousarray(E, dtype=np.float64)
        if Em.ndim != 2 or Em.shape[1] != self.P:
            raise ValueError(f"{name} must be a G x {self.P} matrix in the sampler's basis")
        return Em

    def _x_arg(self, x):
        """one covariate setting of D entries, or None"""
        if x is None:
            return None
        xv = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if self.D > 0 and xv.size != self.D:
            raise ValueError(f"x must have {self.D} entries, one per covariate")
        return xv

    def _obs_counts(self):
        """(n,): the observations of every curve (the multivariate model: the P coordinates of a row)"""
        return np.full(self.n, self.P, dtype=np.int64) if self.offsets is None else np.diff(self.offsets)

    def _curve_list(self, curves):
        """(the index array, which must outlive the call; its pointer; the curves of the result), all n where curves is None"""
        if curves is None:
            return None, None, self.n
        idx = np.ascontiguousarray(curves, dtype=np.int32).reshape(-1)
        return idx, _ip(idx), idx.size

    def set_state(self, **kw):
        for name, v in kw.items():
            a = np.asfortranarray(np.asarray(v, dtype=np.float64).reshape(self._state_shape(name), order="F"))
            _lib.check(self.lib.bfmmm_set_state(self.h, name.encode(), _dp(a), a.size))

    def get_state(self, name):
        out = np.zeros(self._state_shape(name), order="F")
        _lib.check(self.lib.bfmmm_get_state(self.h, name.encode(), _dp(out), out.size))
        return out

    def init_state(self, stage, seed, chain=0):
        _lib.check(self.lib.bfmmm_init_state(self.h, stage, seed, chain))

    def run(self, mask, n_iters, first_iter=0, seed=1, chain=0, phi_chi_zero=False, beta=1.0):
        _lib.check(self.lib.bfmmm_run(self.h, mask, first_iter, n_iters, seed, chain, int(phi_chi_zero), beta))

    def prepare_run(self, mask, n_iters, first_iter=0, seed=1, chain=0, phi_chi_zero=False):
        """Captures the HIP graphs `run` with the same arguments replays (set-up only, launches nothing)."""
        _lib.check(self.lib.bfmmm_prepare_run(self.h, mask, first_iter, n_iters, seed, chain, int(phi_chi_zero)))

    def set_slot_base(self, base):
        """Chain iteration i is written to slot i - base (on-disk batches reuse the slots, include/bfmmm.h)."""
        _lib.check(self.lib.bfmmm_set_slot_base(self.h, int(base)))

    def tempered_transition(self, mask, iteration, N_t, beta_N_t, seed=1, chain=0):
        """Tempered-transition block of BFMMM_warm_start (BFMMM.h:1556-1657) for the chain iteration that `run` has just
        produced; returns (log acceptance probability, accepted)."""
        import ctypes as C
        la = C.c_double(0.0)
        acc = C.c_int(0)
        _lib.check(self.lib.bfmmm_tempered_transition(self.h, mask, iteration, N_t, beta_N_t, seed, chain,
                                                      C.byref(la), C.byref(acc)))
        return la.value, bool(acc.value)

    def run_tt(self, mask, iteration, beta, tt_step, seed=1, chain=0):
        """For the tests: sweep `tt_step` of a tempered-transition block on its own (bfmmm_debug_run_tt), the call the block's loop
        makes.  The debug reads and route words afterwards describe that sweep."""
        _lib.check(self.lib.bfmmm_debug_run_tt(self.h, mask, int(iteration), seed, chain, float(beta), int(tt_step)))

    def tt_trace(self):
        """What the last `tempered_transition` computed on the host (bfmmm_debug_get "tt_trace"): {"N_t", "ladder": (N_t,), "betas":
        (2 N_t,), the temperature of sweep l = 1 .. 2 N_t, "sig" and "rss": (2 N_t + 1,), sigma^2 and the RSS before the block and
        after every sweep, "log_u", "logA", "accepted"}."""
        v = self.debug("tt_trace", 1 << 16)
        N = int(v[0])
        assert v.size == 7 * N + 6, (N, v.size)
        o = np.cumsum([1, N, 2 * N, 2 * N + 1, 2 * N + 1])
        return dict(N_t=N, ladder=v[o[0]:o[1]], betas=v[o[1]:o[2]], sig=v[o[2]:o[3]], rss=v[o[3]:o[4]], log_u=float(v[o[4]]),
                    logA=float(v[o[4] + 1]), accepted=bool(v[o[4] + 2]))

    def get_chain(self, name, n_slots=None):
        T = self.T if n_slots is None else n_slots
        shp = (T, self.K) if name == "tau" else self._draw_shape(name) + (T,)      # tau: slot fastest
        out = np.zeros(shp, order="F")
        _lib.check(self.lib.bfmmm_get_chain(self.h, name.encode(), T, _dp(out), out.size))
        return out

    def diagnostics(self, name, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Split R-hat, bulk / tail ESS, ESS and MCSE of the mean, mean and sd of chain slots [first_slot, first_slot + n_slots)
        of `name` (a get_chain name) over every chain of the batch, computed on the device (bfmmm_chain_diagnostics).
        Returns a dict of the seven statistics, each shaped like one draw of `name` (Z: (n, K); tau: (K,))."""
        T = self._slots(first_slot, n_slots)
        shp = self._draw_shape(name) if name in DRAW_DIMS else (1,)
        cnt = int(np.prod(shp, dtype=np.int64))
        outs = [np.zeros(cnt) for _ in range(7)]
        _lib.check(self.lib.bfmmm_chain_diagnostics(self.h, name.encode(), int(first_slot), T, int(max_workspace_bytes),
                                                    *[_dp(o) for o in outs], cnt))
        return {k: o.reshape(shp, order="F") for k, o in zip(STAT_NAMES, outs)}

    def curve_loglik(self, first_slot=0, n_slots=None):
        """The marginal log-density (scores integrated out) of every curve under chain slots [first_slot, first_slot + n_slots)
        of every chain of the batch, computed on the device from the resident per-curve statistics (bfmmm_chain_curve_loglik;
        DESIGN.md 7d).  Label- and sign-invariant.  Returns an (n, C, S) array."""
        S = self._slots(first_slot, n_slots)
        out = np.zeros((self.n, self.n_chains, max(S, 0)))
        _lib.check(self.lib.bfmmm_chain_curve_loglik(self.h, int(first_slot), S, _dp(out), out.size))
        return out

    def curve_diagnostics(self, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """The seven statistics of `diagnostics` for each curve's log-density (`curve_loglik`), which never leaves the device
        (bfmmm_chain_curve_diagnostics).  Where the R-hat of nu, Phi or Z reports a label switch between chains, this one
        reports mixing, curve by curve.  Returns a dict of arrays of shape (n,)."""
        S = self._slots(first_slot, n_slots)
        outs = [np.zeros(self.n) for _ in range(7)]
        _lib.check(self.lib.bfmmm_chain_curve_diagnostics(self.h, int(first_slot), S, int(max_workspace_bytes),
                                                          *[_dp(o) for o in outs], self.n))
        return dict(zip(STAT_NAMES, outs))

    def loo(self, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """PSIS-LOO and WAIC over curves from the chain slots of every chain, pooled (bfmmm_chain_loo): the dict api.psis_loo
        returns for the (n, C * S) matrix `curve_loglik` holds, without that matrix leaving the device."""
        S = self._slots(first_slot, n_slots)
        outs = [np.zeros(self.n) for _ in range(6)]
        _lib.check(self.lib.bfmmm_chain_loo(self.h, int(first_slot), S, int(max_workspace_bytes), *[_dp(o) for o in outs], self.n))
        return _loo_dict(outs, self.n_chains * S)

    REFINE_TRACE_BYTES = 512 << 20      # loo_marginal(trace=True): the most "refine_prop" and "refine_samples" may take on the host

    @_proposal_option("_loo_marginal_laplace", {"n_stages": lambda v: v != 3, "refine": bool, "refine_samples": lambda v: v is not None,
                                                "refine_stages": lambda v: v != 2})
    def loo_marginal(self, first_slot=0, n_slots=None, n_samples=256, n_stages=3, seed=1, refine=True, ess_floor=10.0,
                     refine_samples=None, refine_stages=2, trace=False, max_workspace_bytes=0):
        """PSIS-LOO and WAIC over curves with the memberships integrated out (bfmmm_chain_loo_marginal).  `loo` runs
        PSIS on log p(y_i | Z_i, draw), which is conditional on the draw's memberships of curve i; leaving the curve out sends them
        back to their prior, so that estimate is the conditional LOO and its importance ratios are heavy-tailed.  This call runs PSIS
        on log p(y_i | draw), the integral over Z_i ~ Dir(alpha_3 pi) that `predict` estimates per (curve, draw), taken here from the
        resident records of the training curves: n_stages rounds of n_samples samples, the traces of predict(Y, time, trace=True)
        with the same seed bit for bit.  With refine, every (curve, draw) pair whose importance-sampling ess is below ess_floor (or
        whose estimate is not finite) is run once more from the last proposal of its first pass: refine_stages rounds of
        refine_samples samples (default 4 * n_samples).  Such a pair would otherwise carry the largest weight of its curve.
        Returns the dict of `loo` and "ess_mean", "ess_min": (n,), after the refinement; "n_refined": (n,), the pairs of the curve
        that were refined; "n_below": (n,), the pairs still below the floor afterwards -- reported, never dropped: read it and
        "pareto_k" before the totals; and the six call parameters.  trace adds "lpd_trace", "ess_trace": (n, C, S) after the
        refinement, "ess_trace_first": (n, C, S) before it, "refined_index": (n_ref, 3), the (curve, chain, slot relative to
        first_slot) of the refined pairs in increasing order, and, for tests and small shapes (where they would take no more than
        REFINE_TRACE_BYTES if every pair were refined), "refine_prop": (n_ref, R2, K) and "refine_samples": (n_ref, R2, J2, K), which then
        takes the place of the parameter of that name.  All chains of the batch, pooled, on one device.
        The keyword proposal="laplace" (bfmmm_chain_loo_marginal_laplace) takes the integral in one round from `predict`'s mixture of
        Student-t components at the modes of the integrand: the traces of predict(Y, time, proposal="laplace", trace=True) bit for bit,
        no stages and no refinement -- n_stages other than its default and refine=True, refine_samples or refine_stages given
        explicitly are refused.  The result then holds "n_modes_mean": (n,) in place of "n_refined" and the refinement's parameters,
        and trace adds "n_modes", "components" and "eta_samples" as `predict` does."""
        S = self._slots(first_slot, n_slots)
        n, Cn, K, Sn = self.n, self.n_chains, self.K, max(S, 0)
        J, R, R2 = int(n_samples), int(n_stages), int(refine_stages)
        J2 = 4 * J if refine_samples is None else int(refine_samples)
        outs = [np.zeros(n) for _ in range(8)]
        n_refined, n_below = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        tr, idx, prop, smp, cap = {}, None, None, None, 0
        if trace:
            tr = {k: np.zeros((n, Cn, Sn)) for k in ("lpd_trace", "ess_trace", "ess_trace_first")}
            cap = n * Cn * Sn
            idx = np.zeros((cap, 3), dtype=np.int32)
            if refine and 8 * cap * max(R2, 0) * (1 + max(J2, 0)) * K <= self.REFINE_TRACE_BYTES:
                prop, smp = np.zeros((cap, max(R2, 0), K)), np.zeros((cap, max(R2, 0), max(J2, 0), K))
        n_ref = C.c_int64(0)
        opt = _opt(dict(tr, prop=prop, smp=smp))
        _lib.check(self.lib.bfmmm_chain_loo_marginal(
            self.h, int(first_slot), S, J, R, int(seed), int(bool(refine)), float(ess_floor), J2, R2, int(max_workspace_bytes),
            *[_dp(o) for o in outs], _ip(n_refined), _ip(n_below), opt("lpd_trace"), opt("ess_trace"),
            opt("ess_trace_first"), None if idx is None else _ip(idx), opt("prop"), opt("smp"), C.byref(n_ref), n, cap))
        out = _loo_dict(outs, Cn * S)
        out.update(ess_mean=outs[6], ess_min=outs[7], n_refined=n_refined, n_below=n_below, n_samples=J, n_stages=R, refine=bool(refine),
                   ess_floor=float(ess_floor), refine_samples=J2, refine_stages=R2)
        out.update(tr)
        if trace:
            m = n_ref.value
            out["refined_index"] = idx[:m].copy()
            if prop is not None:
                out["refine_prop"], out["refine_samples"] = prop[:m].copy(), smp[:m].copy()
        return out

    def _loo_marginal_laplace(self, first_slot, n_slots, n_samples, seed, ess_floor, trace, max_workspace_bytes):
        """loo_marginal(proposal="laplace")"""
        S = self._slots(first_slot, n_slots)
        n, Cn, K, Sn, J = self.n, self.n_chains, self.K, max(S, 0), int(n_samples)
        d = K - 1
        outs = [np.zeros(n) for _ in range(8)]
        n_below, n_modes = np.zeros(n, dtype=np.int32), np.zeros((n, Cn, Sn), dtype=np.int32)
        tr = {}
        if trace:
            tr = {"lpd_trace": np.zeros((n, Cn, Sn)), "ess_trace": np.zeros((n, Cn, Sn)),
                  "components": np.zeros((n, Cn, Sn, K + 2, d + d * (d + 1) // 2 + 2)), "eta_samples": np.zeros((n, Cn, Sn, max(J, 0), d))}
        opt = _opt(tr)
        _lib.check(self.lib.bfmmm_chain_loo_marginal_laplace(
            self.h, int(first_slot), S, J, int(seed), float(ess_floor), int(max_workspace_bytes), *[_dp(o) for o in outs], _ip(n_below),
            opt("lpd_trace"), opt("ess_trace"), _ip(n_modes), opt("components"), opt("eta_samples"), n))
        out = _loo_dict(outs, Cn * S)
        out.update(ess_mean=outs[6], ess_min=outs[7], n_below=n_below, n_modes_mean=n_modes.mean(axis=(1, 2)), n_samples=J,
                   ess_floor=float(ess_floor), proposal="laplace")
        out.update(tr)
        if trace:
            out["n_modes"] = n_modes
        return out

    def loo_pointwise(self, curves=None, first_slot=0, n_slots=None, trace=False, max_workspace_bytes=0):
        """Observation-level PSIS-LOO and LOO-PIT from the chain slots of every chain, pooled (bfmmm_chain_loo_pointwise):
        every observation y_ij of the selected curves (None: all) is left out in turn with the rest of its curve kept and the scores
        chi_i integrated out -- "does the model interpolate a curve between its own observations".  Returns the dict of `loo` over the
        N_obs observations (curve by curve in the order of `curves`, then observation by observation; the multivariate model: the P
        coordinates of a curve) and "pit": E_loo[Phi(z_ij)], uniform under a calibrated model, "mean" and "sd": the LOO predictive
        mean and sd of every observation, all (N_obs,); "offsets": (n_curves + 1,), curve j of the selection owns entries
        offsets[j]:offsets[j + 1]; "curve_elpd_loo": the sums of "pointwise_elpd_loo" per curve.  trace adds "loglik_trace",
        "pit_trace", "mean_trace" and "var_trace": (N_obs, C, S), refused above REFINE_TRACE_BYTES on the host."""
        S = self._slots(first_slot, n_slots)
        idx, pc, m = self._curve_list(curves)
        sel = np.arange(self.n) if idx is None else idx
        if sel.size and (sel.min() < 0 or sel.max() >= self.n):
            raise ValueError(f"loo_pointwise: 'curves' must lie in 0 .. {self.n - 1}")
        offsets = np.zeros(m + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(self._obs_counts()[sel])
        N = int(offsets[-1])
        Cn, Sn = self.n_chains, max(S, 0)
        tr = {}
        if trace:
            if 4 * 8 * N * Cn * Sn > self.REFINE_TRACE_BYTES:
                raise ValueError(f"loo_pointwise: the four traces of {N} observations x {Cn} chains x {Sn} slots take "
                                 f"{4 * 8 * N * Cn * Sn} bytes on the host, above REFINE_TRACE_BYTES = {self.REFINE_TRACE_BYTES}: "
                                 f"select fewer curves or slots")
            tr = {k: np.zeros((N, Cn, Sn)) for k in ("loglik_trace", "pit_trace", "mean_trace", "var_trace")}
        outs = [np.zeros(N) for _ in range(9)]
        opt = _opt(tr)
        _lib.check(self.lib.bfmmm_chain_loo_pointwise(self.h, pc, m, int(first_slot), S, int(max_workspace_bytes), *[_dp(o) for o in outs],
                                                      opt("loglik_trace"), opt("pit_trace"), opt("mean_trace"), opt("var_trace"), N))
        out = _loo_dict(outs, Cn * S)
        out.update(pit=outs[6], mean=outs[7], sd=outs[8], offsets=offsets,
                   curve_elpd_loo=np.array([outs[1][offsets[j]:offsets[j + 1]].sum() for j in range(m)]))
        out.update(tr)
        return out

    def loo_by_chain(self, unit="observation", curves=None, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """PSIS-LOO and WAIC of every chain of the batch by itself (bfmmm_chain_loo_by_chain): the six pointwise arrays
        of `loo` (unit "curve"; `curves` must be None) or of `loo_pointwise` (unit "observation", with its "offsets"), each of shape
        (rows, C), column c from PSIS on the n_slots draws of chain c alone -- api.psis_loo of that chain's log-density matrix, bit
        for bit.  "elpd_loo" and "se_elpd_loo": (C,), per chain; "khat_threshold" for S = n_slots draws and "n_khat_above": (C,).  A
        chain has 1 / C of the pooled draws, so its k-hat is worse than the pooled one: read "n_khat_above" first."""
        from . import api
        units = {"curve": 0, "observation": 1}
        if unit not in units:
            raise ValueError(f"loo_by_chain: 'unit' must be one of {sorted(units)}")
        if unit == "curve" and curves is not None:
            raise ValueError("loo_by_chain: 'curves' goes with unit \"observation\"")
        S = self._slots(first_slot, n_slots)
        idx, pc, m = self._curve_list(curves)
        out = {}
        rows = self.n
        if unit == "observation":
            sel = np.arange(self.n) if idx is None else idx
            if sel.size and (sel.min() < 0 or sel.max() >= self.n):
                raise ValueError(f"loo_by_chain: 'curves' must lie in 0 .. {self.n - 1}")
            offsets = np.zeros(m + 1, dtype=np.int64)
            offsets[1:] = np.cumsum(self._obs_counts()[sel])
            rows = int(offsets[-1])
            out["offsets"] = offsets
        Cn = self.n_chains
        outs = [np.zeros((rows, Cn)) for _ in range(6)]
        _lib.check(self.lib.bfmmm_chain_loo_by_chain(self.h, units[unit], pc, m if curves is not None else 0, int(first_slot), S,
                                                     int(max_workspace_bytes), *[_dp(o) for o in outs], rows * Cn))
        out.update(zip(_PW_NAMES, outs))
        tot = [api._total_se(outs[1][:, c]) for c in range(Cn)]
        with np.errstate(divide="ignore"):
            thr = float(min(1.0 - 1.0 / np.log10(float(S)), 0.7))
        out.update(elpd_loo=np.array([t[0] for t in tot]), se_elpd_loo=np.array([t[1] for t in tot]), khat_threshold=thr,
                   n_khat_above=np.sum(outs[3] > thr, axis=0).astype(np.int64))
        return out

    def chain_stacking(self, unit="observation", curves=None, first_slot=0, n_slots=None, max_workspace_bytes=0, **kw):
        """Stacking weights of the chains of the batch (Yao et al. 2022): `loo_by_chain`, then api.stacking (keywords go
        to it) on its "pointwise_elpd_loo" with the chains as candidates.  Returns the dict of api.stacking -- "weights": (C,); a
        weight near zero says that the chain sits in a mode that predicts worse -- and "by_chain", the dict of `loo_by_chain`.  A
        diagnostic: the pooled summaries of this class weight the chains equally."""
        from . import api
        by = self.loo_by_chain(unit=unit, curves=curves, first_slot=first_slot, n_slots=n_slots, max_workspace_bytes=max_workspace_bytes)
        out = api.stacking(by["pointwise_elpd_loo"], device=self.device, **kw)
        out["by_chain"] = by
        return out

    def loo_blocks(self, blocks=None, block_size=None, horizon=None, curves=None, first_slot=0, n_slots=None, trace=False,
                   max_workspace_bytes=0):
        """Leave-block-out PSIS cross-validation within curves from the chain slots of every chain, pooled (bfmmm_chain_loo_blocks;
        DESIGN.md 7s): every listed block of observations of a training curve is left out in turn with the rest of its curve kept, Z_i at
        the draw's value and the scores chi_i integrated out -- "given part of a curve, how well does the model predict a stretch of
        it".  Exactly one of blocks (a sequence of (curve, indices) pairs, in the order of the result), block_size (every selected
        curve cut into consecutive blocks, the last one shorter) and horizon (one block a curve, its last `horizon` observations:
        leave-future-out) is given; `curves` goes with the latter two (see block_plan).  A block has 1 to 64 distinct observations;
        blocks may overlap.  The multivariate model: the P coordinates of a row are its observations.
        Returns the dict of `loo` over the BLOCKS (PSIS on the block's joint log-density; "pareto_k" says when a block is too large
        for the correction) and, per listed observation, "pit": E[Phi(z_j)], "mean" and "sd": the marginals of the leave-block-out
        predictive law, (N_rows,); "offsets": (n_blocks + 1,), block k owns rows offsets[k]:offsets[k + 1]; "block_curve",
        "block_size": (n_blocks,); "obs": (N_rows,), the index of each listed observation within its curve; "curve_elpd_loo" and
        "curve_index": the sums of the block elpds per distinct curve, in order of first appearance.  trace adds "loglik_trace":
        (n_blocks, C, S) and "pit_trace", "mean_trace", "var_trace": (N_rows, C, S), refused above REFINE_TRACE_BYTES on the host."""
        S = self._slots(first_slot, n_slots)
        bc, bo, bx = block_plan(self._obs_counts(), blocks=blocks, block_size=block_size, horizon=horizon, curves=curves)
        nb, N = len(bc), int(bo[-1])
        Cn, Sn = self.n_chains, max(S, 0)
        tr = {}
        if trace:
            need = 8 * (3 * N + nb) * Cn * Sn
            if need > self.REFINE_TRACE_BYTES:
                raise ValueError(f"loo_blocks: the four traces of {nb} blocks and {N} observations x {Cn} chains x {Sn} slots take "
                                 f"{need} bytes on the host, above REFINE_TRACE_BYTES = {self.REFINE_TRACE_BYTES}: "
                                 f"list fewer blocks or slots")
            tr = {"loglik_trace": np.zeros((nb, Cn, Sn))}
            tr.update({k: np.zeros((N, Cn, Sn)) for k in ("pit_trace", "mean_trace", "var_trace")})
        outs = [np.zeros(nb) for _ in range(6)] + [np.zeros(N) for _ in range(3)]
        opt = _opt(tr)
        _lib.check(self.lib.bfmmm_chain_loo_blocks(self.h, _ip(bc), bo.ctypes.data_as(_lib.c_int64_p), _ip(bx), nb, int(first_slot), S,
                                                   int(max_workspace_bytes), *[_dp(o) for o in outs], opt("loglik_trace"),
                                                   opt("pit_trace"), opt("mean_trace"), opt("var_trace"), nb, N))
        out = _loo_dict(outs, Cn * S)
        # per distinct curve, in order of first appearance: the curve's blocks in the order of the list, summed
        uniq, first = np.unique(bc, return_index=True)
        order = np.argsort(bc, kind="stable")
        sums = np.array([seg.sum() for seg in np.split(outs[1][order], np.cumsum(np.bincount(bc)[uniq])[:-1])])
        by_first = np.argsort(first, kind="stable")
        out.update(pit=outs[6], mean=outs[7], sd=outs[8], offsets=bo, block_curve=bc, block_size=np.diff(bo), obs=bx,
                   curve_index=uniq[by_first], curve_elpd_loo=sums[by_first])
        out.update(tr)
        return out

    def _fit_args(self, E, which, curves, first_slot, n_slots):
        w = {"mean": 0, "fit": 1}.get(which, which)
        if isinstance(w, str):
            raise ValueError("which must be 'mean' or 'fit'")
        w = int(w)
        Em = self._basis_arg(E, "E")
        S = self._slots(first_slot, n_slots)
        idx, pc, m = self._curve_list(curves)
        return w, Em, S, idx, pc, m

    def curve_fit(self, E, which="fit", curves=None, first_slot=0, n_slots=None):
        """Every curve's fitted function on the rows of E (G x P, in the sampler's basis: api.TensorBSpline rows on a time grid,
        a curve's own get_basis() rows, the identity for the multivariate model) under chain slots [first_slot, first_slot +
        n_slots) of every chain of the batch (bfmmm_chain_curve_fit).  which="mean": E c_i, the curve's mean
        function; "fit": E (c_i + sum_m chi_im V_im).  Label- and sign-invariant.  curves: indices, in any order (default: all).
        Returns an (m, G, C, S) array; meant for a handful of curves."""
        w, Em, S, idx, pc, m = self._fit_args(E, which, curves, first_slot, n_slots)
        out = np.zeros((m, Em.shape[0], self.n_chains, max(S, 0)))
        _lib.check(self.lib.bfmmm_chain_curve_fit(self.h, w, _dp(Em), Em.shape[0], pc, m, int(first_slot), S, _dp(out), out.size))
        return out

    def curve_bands(self, E, which="fit", probs=(0.025, 0.5, 0.975), curves=None, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Pointwise posterior mean, sd and quantiles of `curve_fit`'s values with the chains pooled, computed on the device
        without the values leaving it (bfmmm_chain_curve_bands).  Quantiles follow arma::quantile's rule, as the single-chain
        credible bands do.  Returns {"mean": (m, G), "sd": (m, G), "quantiles": (m, G, nq), "probs": (nq,)}."""
        w, Em, S, idx, pc, m = self._fit_args(E, which, curves, first_slot, n_slots)
        pr = _probs_arg(probs)
        G = Em.shape[0]
        mean, sd, qs = np.zeros((m, G)), np.zeros((m, G)), np.zeros((m, G, pr.size))
        _lib.check(self.lib.bfmmm_chain_curve_bands(self.h, w, _dp(Em), G, pc, m, int(first_slot), S, _dp(pr), pr.size,
                                                    int(max_workspace_bytes), _dp(mean), _dp(sd), _dp(qs), m * G))
        return {"mean": mean, "sd": sd, "quantiles": qs, "probs": pr}

    def curve_bands_simultaneous(self, E, which="fit", alpha=0.05, curves=None, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Simultaneous (1 - alpha) credible band of every curve's `curve_fit` values with the chains pooled, by the reference's
        rule (FMeanCI's `simultaneous`), on the device (bfmmm_chain_curve_bands_sim): crit is the (1 - alpha)
        quantile over the draws of max_g |v(g) - mean(g)| / sd(g), and the band mean -/+ crit sd holds whole posterior curves,
        which `curve_bands`' pointwise quantiles do not.  mean and sd are `curve_bands`'.
        Returns {"mean": (m, G), "sd": (m, G), "crit": (m,), "lower": (m, G), "upper": (m, G), "alpha": alpha}."""
        w, Em, S, idx, pc, m = self._fit_args(E, which, curves, first_slot, n_slots)
        G = Em.shape[0]
        mean, sd, lower, upper, crit = np.zeros((m, G)), np.zeros((m, G)), np.zeros((m, G)), np.zeros((m, G)), np.zeros(m)
        _lib.check(self.lib.bfmmm_chain_curve_bands_sim(self.h, w, _dp(Em), G, pc, m, int(first_slot), S, float(alpha),
                                                        int(max_workspace_bytes), _dp(mean), _dp(sd), _dp(crit), _dp(lower), _dp(upper),
                                                        m * G))
        return {"mean": mean, "sd": sd, "crit": crit, "lower": lower, "upper": upper, "alpha": alpha}

    def similarity(self, curves=None, sd=True, per_chain=False, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """The pooled co-membership matrix of the curves: mean (and sd) over chain slots [first_slot, first_slot + n_slots) of
        every chain of the batch of d_ij = sum_k Z_ik Z_jk, the posterior similarity of curves i and j, computed on the device
        (bfmmm_chain_similarity).  Label-invariant, so chains pool as they are.  curves: the rows wanted, indices
        in any order (default: all n); columns are all curves.  per_chain: also each chain's own mean, which shows whether the
        chains agree on the clustering where their labels differ.
        Returns {"mean": (m, n), "sd": (m, n) if sd, "chain_mean": (m, C, n) if per_chain}."""
        S = self._slots(first_slot, n_slots)
        idx, pc, m = self._curve_list(curves)
        out = {"mean": np.zeros((m, self.n))}
        if sd:
            out["sd"] = np.zeros((m, self.n))
        if per_chain:
            out["chain_mean"] = np.zeros((m, self.n_chains, self.n))
        _lib.check(self.lib.bfmmm_chain_similarity(self.h, pc, m if curves is not None else 0, int(first_slot), S, int(max_workspace_bytes),
                                                   _dp(out["mean"]), _dp(out["sd"]) if sd else None,
                                                   _dp(out["chain_mean"]) if per_chain else None, m * self.n))
        return out

    def similarity_loss(self, first_slot=0, n_slots=None, diagnostics=True, max_workspace_bytes=0):
        """The least-squares loss of every draw of chain slots [first_slot, first_slot + n_slots) of every chain of the batch,
        loss(q, t) = sum_ij (d_ij(q, t) - m_ij)^2 with m the pooled mean `similarity` returns, computed on the device
        (bfmmm_chain_similarity_loss), and the draw that minimises it (Dahl 2006).  Label-invariant; with
        diagnostics, split R-hat, ESS, MCSE, mean and sd of the loss trace tell whether the chains agree on the clustering.
        Returns {"loss": (C, S), "chain": int, "slot": int (absolute), "min": float} and, with diagnostics, the seven
        STAT_NAMES as floats."""
        S = self._slots(first_slot, n_slots)
        loss = np.zeros((self.n_chains, max(S, 0)))
        chain, slot = C.c_int32(-1), C.c_int32(-1)
        stats = np.zeros(7)
        _lib.check(self.lib.bfmmm_chain_similarity_loss(self.h, int(first_slot), S, int(max_workspace_bytes), _dp(loss), loss.size,
                                                        C.byref(chain), C.byref(slot), _dp(stats) if diagnostics else None))
        out = {"loss": loss, "chain": chain.value, "slot": slot.value, "min": float(loss[chain.value, slot.value - int(first_slot)])}
        if diagnostics:
            out.update((k, float(v)) for k, v in zip(STAT_NAMES, stats))
        return out

    def get_slot(self, name, slot, chain=None):
        """One slot of `name` (a get_chain name): get_chain(name)[..., slot] ("tau": [slot]) without the other slots
        (bfmmm_get_slot).  chain: the chain to read (default: the selected one); the selection is restored afterwards."""
        out = np.zeros(self._draw_shape(name) if name in DRAW_DIMS else (1,), order="F")
        prev = self.lib.bfmmm_selected_chain(self.h)      # the handle's own record, whoever selected last
        if chain is not None:
            self.select_chain(chain)
        try:
            _lib.check(self.lib.bfmmm_get_slot(self.h, name.encode(), int(slot), _dp(out), out.size))
        finally:
            if chain is not None:
                self.select_chain(prev)
        return out

    def set_chain(self, name, values, first_slot=0, chain=None):
        """Writes draws of `name` (a get_chain name) into chain slots [first_slot, first_slot + n_slots): the mirror of get_chain
        (bfmmm_set_chain).  values: shaped as get_chain returns it, (..., n_slots) ("tau": (n_slots, K)).  chain: the
        chain to write (default: the selected one); the selection is restored afterwards.  Nothing but those slots changes.
        Returns the number of slots written."""
        lead = self._draw_shape(name) if name in DRAW_DIMS else ()      # an unknown name: the library refuses it
        a = np.asarray(values, dtype=np.float64)
        if name == "tau":
            if a.ndim != 2 or a.shape[1] != self.K:
                raise ValueError(f"set_chain('tau'): values must be shaped (n_slots, {self.K}), got {a.shape}")
            S = a.shape[0]
        else:
            if a.ndim != len(lead) + 1 or a.shape[:-1] != lead:
                raise ValueError(f"set_chain('{name}'): values must be shaped {lead + ('n_slots',)}, got {a.shape}")
            S = a.shape[-1]
        a = np.asfortranarray(a)
        prev = self.lib.bfmmm_selected_chain(self.h)
        if chain is not None:
            self.select_chain(chain)
        try:
            _lib.check(self.lib.bfmmm_set_chain(self.h, name.encode(), int(first_slot), int(S), _dp(a), a.size))
        finally:
            if chain is not None:
                self.select_chain(prev)
        return S

    def load_chain(self, arrays, first_slot=0, chain=None):
        """set_chain for every entry of the dict `arrays` (name -> array in get_chain's layout), which must agree on the number of
        draws.  Returns the number of slots written."""
        counts = {nm: (np.shape(v)[0] if nm == "tau" else np.shape(v)[-1]) for nm, v in arrays.items()}
        if len(set(counts.values())) > 1:
            raise ValueError(f"load_chain: the arrays disagree on the number of draws: {counts}")
        S = 0
        for nm, v in arrays.items():
            S = self.set_chain(nm, v, first_slot=first_slot, chain=chain)
        return S

    def slot_loglik(self, first_slot=0, n_slots=None, store=False, per_curve=False, max_workspace_bytes=0):
        """The log-likelihood given the scores of chain slots [first_slot, first_slot + n_slots) of every chain of the batch,
        recomputed on the device from the resident per-curve statistics and the slots (bfmmm_chain_slot_loglik): what
        a run stores in "loglik", for chains that were loaded with set_chain, and a check of the stored array otherwise.  store:
        also write it into the "loglik" slots of the range.  Returns the (C, S) array, or with per_curve
        {"loglik": (C, S), "curve": (n, C, S)}, curve the log-density of each curve given its scores."""
        S = self._slots(first_slot, n_slots)
        ll = np.zeros((self.n_chains, max(S, 0)))
        cv = np.zeros((self.n, self.n_chains, max(S, 0))) if per_curve else None
        _lib.check(self.lib.bfmmm_chain_slot_loglik(self.h, int(first_slot), S, int(bool(store)), int(max_workspace_bytes), _dp(ll),
                                                    _dp(cv) if per_curve else None, cv.size if per_curve else ll.size))
        return {"loglik": ll, "curve": cv} if per_curve else ll

    def representative_draw(self, names=("Z",), first_slot=0, n_slots=None, max_workspace_bytes=0):
        """The least-squares draw of the clustering (`similarity_loss` without its diagnostics) and the arrays `names` of that
        draw, all in the draw's own consistent labelling.  Returns {"chain", "slot", "loss"} plus one array per name."""
        r = self.similarity_loss(first_slot, n_slots, diagnostics=False, max_workspace_bytes=max_workspace_bytes)
        out = {"chain": r["chain"], "slot": r["slot"], "loss": r["min"]}
        for nm in names:
            out[nm] = self.get_slot(nm, r["slot"], chain=r["chain"])
        return out

    def align(self, pivot=None, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Aligns the component labels of every draw of chain slots [first_slot, first_slot + n_slots) of every chain of the batch
        to a pivot (the pivot method; bfmmm_chain_align): perm maximises sum_l (Z' Zref)[perm[l], l] exactly over
        all K! permutations, so that Z[:, perm] is the draw in the pivot's labelling.  Labels only: eigenfunction signs are not
        touched.  pivot: None for the `representative_draw` of the same slots, (chain, slot) for that draw (slot absolute), or an
        (n, K) array.  Returns {"perm": (C, S, K) int32, "score": (C, S), "pivot": {"chain", "slot", "Z"} or None for an array,
        "chain_perm": (C, K), each chain's most frequent permutation (the lexicographically smallest of several),
        "modal_share": (C,), the share of the chain's draws that have it: below 1 the labels switch within the chain}."""
        S = self._slots(first_slot, n_slots)
        info = None
        if pivot is None:
            r = self.representative_draw(("Z",), first_slot, n_slots, max_workspace_bytes)
            info = {"chain": r["chain"], "slot": r["slot"], "Z": r["Z"]}
        elif isinstance(pivot, tuple) and len(pivot) == 2 and all(isinstance(v, (int, np.integer)) for v in pivot):
            info = {"chain": int(pivot[0]), "slot": int(pivot[1]), "Z": self.get_slot("Z", int(pivot[1]), chain=int(pivot[0]))}
        Zref = np.asfortranarray(info["Z"] if info is not None else pivot, dtype=np.float64)
        if Zref.shape != (self.n, self.K):
            raise ValueError(f"pivot must be None, (chain, slot) or an array of shape ({self.n}, {self.K})")
        perm = np.zeros((self.n_chains, max(S, 0), self.K), dtype=np.int32)
        score = np.zeros((self.n_chains, max(S, 0)))
        _lib.check(self.lib.bfmmm_chain_align(self.h, _dp(Zref), int(first_slot), S, _ip(perm),
                                              _dp(score), perm.size))
        chain_perm = np.zeros((self.n_chains, self.K), dtype=np.int32)
        share = np.zeros(self.n_chains)
        for q in range(self.n_chains):
            rows, counts = np.unique(perm[q], axis=0, return_counts=True)      # rows in lexicographic order: argmax takes the first
            chain_perm[q] = rows[int(np.argmax(counts))]
            share[q] = counts.max() / float(S)
        return {"perm": perm, "score": score, "pivot": info, "chain_perm": chain_perm, "modal_share": share}

    def _perm_arg(self, perm, S):
        p = np.ascontiguousarray(perm, dtype=np.int32)
        if p.shape != (self.n_chains, S, self.K):
            raise ValueError(f"perm must have shape ({self.n_chains}, {S}, {self.K}): align()['perm'] of the same slots")
        return p

    @_rescale_option("_rescaled_summary")
    def aligned_summary(self, name, perm, probs=(0.025, 0.5, 0.975), first_slot=0, n_slots=None, max_workspace_bytes=0):
        """`diagnostics(name)` with every draw's components relabelled by its row of perm (`align`'s "perm" of the same slots),
        and pooled quantiles of the same values, on the device (bfmmm_chain_aligned_summary): memberships with
        credible intervals for "Z", and an R-hat of nu or Z that measures mixing rather than labelling.  Names without a component
        axis are summarised as they are.  Keyword-only rescale=None: the dict of `rescale` for the same slots, and the summary is the
        one after the reference's rescale step (bfmmm_chain_rescaled_summary): "nu", "Phi", "eta" and "xi" mixed over
        their component axis by every draw's A, "Z" by its A^-1 -- memberships that reach 0 and 1, the reference's ZCI; other names
        are refused, the reference defines no rescale for them.  perm may then be left out or None (the dict has it); where it is
        given it must be the dict's own: a dict made with perm=None takes no perm here, not even the identity.
        Returns the seven STAT_NAMES shaped like a draw, plus "quantiles": shape + (nq,) by
        arma::quantile's rule, and "probs"."""
        S = self._slots(first_slot, n_slots)
        p = self._perm_arg(perm, S)
        pr = _probs_arg(probs)
        shp = self._draw_shape(name) if name in DRAW_DIMS else (1,)
        cnt = int(np.prod(shp, dtype=np.int64))
        outs = [np.zeros(cnt) for _ in range(7)]
        qs = np.zeros((cnt, pr.size))
        _lib.check(self.lib.bfmmm_chain_aligned_summary(self.h, name.encode(), _ip(p), int(first_slot), S,
                                                        _dp(pr) if pr.size else None, pr.size, int(max_workspace_bytes),
                                                        *[_dp(o) for o in outs], _dp(qs) if pr.size else None, cnt))
        out = {k: o.reshape(shp, order="F") for k, o in zip(STAT_NAMES, outs)}
        out["quantiles"] = qs.reshape(shp + (pr.size,), order="F") if shp else qs.reshape((pr.size,))
        out["probs"] = pr
        return out

    @_rescale_option("_cluster_mean_bands_rescaled", with_x=True)
    def cluster_mean_bands(self, E, perm, probs=(0.025, 0.5, 0.975), first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Pointwise posterior mean, sd and quantiles of the K cluster mean functions E nu_k (E: G x P rows in the sampler's basis,
        as in `curve_fit`) with the labels aligned by perm (`align`'s "perm" of the same slots) and the chains pooled, on the
        device (bfmmm_chain_cluster_mean_bands); the reference's FMeanCI without rescale / trans_mats.  With
        covariates set: the mean function at x = 0.  Keyword-only rescale=None: the dict of `rescale` for the same slots (perm as
        in `aligned_summary`), and the bands are those of E sum_c A[k][c] (nu_c + sum_d x_d eta_c,d), the reference's FMeanCI with
        rescale / trans_mats (bfmmm_chain_cluster_mean_bands_rescaled).  Keyword-only x=None: one covariate setting
        of D entries (covariates must be set), honoured only with rescale and refused without it.  Returns {"mean": (K, G), "sd": (K, G), "quantiles": (K, G, nq), "probs"}."""
        Em = self._basis_arg(E, "E")
        S = self._slots(first_slot, n_slots)
        p = self._perm_arg(perm, S)
        pr = _probs_arg(probs)
        G, K = Em.shape[0], self.K
        mean, sd, qs = np.zeros(K * G), np.zeros(K * G), np.zeros((K * G, pr.size))
        _lib.check(self.lib.bfmmm_chain_cluster_mean_bands(self.h, _ip(p), _dp(Em), G, int(first_slot), S,
                                                           _dp(pr) if pr.size else None, pr.size, int(max_workspace_bytes), _dp(mean),
                                                           _dp(sd), _dp(qs) if pr.size else None, K * G))
        return {"mean": mean.reshape((K, G), order="F"), "sd": sd.reshape((K, G), order="F"),
                "quantiles": qs.reshape((K, G, pr.size), order="F"), "probs": pr}

    @_rescale_option("_cluster_cov_bands_rescaled")
    def cluster_cov_bands(self, E, perm, E2=None, pairs=None, x=None, diagonal=False, probs=(0.025, 0.5, 0.975),
                          simultaneous=None, trace=False, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """The covariance surfaces between clusters, C^(k,l)(g, h) = sum_m (E_g . theta_km)(E2_h . theta_lm), theta_km = phi_km +
        sum_d x_d xi_kmd, with the labels aligned by perm (`align`'s "perm" of the same slots) and the chains pooled: pointwise
        mean, sd and quantiles and, with simultaneous=alpha, the simultaneous (1 - alpha) band of every pair by
        `curve_bands_simultaneous`' rule, on the device (bfmmm_chain_cluster_cov_bands); the reference's FCovCI
        without rescale / trans_mats.  Keyword-only rescale=None: the dict of `rescale` for the same slots (perm as in
        `aligned_summary`), and theta~_km = sum_c A[k][c] theta_cm takes the place of theta_{perm[k], m}, the reference's FCovCI with
        rescale / trans_mats (bfmmm_chain_cluster_cov_bands_rescaled).  The sum over m does not see the signs of the
        eigenfunctions, so labels are all that has to be aligned.  E (G1 x P) and E2 (G2 x P; default: E) are rows in the sampler's basis.  pairs: (k, l) pairs of aligned
        components in any order (default: all k <= l, (0, 0), (0, 1), ..).  x: one covariate setting of D entries (covariance-
        adjusted samplers; default: phi alone).  diagonal: only g = h (E2 must be None), the variance function where k = l.
        trace: also the values of every draw, chain-major.
        Returns {"mean", "sd": (m, G1, G2), "quantiles": (m, G1, G2, nq), "probs", "pairs": (m, 2)}, with simultaneous also
        {"crit": (m,), "lower", "upper": (m, G1, G2), "alpha"}, with trace also {"trace": (m, G1, G2, N)}; with diagonal the G2
        axis is dropped."""
        S = self._slots(first_slot, n_slots)
        p = self._perm_arg(perm, S)
        return self._cluster_cov(self.lib.bfmmm_chain_cluster_cov_bands, _ip(p), E, E2, pairs, x, diagonal, probs, simultaneous, trace,
                                 first_slot, S, max_workspace_bytes)

    def _cluster_cov(self, call, labels, E, E2, pairs, x, diagonal, probs, simultaneous, trace, first_slot, S, max_workspace_bytes):
        """the body of `cluster_cov_bands` without and with rescale=: `labels` is the pointer to perm or to the transform"""
        E1m = self._basis_arg(E, "E")
        E2m = None if E2 is None else self._basis_arg(E2, "E2")
        pr = _probs_arg(probs)
        if pairs is None:
            pl = np.array([(k, l) for k in range(self.K) for l in range(k, self.K)], dtype=np.int32).reshape(-1, 2)
        else:
            pl = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        xv = self._x_arg(x)
        m, G1 = pl.shape[0], E1m.shape[0]
        G2 = G1 if E2m is None else E2m.shape[0]
        N = self.n_chains * max(S, 0)
        cell = (G1,) if diagonal else (G1, G2)
        out = {"mean": np.zeros((m,) + cell), "sd": np.zeros((m,) + cell), "quantiles": np.zeros((m,) + cell + (pr.size,)),
               "probs": pr, "pairs": pl}
        if simultaneous is not None:
            out.update(crit=np.zeros(m), lower=np.zeros((m,) + cell), upper=np.zeros((m,) + cell), alpha=simultaneous)
        if trace:
            out["trace"] = np.zeros((m,) + cell + (N,))
        band = [_dp(out[k]) if simultaneous is not None else None for k in ("crit", "lower", "upper")]
        _lib.check(call(
            self.h, labels, _dp(E1m), G1, None if E2m is None else _dp(E2m), G2, int(bool(diagonal)),
            None if pairs is None else _ip(pl), m if pairs is not None else 0, None if xv is None else _dp(xv),
            int(first_slot), S, _dp(pr) if pr.size else None, pr.size, float(simultaneous) if simultaneous is not None else 0.0,
            int(max_workspace_bytes), _dp(out["mean"]), _dp(out["sd"]), _dp(out["quantiles"]) if pr.size else None, *band,
            _dp(out["trace"]) if trace else None, out["mean"].size))
        return out

    def rescale(self, perm=None, transform=None, first_slot=0, n_slots=None):
        """The reference's `rescale` step for every draw of chain slots [first_slot, first_slot + n_slots) of every chain of the
        batch, on the device (bfmmm_chain_rescale).  A mixed-membership model is identified only up to an invertible
        K x K map of the simplex; the reference (ZCI, FMeanCI, FCovCI, MVMeanCI, MVCovCI, rescale on by default) reports Z A^-1,
        A nu, A Phi, A eta and A xi with A the map that makes the purest curve of every component a vertex: row k of A is the Z row
        of the first curve that attains max_i Z[i, perm[k]].  perm: `align`'s "perm" of the same slots (None: the identity).
        transform: (C, S, K, K) matrices used as A instead of the rule, the reference's trans_mats, already in the aligned
        labelling; perm is then only carried along.  The reference refuses the rule for K > 2, where Z A^-1 may leave the simplex;
        here it is allowed and "z_min" reports by how much.  A singular draw (two components share their pure curve, or A is not
        finite) gets a NaN inverse, rcond 0 and z_min NaN, is counted in "n_singular" and passes its NaN on to the pooled rows.
        Returns {"transform", "inverse": (C, S, K, K), "curve": (C, S, K) int32 or None with `transform`, "rcond", "z_min": (C, S),
        "n_singular", "perm", "first_slot", "n_slots"}: the keyword `rescale` of `aligned_summary`, `cluster_mean_bands` and
        `cluster_cov_bands` for the same slots."""
        S = self._slots(first_slot, n_slots)
        Cn, K = self.n_chains, self.K
        p = None if perm is None else self._perm_arg(perm, S)
        tm = None
        if transform is not None:
            tm = np.ascontiguousarray(transform, dtype=np.float64)
            if tm.shape != (Cn, S, K, K):
                raise ValueError(f"transform must have shape ({Cn}, {S}, {K}, {K}): one K x K matrix per chain and slot")
        Sn = max(S, 0)
        out = {"transform": np.zeros((Cn, Sn, K, K)), "inverse": np.zeros((Cn, Sn, K, K)), "curve": np.zeros((Cn, Sn, K), dtype=np.int32),
               "rcond": np.zeros((Cn, Sn)), "z_min": np.zeros((Cn, Sn))}
        ns = C.c_int64(0)
        _lib.check(self.lib.bfmmm_chain_rescale(self.h, None if p is None or tm is not None else _ip(p), None if tm is None else _dp(tm),
                                                int(first_slot), S, _dp(out["transform"]), _dp(out["inverse"]), _ip(out["curve"]),
                                                _dp(out["rcond"]), _dp(out["z_min"]), C.byref(ns), out["transform"].size))
        if tm is not None:
            out["curve"] = None
        out.update(n_singular=int(ns.value), perm=p, first_slot=int(first_slot), n_slots=S)
        return out

    def _rescale_arg(self, rescale, perm, first_slot, S):
        """the dict of `rescale` for these slots, checked against them and against perm where that is given too"""
        need = ("transform", "inverse", "perm", "first_slot", "n_slots")
        if not isinstance(rescale, dict) or any(k not in rescale for k in need):
            raise ValueError("rescale must be the dict Sampler.rescale returns")
        shp = (self.n_chains, S, self.K, self.K)
        if (rescale["first_slot"], rescale["n_slots"]) != (int(first_slot), S):
            raise ValueError(f"rescale is of slots [{rescale['first_slot']}, {rescale['first_slot'] + rescale['n_slots']}), not of "
                             f"[{int(first_slot)}, {int(first_slot) + S}): call Sampler.rescale for the same slots")
        for k in ("transform", "inverse"):
            if np.shape(rescale[k]) != shp:
                raise ValueError(f"rescale['{k}'] has shape {np.shape(rescale[k])}, not {shp}: it is of another sampler")
        if perm is not None:
            p = self._perm_arg(perm, S)
            if rescale["perm"] is None or not np.array_equal(p, rescale["perm"]):
                raise ValueError("perm differs from the perm the rescale dict was computed with")
        return (np.ascontiguousarray(rescale["transform"], dtype=np.float64), np.ascontiguousarray(rescale["inverse"], dtype=np.float64))

    def _rescaled_summary(self, name, rescale, perm=None, probs=(0.025, 0.5, 0.975), first_slot=0, n_slots=None, max_workspace_bytes=0):
        """`aligned_summary` with rescale= (bfmmm_chain_rescaled_summary)"""
        S = self._slots(first_slot, n_slots)
        A, Ai = self._rescale_arg(rescale, perm, first_slot, S)
        pr = _probs_arg(probs)
        shp = self._draw_shape(name) if name in DRAW_DIMS else (1,)
        cnt = int(np.prod(shp, dtype=np.int64))
        outs = [np.zeros(cnt) for _ in range(7)]
        qs = np.zeros((cnt, pr.size))
        _lib.check(self.lib.bfmmm_chain_rescaled_summary(self.h, name.encode(), _dp(A), _dp(Ai), int(first_slot), S,
                                                         _dp(pr) if pr.size else None, pr.size, int(max_workspace_bytes),
                                                         *[_dp(o) for o in outs], _dp(qs) if pr.size else None, cnt))
        out = {k: o.reshape(shp, order="F") for k, o in zip(STAT_NAMES, outs)}
        out["quantiles"] = qs.reshape(shp + (pr.size,), order="F") if shp else qs.reshape((pr.size,))
        out["probs"] = pr
        return out

    def _cluster_mean_bands_rescaled(self, E, rescale, perm=None, x=None, probs=(0.025, 0.5, 0.975), first_slot=0, n_slots=None,
                                     max_workspace_bytes=0):
        """`cluster_mean_bands` with rescale= (bfmmm_chain_cluster_mean_bands_rescaled)"""
        Em = self._basis_arg(E, "E")
        S = self._slots(first_slot, n_slots)
        A, _ = self._rescale_arg(rescale, perm, first_slot, S)
        pr = _probs_arg(probs)
        xv = self._x_arg(x)
        G, K = Em.shape[0], self.K
        mean, sd, qs = np.zeros(K * G), np.zeros(K * G), np.zeros((K * G, pr.size))
        _lib.check(self.lib.bfmmm_chain_cluster_mean_bands_rescaled(self.h, _dp(A), _dp(Em), G, None if xv is None else _dp(xv),
                                                                    int(first_slot), S, _dp(pr) if pr.size else None, pr.size,
                                                                    int(max_workspace_bytes), _dp(mean), _dp(sd),
                                                                    _dp(qs) if pr.size else None, K * G))
        return {"mean": mean.reshape((K, G), order="F"), "sd": sd.reshape((K, G), order="F"),
                "quantiles": qs.reshape((K, G, pr.size), order="F"), "probs": pr}

    def _cluster_cov_bands_rescaled(self, E, rescale, perm=None, E2=None, pairs=None, x=None, diagonal=False, probs=(0.025, 0.5, 0.975),
                                    simultaneous=None, trace=False, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """`cluster_cov_bands` with rescale= (bfmmm_chain_cluster_cov_bands_rescaled)"""
        S = self._slots(first_slot, n_slots)
        A, _ = self._rescale_arg(rescale, perm, first_slot, S)
        return self._cluster_cov(self.lib.bfmmm_chain_cluster_cov_bands_rescaled, _dp(A), E, E2, pairs, x, diagonal, probs, simultaneous,
                                 trace, first_slot, S, max_workspace_bytes)

    def cluster_contrast_bands(self, E, contrasts="pairwise", perm=None, rescale=None, weights=None, probs=(0.025, 0.5, 0.975),
                               simultaneous=None, trace=False, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Contrasts of the cluster mean functions and covariate effects on the rows of E (G x P in the sampler's basis; the identity
        for the multivariate model) with the chains pooled, on the device (bfmmm_chain_cluster_contrast_bands): where
        clusters k and l differ (nu_k - nu_l), what covariate d does to cluster k's mean function (eta_kd), f_k(x) - f_k(x'), and
        differences of differences, each with the joint posterior of its terms, which two marginal bands cannot give.  Exactly one of
        perm (`align`'s "perm" of the same slots) and rescale (the dict of `rescale` for the same slots) says how every draw is
        labelled.  contrasts: "pairwise", "effects", a list of contrasts of terms (weight, k) or (weight, k, x), or a dict {"nu": (R,
        K), "eta": (R, K, D)}: the spellings of `contrast_plan`; at most 64.  weights: G quadrature weights, finite and >= 0, of the
        size of a contrast per draw, norm = sqrt(sum_g w_g v(g)^2) (default 1 / G each: the root mean square over the grid).
        Returns {"mean", "sd", "prob_positive": (R, G), "quantiles": (R, G, nq), "probs", "w_nu": (R, K), "w_eta": (R, K, D) or None,
        "norm": the seven STAT_NAMES (R,) and "quantiles" (R, nq) of the size per draw -- its split R-hat says whether the chains
        agree on how far apart two clusters are, whatever their labels}; prob_positive is the share of draws with v > 0, strictly.
        With simultaneous=alpha also {"crit": (R,), "lower", "upper": (R, G), "excludes_zero": (R, G), "p_sim": (R,), "alpha"}: the
        simultaneous (1 - alpha) band of every contrast by `cluster_cov_bands`' rule, where it excludes zero, and the smallest level
        at which it would exclude the zero function somewhere (1.0 where the contrast does not vary).  With trace also {"trace":
        (R, G, N), "norm_trace": (R, C, S)}."""
        if (perm is None) == (rescale is None):
            raise ValueError("cluster_contrast_bands: exactly one of 'perm' and 'rescale' must be given")
        Em = self._basis_arg(E, "E")
        S = self._slots(first_slot, n_slots)
        K, Cn = self.K, self.n_chains
        if rescale is not None:
            A, _ = self._rescale_arg(rescale, None, first_slot, S)
        else:
            p = self._perm_arg(perm, S)
            if not np.array_equal(np.sort(p, axis=-1), np.broadcast_to(np.arange(K, dtype=np.int32), p.shape)):
                raise ValueError(f"cluster_contrast_bands: every row of perm must be a permutation of 0 .. {K - 1}")
            A = np.ascontiguousarray((p[..., None] == np.arange(K)).astype(np.float64))      # [q, s, k, c] = 1 where c = perm[k]
        w_nu, w_eta = contrast_plan(K, self.D, contrasts)
        wv = None
        if weights is not None:
            wv = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if wv.size != Em.shape[0]:
                raise ValueError(f"weights must have {Em.shape[0]} entries, one per row of E")
        pr = _probs_arg(probs)
        R, G, Sn = w_nu.shape[0], Em.shape[0], max(S, 0)
        N = Cn * Sn
        out = {"mean": np.zeros((R, G)), "sd": np.zeros((R, G)), "quantiles": np.zeros((R, G, pr.size)), "probs": pr}
        npos, nexc = np.zeros((R, G), dtype=np.int32), np.zeros(R, dtype=np.int32)
        stats, nq_out = np.zeros((7, R)), np.zeros((R, pr.size))
        band = simultaneous is not None
        if band:
            out.update(crit=np.zeros(R), lower=np.zeros((R, G)), upper=np.zeros((R, G)))
        tr = {"trace": np.zeros((R, G, N)), "norm_trace": np.zeros((R, Cn, Sn))} if trace else {}
        _lib.check(self.lib.bfmmm_chain_cluster_contrast_bands(
            self.h, _dp(A), _dp(Em), G, _dp(w_nu), None if w_eta is None else _dp(w_eta), R, None if wv is None else _dp(wv),
            int(first_slot), S, _dp(pr) if pr.size else None, pr.size, float(simultaneous) if band else 0.0, int(max_workspace_bytes),
            _dp(out["mean"]), _dp(out["sd"]), _dp(out["quantiles"]) if pr.size else None, _ip(npos),
            *[_dp(out[k]) if band else None for k in ("crit", "lower", "upper")], _ip(nexc) if band else None, _dp(stats),
            _dp(nq_out) if pr.size else None, _opt(tr)("trace"), _opt(tr)("norm_trace"), R * G))
        out["prob_positive"] = npos / float(max(N, 1))
        out["norm"] = dict(zip(STAT_NAMES, stats), quantiles=nq_out)
        out.update(w_nu=w_nu, w_eta=w_eta)
        if band:
            out.update(excludes_zero=(out["lower"] > 0) | (out["upper"] < 0), p_sim=nexc / float(max(N, 1)), alpha=simultaneous)
        out.update(tr)
        return out

    def cluster_eigen(self, E, perm, weights=None, n_functions=None, x=None, ref="mean", probs=(0.025, 0.5, 0.975), trace=False,
                      first_slot=0, n_slots=None, max_workspace_bytes=0):
        """The principal components of the cluster covariance surfaces of `cluster_cov_bands`: per draw and aligned component k the
        eigenvalues lambda_k1 >= .. >= lambda_kM >= 0 and the J = n_functions leading eigenfunctions psi_kj on the grid of the
        operator C^(k,k) discretised with the quadrature weights w, the total variance sum_g w_g C^(k,k)(g, g) and the share
        lambda_kj / total each component explains, with the labels aligned by perm (`align`'s "perm" of the same slots) and the
        chains pooled, on the device (bfmmm_chain_cluster_eigen).  Without the reference's rescale / trans_mats: the
        per-draw transform of `rescale` is out of scope here.  These do not see the signs or the joint rotation of
        the sampler's own eigenfunction blocks, which are not identified.  E (G x P): rows in the sampler's basis (the identity for
        the multivariate model, where this is PCA of Phi_k Phi_k').  weights: G non-negative quadrature weights (default: 1).
        n_functions: default M.  x: one covariate setting of D entries (covariance-adjusted samplers; default: phi alone).
        ref fixes the sign of every eigenfunction, <psi, ref>_w >= 0: "mean" (default) takes the J leading w-eigenfunctions of the
        posterior mean surfaces (`cluster_cov_bands` and numpy.linalg.eigh on the host), each signed so that its entry of
        largest |sqrt(w) psi| is positive; an array (K, J, G) is used as it is; None applies that largest-entry rule to every draw.
        Returns {"values": {"mean", "sd", "rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean": (K, M), "quantiles": (K, M, nq)},
        "pve": {"mean", "sd": (K, M), "quantiles": (K, M, nq)}, "total": {"mean", "sd": (K,), "quantiles": (K, nq)},
        "functions": {"mean", "sd": (K, J, G), "quantiles": (K, J, G, nq)}, "ref": (K, J, G) or None, "max_sweeps", "probs"},
        with trace also {"values_trace": (K, M, N), "functions_trace": (K, J, G, N)}, N = C S chain-major."""
        Em = self._basis_arg(E, "E")
        S = self._slots(first_slot, n_slots)
        p = self._perm_arg(perm, S)
        pr = _probs_arg(probs)
        G, K = Em.shape[0], self.K
        M = self.M
        J = M if n_functions is None else int(n_functions)
        wv = None
        if weights is not None:
            wv = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if wv.size != G:
                raise ValueError(f"weights must have {G} entries, one per row of E")
        xv = self._x_arg(x)
        rv = None
        if isinstance(ref, str):
            if ref != "mean":
                raise ValueError('ref must be "mean", None or an array of shape (K, n_functions, G)')
            if 0 < J <= M and (wv is None or (np.all(np.isfinite(wv)) and np.all(wv >= 0))):
                rv = self._mean_eigenfunctions(Em, p, wv, J, xv, first_slot, n_slots, max_workspace_bytes)
        elif ref is not None:
            rv = np.ascontiguousarray(ref, dtype=np.float64)
            if rv.shape != (K, J, G):
                raise ValueError(f"ref must have shape ({K}, {J}, {G})")
        N = self.n_chains * max(S, 0)
        Jn = max(min(J, M), 0)
        nqs = pr.size
        vd = np.zeros((7, K, M))
        out = {"values": {"quantiles": np.zeros((K, M, nqs))},
               "pve": {"mean": np.zeros((K, M)), "sd": np.zeros((K, M)), "quantiles": np.zeros((K, M, nqs))},
               "total": {"mean": np.zeros(K), "sd": np.zeros(K), "quantiles": np.zeros((K, nqs))},
               "functions": {"mean": np.zeros((K, Jn, G)), "sd": np.zeros((K, Jn, G)), "quantiles": np.zeros((K, Jn, G, nqs))},
               "ref": rv, "probs": pr}
        if trace:
            out["values_trace"] = np.zeros((K, M, N))
            out["functions_trace"] = np.zeros((K, Jn, G, N))
        ms = C.c_int32(0)
        q = (lambda a: _dp(a)) if nqs else (lambda a: None)
        fnp = (lambda a: _dp(a)) if Jn > 0 else (lambda a: None)
        _lib.check(self.lib.bfmmm_chain_cluster_eigen(
            self.h, _ip(p), _dp(Em), G, None if wv is None else _dp(wv), None if xv is None else _dp(xv),
            J, None if rv is None else _dp(rv), int(first_slot), S, _dp(pr) if nqs else None, nqs, int(max_workspace_bytes),
            _dp(vd), q(out["values"]["quantiles"]), _dp(out["pve"]["mean"]), _dp(out["pve"]["sd"]), q(out["pve"]["quantiles"]),
            _dp(out["total"]["mean"]), _dp(out["total"]["sd"]), q(out["total"]["quantiles"]), fnp(out["functions"]["mean"]),
            fnp(out["functions"]["sd"]), fnp(out["functions"]["quantiles"]) if nqs else None,
            _dp(out["values_trace"]) if trace else None, _dp(out["functions_trace"]) if trace and Jn > 0 else None, C.byref(ms),
            K * Jn * G))
        out["values"].update((k, vd[i]) for i, k in enumerate(STAT_NAMES))
        out["max_sweeps"] = int(ms.value)
        return out

    @_proposal_option("_predict_laplace", {"n_stages": lambda v: v != 3, "z_samples": lambda v: v is not None, "return_samples": bool})
    def predict(self, Y_new, time_new=None, basis_new=None, X_new=None, perm=None, n_samples=256, n_stages=3, seed=1,
                trace=False, z_samples=None, return_samples=False, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Held-out curves under the fitted model (bfmmm_chain_predict): for every new curve the log predictive
        density log p(y_new | data) and the predictive law of its memberships Z_new ~ Dir(alpha_3 pi), with the chains pooled over
        chain slots [first_slot, first_slot + n_slots), on the device.  The integral over Z_new is taken per draw by importance
        sampling in n_stages rounds of n_samples samples: the first round proposes from the prior, every later one from a Dirichlet
        fitted to the weighted moments of the round before; the results are the last round's.  K-fold cross-validation is a fit per
        fold and the sum of the folds' "elpd".
        Y_new: a list of 1-D arrays with time_new (spline samplers) or basis_new (a list of n_i x P matrices; samplers created from a
        basis), or an (m, P) matrix (multivariate model).  X_new: (m, D), required exactly when covariates are set.  perm: `align`'s
        "perm" of the same slots, which relabels the membership columns (default: the labels as they are, which only means something
        where no chain switches labels); "lpd" and the ESS do not depend on it.  z_samples: (C, S, J, K) memberships that take the
        place of the stage-0 samples of every curve (n_stages must be 1; the deterministic hook of the tests).
        Returns {"lpd": (m,), "elpd": sum lpd, "se_elpd": sqrt(m var(lpd)), "Z_mean": (m, K), "Z_sd": (m, K), the sd of the whole
        predictive law, "ess_mean", "ess_min": (m,), the importance-sampling effective sample size of the last round over the draws,
        "n_samples", "n_stages"}.  A curve whose ess_min is small against n_samples (below 10, say) is not to be trusted: raise
        n_stages or n_samples.  trace adds "lpd_trace", "ess_trace": (m, C, S), "Z_trace": (m, C, S, K) and "proposal": (m, C, S, R, K);
        return_samples adds "samples": (m, C, S, R, J, K), for small shapes.
        The keyword proposal="laplace" (bfmmm_chain_predict_laplace) takes the same integral in one round of n_samples samples from
        a mixture of Student-t components at the modes of the integrand over the log-ratios of Z_new, found by a damped Newton search
        from K + 1 starts, with a defensive component at the prior: n_stages other than its default, z_samples and return_samples are
        refused.  The result then holds "n_modes_mean": (m,), the modes kept per draw ("n_stages" is 1), and trace adds "n_modes":
        (m, C, S), "components": (m, C, S, K + 2, d + d (d + 1) / 2 + 2) -- centre, L packed by rows, g_c and J_c of component c, d = K - 1
        -- and "eta_samples": (m, C, S, J, d) in place of "proposal"."""
        return self._predict_call(None, Y_new, time_new, basis_new, X_new, perm, n_samples, n_stages, seed, trace, z_samples,
                                  return_samples, first_slot, n_slots, max_workspace_bytes)

    def _predict_laplace(self, Y_new, time_new, basis_new, X_new, perm, n_samples, seed, trace, first_slot, n_slots, max_workspace_bytes):
        """predict(..., proposal="laplace")"""
        return self._predict_call(None, Y_new, time_new, basis_new, X_new, perm, n_samples, 1, seed, trace, None, False, first_slot, n_slots,
                                  max_workspace_bytes, laplace=True)

    def predict_fit(self, Y_new, E, time_new=None, basis_new=None, X_new=None, perm=None, probs=(0.025, 0.5, 0.975), noise=False,
                    n_samples=256, n_stages=3, seed=1, trace=False, z_samples=None, first_slot=0, n_slots=None, max_workspace_bytes=0):
        """Held-out, partly observed curves completed (bfmmm_chain_predict_fit): `predict` with the same arguments --
        the same samples and the same "lpd", "Z_mean", "Z_sd" and ESS, bit for bit -- and, on the rows of the evaluation basis E
        (G x P, rows in the sampler's basis as in `curve_bands`; the identity for the multivariate model), where each new curve runs
        given the points it was observed at: the predictive mean function, the sd of its predictive law and pointwise quantile
        bands, with the chains pooled on the device.  For K-fold cross-validation E holds the basis rows of the left-out points.
        The parameter draws are pooled with equal weights, as "Z_mean" pools them: the new curve does not reweight them.  noise
        adds the observation noise sigma^2 to the variance and sigma eps to the paths (bands for a new observation, not for the
        function).  probs: up to 16 probabilities, () for none.
        Returns `predict`'s dict and "mean", "sd": (m, G), "quantiles": (m, G, nq), "probs"; trace adds `predict`'s traces and
        "mean_trace", "var_trace", "path_trace": (m, G, C, S), the per-draw mean, variance and sampled path; "path_index", "path_u":
        (m, C, S), the sample j* the path took and the uniform that chose it; "path_xi": (m, C, S, M), its standard normals."""
        Em = self._basis_arg(E, "E")
        fit = {"E": Em, "probs": _probs_arg(probs), "noise": bool(noise)}
        return self._predict_call(fit, Y_new, time_new, basis_new, X_new, perm, n_samples, n_stages, seed, trace, z_samples, False,
                                  first_slot, n_slots, max_workspace_bytes)

    def _predict_call(self, fit, Y_new, time_new, basis_new, X_new, perm, n_samples, n_stages, seed, trace, z_samples, return_samples,
                      first_slot, n_slots, max_workspace_bytes, laplace=False):
        """The arguments of `predict` marshalled and bfmmm_chain_predict called, or with fit = {"E", "probs", "noise"}
        bfmmm_chain_predict_fit"""
        S = self._slots(first_slot, n_slots)
        Cn, K, J, R = self.n_chains, self.K, int(n_samples), int(n_stages)
        y = t = B = off = None
        if self.offsets is None:
            y = np.asfortranarray(Y_new, dtype=np.float64)
            if y.ndim != 2 or y.shape[1] != self.P:
                raise ValueError(f"Y_new must be an (m, {self.P}) matrix")
            m = y.shape[0]
            if time_new is not None or basis_new is not None:
                raise ValueError("the multivariate model takes Y_new alone")
        else:
            m = len(Y_new)
            off = np.zeros(m + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(v) for v in Y_new])
            cat = lambda vs, w: np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, w) for v in vs], axis=0)) \
                if m else np.zeros((0, w))
            y = cat(Y_new, 1).reshape(-1)
            if basis_new is not None:
                if any(np.shape(b) != (len(v), self.P) for b, v in zip(basis_new, Y_new)) or len(basis_new) != m:
                    raise ValueError(f"basis_new must hold one n_i x {self.P} matrix per new curve")
                B = cat(basis_new, self.P)
            if time_new is not None:
                if len(time_new) != m or any(len(a) != len(v) for a, v in zip(time_new, Y_new)):
                    raise ValueError("time_new must hold one array per new curve, as long as the curve")
                t = cat(time_new, 1).reshape(-1)
        Xm = None
        if X_new is not None:
            Xm = np.asfortranarray(X_new, dtype=np.float64)
            if Xm.ndim != 2 or Xm.shape[0] != m or (self.D > 0 and Xm.shape[1] != self.D):
                raise ValueError(f"X_new must be an ({m}, {self.D}) matrix")
        p = None if perm is None else self._perm_arg(perm, S)
        zs = None
        if z_samples is not None:
            zs = np.ascontiguousarray(z_samples, dtype=np.float64)
            if zs.shape != (Cn, S, J, K):
                raise ValueError(f"z_samples must have shape ({Cn}, {S}, {J}, {K}): (chains, slots, n_samples, K)")
        Sn = max(S, 0)
        out = {"lpd": np.zeros(m), "Z_mean": np.zeros((m, K)), "Z_sd": np.zeros((m, K)), "ess_mean": np.zeros(m), "ess_min": np.zeros(m)}
        tr = {}
        if trace:
            tr = {"lpd_trace": np.zeros((m, Cn, Sn)), "ess_trace": np.zeros((m, Cn, Sn)), "Z_trace": np.zeros((m, Cn, Sn, K))}
            if not laplace:
                tr["proposal"] = np.zeros((m, Cn, Sn, max(R, 0), K))
        if return_samples:
            tr["samples"] = np.zeros((m, Cn, Sn, max(R, 0), max(J, 0), K))
        opt = lambda k: _dp(tr[k]) if k in tr else None
        head = (self.h, None if y is None else _dp(y), None if t is None else _dp(t), None if B is None else _dp(B),
                None if off is None else off.ctypes.data_as(_lib.c_int64_p), m, None if Xm is None else _dp(Xm),
                None if p is None else _ip(p), int(first_slot), S, J, R, int(seed), None if zs is None else _dp(zs))
        pooled = (_dp(out["lpd"]), _dp(out["Z_mean"]), _dp(out["Z_sd"]), _dp(out["ess_mean"]), _dp(out["ess_min"]))
        traces = (opt("lpd_trace"), opt("Z_trace"), opt("ess_trace"), opt("proposal"), opt("samples"))
        if laplace:
            d = K - 1
            n_modes = np.zeros((m, Cn, Sn), dtype=np.int32)
            if trace:
                tr["components"] = np.zeros((m, Cn, Sn, K + 2, d + d * (d + 1) // 2 + 2))
                tr["eta_samples"] = np.zeros((m, Cn, Sn, max(J, 0), d))
            _lib.check(self.lib.bfmmm_chain_predict_laplace(*head[:11], int(seed), int(max_workspace_bytes), *pooled, *traces[:3], _ip(n_modes),
                                                            opt("components"), opt("eta_samples"), m))
            out["n_modes_mean"] = n_modes.mean(axis=(1, 2)) if Cn * Sn > 0 else np.zeros(m)
            if trace:
                tr["n_modes"] = n_modes
        elif fit is None:
            _lib.check(self.lib.bfmmm_chain_predict(*head, int(max_workspace_bytes), *pooled, *traces, m))
        else:
            Em, pr = fit["E"], fit["probs"]
            G = Em.shape[0]
            out.update(mean=np.zeros((m, G)), sd=np.zeros((m, G)), quantiles=np.zeros((m, G, pr.size)), probs=pr)
            if trace:
                tr.update(mean_trace=np.zeros((m, G, Cn, Sn)), var_trace=np.zeros((m, G, Cn, Sn)), path_trace=np.zeros((m, G, Cn, Sn)),
                          path_index=np.zeros((m, Cn, Sn), dtype=np.int32), path_u=np.zeros((m, Cn, Sn)),
                          path_xi=np.zeros((m, Cn, Sn, self.M)))
            _lib.check(self.lib.bfmmm_chain_predict_fit(
                *head, _dp(Em), G, int(fit["noise"]), _dp(pr) if pr.size else None, pr.size, int(max_workspace_bytes), *pooled,
                _dp(out["mean"]), _dp(out["sd"]), _dp(out["quantiles"]) if pr.size else None, *traces, opt("mean_trace"),
                opt("var_trace"), opt("path_trace"), _ip(tr["path_index"]) if trace else None, opt("path_u"), opt("path_xi"), m))
        out.update(tr)
        out["elpd"] = float(np.sum(out["lpd"]))
        out["se_elpd"] = float(np.sqrt(m * np.var(out["lpd"]))) if m > 0 else 0.0
        out["n_samples"], out["n_stages"] = J, R
        return out

    def _mean_eigenfunctions(self, Em, perm, wv, J, xv, first_slot, n_slots, max_workspace_bytes):
        """(K, J, G): the J leading w-eigenfunctions of the posterior mean surfaces C^(k,k), numpy.linalg.eigh of
        sqrt(w) C sqrt(w)' on the host, each signed so that its entry of largest |sqrt(w) psi| (lowest g on ties) is positive"""
        K, G = self.K, Em.shape[0]
        cm = self.cluster_cov_bands(Em, perm, pairs=[(k, k) for k in range(K)], x=xv, probs=(), first_slot=first_slot, n_slots=n_slots,
                                    max_workspace_bytes=max_workspace_bytes)["mean"]
        sw = np.ones(G) if wv is None else np.sqrt(wv)
        out = np.zeros((K, J, G))
        for k in range(K):
            A = sw[:, None] * (0.5 * (cm[k] + cm[k].T)) * sw[None, :]
            _, vec = np.linalg.eigh(A)
            for j in range(min(J, G)):
                u = vec[:, G - 1 - j]
                g = int(np.argmax(np.abs(u)))                # the first of several
                u = u if u[g] >= 0 else -u
                out[k, j] = np.divide(u, sw, out=np.zeros(G), where=sw > 0)
        return out

    def curve_cov(self, E, E2=None, curves=None, sd=True, per_chain=False, diagonal=False, first_slot=0, n_slots=None,
                  max_workspace_bytes=0):
        """The pooled covariance surface of every curve: mean (and sd) over chain slots [first_slot, first_slot + n_slots) of
        every chain of the batch of C_i(g, h) = sum_m (E_g . V_im)(E2_h . V_im), the covariance function of curve i under a draw,
        computed on the device (bfmmm_chain_curve_cov).  Label- and sign-invariant, so chains pool as they are.
        E (G1 x P) and E2 (G2 x P; default: E) are rows in the sampler's basis, as in `curve_fit`.  curves: indices in any order
        (default: all n).  diagonal: only g = h, the curve's variance function (E2 must be None).  per_chain: also each chain's
        own mean.  Returns {"mean": (m, G1, G2), "sd": (m, G1, G2) if sd, "chain_mean": (m, C, G1, G2) if per_chain}; with
        diagonal the shapes are (m, G1) and (m, C, G1)."""
        E1m = self._basis_arg(E, "E")
        E2m = None if E2 is None else self._basis_arg(E2, "E2")
        S = self._slots(first_slot, n_slots)
        idx, pc, m = self._curve_list(curves)
        G1 = E1m.shape[0]
        G2 = G1 if E2m is None else E2m.shape[0]
        cell = (G1,) if diagonal else (G1, G2)
        out = {"mean": np.zeros((m,) + cell)}
        if sd:
            out["sd"] = np.zeros((m,) + cell)
        if per_chain:
            out["chain_mean"] = np.zeros((m, self.n_chains) + cell)
        _lib.check(self.lib.bfmmm_chain_curve_cov(self.h, _dp(E1m), G1, None if E2m is None else _dp(E2m), G2, int(bool(diagonal)), pc,
                                                  m if curves is not None else 0, int(first_slot), S, int(max_workspace_bytes),
                                                  _dp(out["mean"]), _dp(out["sd"]) if sd else None,
                                                  _dp(out["chain_mean"]) if per_chain else None, out["mean"].size))
        return out

    def get_basis(self):
        n_obs = int(self.offsets[-1])
        out = np.zeros((n_obs, self.P))
        _lib.check(self.lib.bfmmm_get_basis(self.h, _dp(out), out.size))
        return [out[self.offsets[i]:self.offsets[i + 1]] for i in range(self.n)]

    def debug(self, name, capacity=1 << 24):
        out = np.zeros(capacity)
        cnt = C.c_int64()
        _lib.check(self.lib.bfmmm_debug_get(self.h, name.encode(), _dp(out), capacity, C.byref(cnt)))
        return out[:cnt.value].copy()

    def dims(self):
        v = self.debug("dims", 64)
        names = ["n", "K", "P", "M", "BW", "LG", "LREC", "MD", "A", "R", "NT", "n_obs_total", "half_sum"]
        d = {k: int(x) for k, x in zip(names, v)}
        d["YY"] = float(v[13])
        d["BWP"] = int(v[14])
        return d

    DYN_NAMES = ("iter", "slot", "tt_step", "status", "slot_base", "beta", "zprep_valid", "zprep_iter", "zprep_tt", "znorm_valid",
                 "znorm_iter", "znorm_tt", "piprep_valid", "piprep_iter", "sigma2", "alpha3", "rss", "loglik")

    def dyn(self):
        """The scalars of the selected chain's device state that a hand-over between runs depends on (bfmmm_debug_get "dyn")."""
        v = self.debug("dyn", 32)
        return {k: (float(x) if k in ("beta", "sigma2", "alpha3", "rss", "loglik") else int(x)) for k, x in zip(self.DYN_NAMES, v)}

    def sweep_route(self):
        """Which sweep kernel the last `run` launched (bfmmm_debug_get "sweep_route", recorded on the host)."""
        v = self.debug("sweep_route", 8)
        return dict(kernel=("diag", "chain", "general")[int(v[0])] if v[0] >= 0 else None, targ=int(v[1]), mv=bool(v[2]),
                    direct=bool(v[3]), threads=int(v[4]))

    def curve_route(self):
        """Which instances of the per-curve kernels the last `run` took (bfmmm_debug_get "curve_route", recorded on the host):
        {"z": the last Z update, {"form": None / "standalone" / "lean" / "fused", BW, LPC, COV, KT, KEX}, "chi": the last k_curve_chi
        launch, {BW, LPC, COV, SMALL, KX, MX, mode, fuse}}."""
        v = self.debug("curve_route", 16)
        z = dict(form=(None, "standalone", "lean", "fused")[int(v[0])], BW=int(v[1]), LPC=int(v[2]), COV=bool(v[3]), KT=int(v[4]),
                 KEX=bool(v[5]))
        chi = dict(BW=int(v[6]), LPC=int(v[7]), COV=bool(v[8]), SMALL=bool(v[9]), KX=int(v[10]), MX=int(v[11]), mode=int(v[12]),
                   fuse=bool(v[13]))
        return dict(z=z, chi=chi)

    def hyper_route(self):
        """Where the scalar jobs of the last `run` rode (bfmmm_debug_get "hyper_route", recorded on the host): "hyper", the host of
        the delta / A / gamma / tau job ("chi": k_curve_chi; "lean_z": the lean k_curve_z of the bodies, k_curve_chi in the closing
        iteration; "deferred": the next iteration's k_pair_gram, k_loglik_flush for the last), "pi", the host of the pi / alpha_3 job
        ("pair_gram", "pair_gram_solo_ll": the deferred log-likelihood in a workgroup of its own, "factor"), and "pi_prepare",
        whether k_factor prepares the next iteration's pi / alpha_3 tables."""
        v = self.debug("hyper_route", 8)
        return dict(hyper=("chi", "lean_z", "deferred")[int(v[0])] if v[0] >= 0 else None,
                    pi=("pair_gram", "pair_gram_solo_ll", "factor")[int(v[1])] if v[1] >= 0 else None, pi_prepare=bool(v[2]))

    def cov_route(self):
        """What the eta / Xi block of every iteration of the last `run` launches (bfmmm_debug_get "cov_route", recorded on the
        host; covariates set): BW, LPC and DX (0: the general instance) of k_cov_group, the D instance of k_cov_w2, PP of
        k_cov_factor, NB2, NBS, NPG, the number of k_cov_group launches, do_eta, do_xi."""
        v = self.debug("cov_route", 16)
        names = ("BW", "LPC", "DX", "W2D", "PP", "NB2", "NBS", "NPG", "launches")
        out = {k: int(x) for k, x in zip(names, v)}
        out.update(do_eta=bool(v[9]), do_xi=bool(v[10]))
        return out

    def set_profile(self, enable):
        _lib.check(self.lib.bfmmm_set_profile(self.h, int(enable)))

    def timing(self, name="total"):
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(self.lib.bfmmm_get_timing(self.h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value
