"""The full text of what the chain-slot entry points (capi_chain.hip, capi_cluster.hip, capi_loo.hip) answer to bad calls: one message
per check, the first message of calls that are wrong twice (the order of the checks), and the byte counts of the workspace refusals,
worked out here by the formulas of those files for the shared tiny sampler (n = 6, K = 2, M = 2, P = 5, 2 chains, T = 4).  Of the
cluster-level calls' checks three cannot be reached on it: more than 2^22 draws a row, more than 8 covariates (set_covariates
refuses them first) and a model without eigenfunctions."""
import ctypes as C

import numpy as np
import pytest

from tiny_sampler import K, M, N, NCH, P, T, basis_rows, make_tiny

pytestmark = pytest.mark.gpu

G = 3
CS = NCH * T                       # draws per row over all slots


@pytest.fixture(scope="module")
def smp():
    s = make_tiny(run=True)
    yield s
    s.close()


def _fit_shared(m, which=1, D=0):
    """E's projection table, E, 16 doubles and the curve list padded to an even count (fit_shared_bytes)"""
    NJ = K * ((M + 1) if which else 1) * (1 + D)
    return 8 * (CS * G * NJ + G * P + 16) + 4 * ((m + 1) & ~1)


def _cov_table_doubles(G1):
    """cov_table_doubles without covariates: C S KP GP RS with RS = 4 ceil(M / 4) + 2, GP = G1 rounded up to 16 and KP = K
    where all K components fit one stage (K (16 + 16) RS <= 5120)"""
    RS = 4 * ((M + 3) // 4) + 2
    assert K * 32 * RS <= 5120
    return CS * K * ((G1 + 15) // 16 * 16) * RS


def _cases(smp):
    """(label, call returning the library's status, expected message)"""
    from bayesfmmm_amd import _lib
    lib, h = smp.lib, smp.h
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    E = basis_rows(smp, 2 * G)
    pe, pe2 = E[:G].ctypes.data_as(dp), E[G:].ctypes.data_as(dp)
    buf = [np.zeros(4096) for _ in range(7)]
    o = [b.ctypes.data_as(dp) for b in buf]
    probs = np.array([0.025, 0.5, 0.975] + [0.5] * 14)
    pp = probs.ctypes.data_as(dp)
    bad_probs = np.array([0.5, 1.5])
    keep = {"E": E, "buf": buf, "probs": probs, "bad_probs": bad_probs}

    def idx(v):
        a = np.array(v, dtype=np.int32)
        keep[len(keep)] = a
        return a.ctypes.data_as(ip)

    diag = lambda name, first, S, budget, cap: lambda: lib.bfmmm_chain_diagnostics(h, name, first, S, budget, *o, cap)
    cll = lambda first, S, cap: lambda: lib.bfmmm_chain_curve_loglik(h, first, S, o[0], cap)
    cdiag = lambda first, S, budget, cap: lambda: lib.bfmmm_chain_curve_diagnostics(h, first, S, budget, *o, cap)
    loo = lambda first, S, budget, cap: lambda: lib.bfmmm_chain_loo(h, first, S, budget, *o[:6], cap)
    fit = lambda which, g, cur, nc, first, S, cap: lambda: lib.bfmmm_chain_curve_fit(h, which, pe, g, cur, nc, first, S, o[0], cap)
    bands = lambda which, cur, nc, first, S, pr, nq, budget, cap: lambda: lib.bfmmm_chain_curve_bands(
        h, which, pe, G, cur, nc, first, S, pr, nq, budget, o[0], o[1], o[2], cap)
    sim = lambda cur, nc, first, S, alpha, budget, cap: lambda: lib.bfmmm_chain_curve_bands_sim(
        h, 1, pe, G, cur, nc, first, S, alpha, budget, o[0], o[1], o[2], o[3], o[4], cap)
    simil = lambda cur, nc, first, S, budget, sd, cm, cap: lambda: lib.bfmmm_chain_similarity(
        h, cur, nc, first, S, budget, o[0], o[1] if sd else None, o[2] if cm else None, cap)
    cov = lambda e2, g2, dg, cur, nc, first, S, budget, sd, cm, cap: lambda: lib.bfmmm_chain_curve_cov(
        h, pe, G, e2, g2, dg, cur, nc, first, S, budget, o[0], o[1] if sd else None, o[2] if cm else None, cap)

    row7 = 8 * CS + 7 * 8                       # a RowCall in the LDS tier: the row and its seven statistics
    bands_pc = 8 * G * (2 + 3)                  # rows sorted in LDS: mean, sd and three quantiles of G grid points
    sim_pc = 8 * (4 * G + 1)                    # mean, sd, lower, upper of G grid points and crit
    cov_sh = 8 * (_cov_table_doubles(G) + G * P)
    cov_sh2 = 8 * (2 * _cov_table_doubles(G) + 2 * G * P) + 4 * 2      # E2 given, a list of one curve
    cov_pc = 8 * G * G * (1 + 1 + NCH)
    fn = "bfmmm_chain_"
    cases = [
        ("diag first_slot", diag(b"nu", T, 1, 0, K * P), fn + "diagnostics: 'first_slot' out of range"),
        ("diag first_slot + budget", diag(b"nu", -1, 1, -1, K * P), fn + "diagnostics: 'first_slot' out of range"),
        ("diag budget + name", diag(b"nope", 0, T, -1, 1), fn + "diagnostics: 'max_workspace_bytes' must not be negative"),
        ("diag name + capacity", diag(b"nope", 0, T, 0, 0), fn + "diagnostics: unknown name 'nope'"),
        ("diag capacity", diag(b"nu", 0, T, 0, K * P - 1), fn + f"diagnostics(nu): 'capacity' below {K * P} entries"),
        ("diag budget", diag(b"nu", 0, T, row7 - 1, K * P), fn + f"diagnostics: 'max_workspace_bytes' below the {row7} bytes of one row"),
        ("curve_loglik n_slots + capacity", cll(1, T, 0), fn + "curve_loglik: 'n_slots' out of range (first_slot + n_slots > T)"),
        ("curve_loglik capacity", cll(0, T, N * CS - 1), fn + f"curve_loglik: 'capacity' below {N * CS} entries"),
        ("curve_diag budget + capacity", cdiag(0, T, -1, N - 1), fn + "curve_diagnostics: 'max_workspace_bytes' must not be negative"),
        ("curve_diag capacity", cdiag(0, T, 0, N - 1), fn + f"curve_diagnostics: 'capacity' below {N} entries"),
        ("curve_diag budget", cdiag(0, T, row7 - 1, N), fn + f"curve_diagnostics: 'max_workspace_bytes' below the {row7} bytes of one row"),
        ("loo first_slot + budget", loo(T, 1, -1, N), fn + "loo: 'first_slot' out of range"),
        ("loo budget + capacity", loo(0, T, -1, 0), fn + "loo: 'max_workspace_bytes' must not be negative"),
        ("loo budget", loo(0, T, 8 * CS - 1, N), fn + f"loo: 'max_workspace_bytes' below the {8 * CS} bytes of one row"),
        ("fit which + curves", fit(2, G, idx([N]), 1, 0, T, 4096), fn + "curve_fit: 'which' must be 0 (mean) or 1 (fit), got 2"),
        ("fit G + n_curves", fit(1, 0, idx([0]), 0, 0, T, 4096), fn + "curve_fit: 'G' must be at least 1"),
        ("fit n_curves + first_slot", fit(1, G, idx([0]), 0, T, 1, 4096), fn + "curve_fit: 'n_curves' must be at least 1 where 'curves' is given"),
        ("fit curves + first_slot", fit(1, G, idx([0, N]), 2, -1, 1, 4096), fn + f"curve_fit: 'curves'[1] = {N} outside 0 .. {N - 1}"),
        ("fit n_slots + capacity", fit(1, G, None, 0, 0, T + 1, 0), fn + "curve_fit: 'n_slots' out of range (first_slot + n_slots > T)"),
        ("fit capacity", fit(1, G, idx([3, 1]), 2, 0, T, 2 * G * CS - 1), fn + f"curve_fit: 'capacity' below {2 * G * CS} entries"),
        ("bands curves + nq", bands(1, idx([-1]), 1, 0, T, pp, 17, 0, 4096), fn + f"curve_bands: 'curves'[0] = -1 outside 0 .. {N - 1}"),
        ("bands nq + budget", bands(1, None, 0, 0, T, pp, 17, -1, 4096), fn + "curve_bands: 'nq' outside 1 .. 16"),
        ("bands probs + budget", bands(1, None, 0, 0, T, bad_probs.ctypes.data_as(dp), 2, -1, 4096), fn + "curve_bands: 'probs'[1] outside [0, 1]"),
        ("bands budget + capacity", bands(1, None, 0, 0, T, pp, 3, -1, 0), fn + "curve_bands: 'max_workspace_bytes' must not be negative"),
        ("bands capacity", bands(1, None, 0, 0, T, pp, 3, 0, N * G - 1), fn + f"curve_bands: 'capacity' below {N * G} rows"),
        ("bands budget", bands(1, None, 0, 0, T, pp, 3, _fit_shared(N) + bands_pc - 1, N * G),
         fn + f"curve_bands: 'max_workspace_bytes' below the {_fit_shared(N) + bands_pc} bytes one curve needs ({_fit_shared(N)} shared by all curves + {bands_pc} per curve)"),
        ("bands budget, mean of three curves", bands(0, idx([5, 0, 2]), 3, 0, T, pp, 3, 1, 3 * G),
         fn + f"curve_bands: 'max_workspace_bytes' below the {_fit_shared(3, 0) + bands_pc} bytes one curve needs ({_fit_shared(3, 0)} shared by all curves + {bands_pc} per curve)"),
        ("sim first_slot + alpha", sim(None, 0, T, 1, 2.0, 0, 4096), fn + "curve_bands_sim: 'first_slot' out of range"),
        ("sim alpha + budget", sim(None, 0, 0, T, 1.0, -1, 4096), fn + "curve_bands_sim: 'alpha' must be inside (0, 1)"),
        ("sim budget + capacity", sim(None, 0, 0, T, 0.05, -1, 0), fn + "curve_bands_sim: 'max_workspace_bytes' must not be negative"),
        ("sim capacity", sim(None, 0, 0, T, 0.05, 0, N * G - 1), fn + f"curve_bands_sim: 'capacity' below {N * G} rows"),
        ("sim budget", sim(None, 0, 0, T, 0.05, _fit_shared(N) + sim_pc - 1, N * G),
         fn + f"curve_bands_sim: 'max_workspace_bytes' below the {_fit_shared(N) + sim_pc} bytes one curve needs ({_fit_shared(N)} shared by all curves + {sim_pc} per curve)"),
        ("similarity n_curves + first_slot", simil(idx([0]), -1, T, 1, 0, 1, 0, 4096), fn + "similarity: 'n_curves' must not be negative"),
        ("similarity curves + first_slot", simil(idx([N + 1]), 1, -1, 1, 0, 1, 0, 4096), fn + f"similarity: 'curves'[0] = {N + 1} outside 0 .. {N - 1}"),
        ("similarity n_slots + budget", simil(None, 0, 0, 0, -1, 1, 0, 4096), fn + "similarity: 'n_slots' out of range (first_slot + n_slots > T)"),
        ("similarity budget + capacity", simil(None, 0, 0, T, -1, 1, 0, 0), fn + "similarity: 'max_workspace_bytes' must not be negative"),
        ("similarity capacity", simil(idx([1, 2]), 2, 0, T, 0, 1, 0, 2 * N - 1), fn + f"similarity: 'capacity' below {2 * N} entries"),
        ("similarity budget", simil(None, 0, 0, T, 8 * N * 2 - 1, 1, 0, N * N), fn + f"similarity: 'max_workspace_bytes' below the {8 * N * 2} bytes of one row"),
        ("similarity budget, selected rows with chain means", simil(idx([1, 2]), 2, 0, T, 1, 0, 1, 2 * N),
         fn + f"similarity: 'max_workspace_bytes' below the {8 * N * (1 + NCH) + 4} bytes of one row"),
        ("cov G2 + diagonal", cov(pe2, 0, 1, None, 0, 0, T, 0, 1, 1, 4096), fn + "curve_cov: 'G2' must be at least 1 where 'E2' is given"),
        ("cov diagonal + curves", cov(pe2, G, 1, idx([N]), 1, 0, T, 0, 1, 1, 4096), fn + "curve_cov: 'diagonal' requires 'E2' to be null"),
        ("cov n_curves + first_slot", cov(None, 0, 0, None, -2, T, 1, 0, 1, 1, 4096), fn + "curve_cov: 'n_curves' must not be negative"),
        ("cov curves + budget", cov(None, 0, 0, idx([-1]), 1, 0, T, -1, 1, 1, 4096), fn + f"curve_cov: 'curves'[0] = -1 outside 0 .. {N - 1}"),
        ("cov first_slot + budget", cov(None, 0, 0, None, 0, T, 1, -1, 1, 1, 4096), fn + "curve_cov: 'first_slot' out of range"),
        ("cov budget + capacity", cov(None, 0, 0, None, 0, 0, T, -1, 1, 1, 0), fn + "curve_cov: 'max_workspace_bytes' must not be negative"),
        ("cov capacity", cov(None, 0, 1, None, 0, 0, T, 0, 1, 1, N * G - 1), fn + f"curve_cov: 'capacity' below {N * G} entries"),
        ("cov budget", cov(None, 0, 0, None, 0, 0, T, cov_sh + cov_pc - 1, 1, 1, N * G * G),
         fn + f"curve_cov: 'max_workspace_bytes' below the {cov_sh + cov_pc} bytes one curve needs ({cov_sh} shared by all curves + {cov_pc} per curve)"),
        ("cov budget, two tables and one curve", cov(pe2, G, 0, idx([4]), 1, 0, T, 1, 0, 0, G * G),
         fn + f"curve_cov: 'max_workspace_bytes' below the {cov_sh2 + 8 * G * G} bytes one curve needs ({cov_sh2} shared by all curves + {8 * G * G} per curve)"),
    ]
    return cases, keep


# ---- the cluster-level calls (capi_cluster.hip) -----------------------------------------------------------------------------------------
CL_G = 3                                 # grid rows of these calls
CL_TAB = CS * K * 16 * 4 * ((M + 3) // 4)      # ccov_table_doubles: C S K GP 4 MB with GP = G rounded up to 16
_OUT7 = ["rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd"]
_ORDER = {
    "align": "h Zref first_slot n_slots perm score capacity",
    "aligned_summary": "h name perm first_slot n_slots probs nq budget " + " ".join(_OUT7) + " quant capacity",
    "rescaled_summary": "h name mix mix_inv first_slot n_slots probs nq budget " + " ".join(_OUT7) + " quant capacity",
    "cluster_mean_bands": "h perm E G first_slot n_slots probs nq budget mean sd quant capacity",
    "cluster_mean_bands_rescaled": "h mix E G x first_slot n_slots probs nq budget mean sd quant capacity",
    "cluster_cov_bands": "h perm E1 G1 E2 G2 diagonal pairs n_pairs x first_slot n_slots probs nq alpha budget mean sd quant crit lower upper "
                         "trace capacity",
    "cluster_cov_bands_rescaled": "h mix E1 G1 E2 G2 diagonal pairs n_pairs x first_slot n_slots probs nq alpha budget mean sd quant crit lower "
                                  "upper trace capacity",
    "rescale": "h perm transform first_slot n_slots mix mix_inv curve rcond z_min n_singular capacity",
    "cluster_contrast_bands": "h mix E G w_nu w_eta R weights first_slot n_slots probs nq alpha budget mean sd quant n_positive crit lower upper "
                              "n_exceed norm_stats norm_quant trace norm_trace capacity",
    "cluster_eigen": "h perm E G w x n_functions ref first_slot n_slots probs nq budget val_diag val_quant pve_mean pve_sd pve_quant tot_mean "
                     "tot_sd tot_quant fn_mean fn_sd fn_quant val_trace fn_trace max_sweeps capacity",
}


def _row7(nq):
    """a row of the seven statistics in the LDS tier: its values, the statistics and nq quantiles (RowReducer::row_bytes)"""
    return 8 * (CS + 7 + nq)


def _row2(nq):
    """a row of mean and sd: its values, the two and nq quantiles, sorted in LDS"""
    return 8 * (CS + 2 + nq)


def _ccov_shared(band, rescaled=False, two=False, m=3):
    """the tables, the grids, 17 doubles of probs, dev and crit of the band, the labels and the pairs (ccov_call)"""
    t = 2 if two else 1
    return 8 * (t * CL_TAB + t * CL_G * P + 17 + (m * CS + m if band else 0)) + (8 * CS * K * K if rescaled else 4 * ((CS * K + 1) & ~1)) + 8 * m


def _contrast_shared(band, R, nq, KD=0):
    """the coefficient table, E, the label maps, the weights of the contrasts and of the grid, 17 doubles of probs, dev, crit and t of
    the band, the R norm rows with their seven statistics and the counts of p_sim (bfmmm_chain_cluster_contrast_bands)"""
    return (8 * (R * P * CS + CL_G * P + CS * K * K + R * (K + KD) + CL_G + 17 + (R * CS + 2 * R if band else 0)) + _row7(nq) * R +
            4 * ((R + 1) & ~1))


def _eigen_shared(J, nq, with_ref=False, w=False):
    """Q, R and ref, E, w, 16 doubles of probs, the small rows with their results, every draw's b, the status words and perm
    (bfmmm_chain_cluster_eigen)"""
    KM = K * M
    rs = 2 * KM + K
    small_ws = rs * (2 + nq) + KM * 7
    ln = K * J * CL_G
    return 8 * (P * P + (K * J * P + ln if with_ref else 0) + CL_G * P + (CL_G if w else 0) + 16 + CS * rs + small_ws + CS * K * J * P) + 4 * 2 * CS * K


def _cluster_cases(s, D):
    """the cases of the cluster-level calls on sampler s with D covariates (0: the shared tiny sampler; else covariance-adjusted)"""
    from bayesfmmm_amd import _lib
    lib, h = s.lib, s.h
    dp, ip = _lib.c_double_p, C.POINTER(C.c_int32)
    keep = []

    def d(v):
        a = np.ascontiguousarray(v, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(dp)

    def i(v):
        a = np.ascontiguousarray(v, dtype=np.int32)
        keep.append(a)
        return a.ctypes.data_as(ip)

    G = CL_G
    E = basis_rows(s, 2 * G)
    pe, pe2 = d(E[:G]), d(E[G:])
    o = [d(np.zeros(4096)) for _ in range(14)]
    io = [i(np.zeros(4096)) for _ in range(3)]
    n_sing = C.c_int64(0)
    keep.append(n_sing)
    pp = d([0.025, 0.5, 0.975] + [0.5] * 14)
    bad_pp = d([0.5, 1.5])
    perm = np.tile(np.arange(K, dtype=np.int32), (CS, 1))
    bad_perm = perm.copy()
    bad_perm[1 * T + 2] = 0                      # chain 1, slot 2 of a call over all slots
    bad_range = perm.copy()
    bad_range[1 * 2 + 1] = 0                     # the same draw of a call over slots 1 and 2
    mix = np.tile(np.eye(K), (CS, 1, 1))
    zref = np.full(N * K, 0.5)
    bad_zref = zref.copy()
    bad_zref[N + 1] = np.inf                     # curve 1, component 1
    x_ok, x_bad = d(np.zeros(max(D, 1))), d([0.0, np.nan][:max(D, 1)] if D > 1 else [np.nan])
    w_nu = np.array([1.0, -1.0])

    def caller(entry, /, **base):
        order = _ORDER[entry].split()
        base = dict(base, h=h)
        assert set(order) == set(base), (entry, set(order) ^ set(base))

        def make(**over):
            assert set(over) <= set(base), (entry, set(over) - set(base))
            a = dict(base, **over)
            return lambda: getattr(lib, "bfmmm_chain_" + entry)(*[a[k] for k in order])
        return make

    seven = dict(zip(_OUT7, o[:7]))
    common = dict(first_slot=0, n_slots=T, probs=pp, nq=3, budget=0)
    align = caller("align", Zref=d(zref), first_slot=0, n_slots=T, perm=io[0], score=o[0], capacity=CS * K)
    asum = caller("aligned_summary", name=b"nu", perm=i(perm), quant=o[7], capacity=K * P, **seven, **common)
    rsum = caller("rescaled_summary", name=b"nu", mix=d(mix), mix_inv=d(mix), quant=o[7], capacity=K * P, **seven, **common)
    mb = caller("cluster_mean_bands", perm=i(perm), E=pe, G=G, mean=o[0], sd=o[1], quant=o[2], capacity=K * G, **common)
    mbr = caller("cluster_mean_bands_rescaled", mix=d(mix), E=pe, G=G, x=None, mean=o[0], sd=o[1], quant=o[2], capacity=K * G, **common)
    ccov_args = dict(E1=pe, G1=G, E2=None, G2=0, diagonal=0, pairs=None, n_pairs=0, x=None, alpha=0.1, mean=o[0], sd=o[1], quant=o[2], crit=o[3],
                     lower=o[4], upper=o[5], trace=None, capacity=3 * G * G, **common)
    cc = caller("cluster_cov_bands", perm=i(perm), **ccov_args)
    ccr = caller("cluster_cov_bands_rescaled", mix=d(mix), **ccov_args)
    resc = caller("rescale", perm=None, transform=None, first_slot=0, n_slots=T, mix=o[0], mix_inv=o[1], curve=io[0], rcond=o[2], z_min=o[3],
                  n_singular=C.byref(n_sing), capacity=CS * K * K)
    con = caller("cluster_contrast_bands", mix=d(mix), E=pe, G=G, w_nu=d(w_nu), w_eta=None, R=1, weights=None, alpha=0.1, mean=o[0], sd=o[1],
                 quant=o[2], n_positive=io[0], crit=o[3], lower=o[4], upper=o[5], n_exceed=io[1], norm_stats=o[6], norm_quant=o[7], trace=None,
                 norm_trace=None, capacity=G, **common)
    eig = caller("cluster_eigen", perm=i(perm), E=pe, G=G, w=None, x=None, n_functions=1, ref=None, val_diag=o[0], val_quant=o[1], pve_mean=o[2],
                 pve_sd=o[3], pve_quant=o[4], tot_mean=o[5], tot_sd=o[6], tot_quant=o[7], fn_mean=o[8], fn_sd=o[9], fn_quant=o[10], val_trace=None,
                 fn_trace=None, max_sweeps=io[2], capacity=K * G, **common)

    fn = "bfmmm_chain_"
    first, slots, neg = "'first_slot' out of range", "'n_slots' out of range (first_slot + n_slots > T)", "'max_workspace_bytes' must not be negative"
    not_perm = f"'perm' of chain 1, slot 2 is not a permutation of 0 .. {K - 1}"
    one_row = lambda name, b: fn + f"{name}: 'max_workspace_bytes' below the {b} bytes of one row"
    rows = lambda name, sh, per: fn + f"{name}: 'max_workspace_bytes' below the {sh + per} bytes one row needs ({sh} shared by all rows + {per} per row)"
    if D:
        # what only a sampler with covariates reaches: an entry of x or of w_eta that is not finite, and the checks on either side
        w_eta_bad = np.zeros((1, K, D))
        w_eta_bad[0, 1, D - 1] = np.nan
        return [
            ("mean_bands_rescaled x finite", mbr(x=x_bad), fn + f"cluster_mean_bands_rescaled: 'x'[{D - 1}] is not finite"),
            ("mean_bands_rescaled x finite + capacity", mbr(x=x_bad, capacity=0), fn + f"cluster_mean_bands_rescaled: 'x'[{D - 1}] is not finite"),
            ("mean_bands_rescaled budget + x finite", mbr(x=x_bad, budget=-1), fn + "cluster_mean_bands_rescaled: " + neg),
            ("cov_bands x finite", cc(x=x_bad), fn + f"cluster_cov_bands: 'x'[{D - 1}] is not finite"),
            ("cov_bands pairs + x finite", cc(x=x_bad, pairs=i([0, K]), n_pairs=1), fn + f"cluster_cov_bands: 'pairs'[0] = (0, {K}) outside 0 .. {K - 1}"),
            ("cov_bands x finite + first_slot", cc(x=x_bad, first_slot=T), fn + f"cluster_cov_bands: 'x'[{D - 1}] is not finite"),
            ("cov_bands_rescaled x finite", ccr(x=x_bad), fn + f"cluster_cov_bands_rescaled: 'x'[{D - 1}] is not finite"),
            ("cov_bands budget with x", cc(x=x_ok, budget=1, crit=None, lower=None, upper=None),
             rows("cluster_cov_bands", _ccov_shared(False) + 8 * D, _row2(3))),
            ("eigen x finite", eig(x=x_bad), fn + f"cluster_eigen: 'x'[{D - 1}] is not finite"),
            ("eigen w + x finite", eig(x=x_bad, w=d([1.0, -1.0, 1.0])), fn + "cluster_eigen: 'w'[1] is negative or not finite"),
            ("eigen x finite + fn_mean", eig(x=x_bad, fn_mean=None), fn + f"cluster_eigen: 'x'[{D - 1}] is not finite"),
            ("contrast w_eta finite", con(w_eta=d(w_eta_bad)), fn + f"cluster_contrast_bands: 'w_eta'[0, 1, {D - 1}] is not finite"),
            ("contrast w_nu finite + w_eta finite", con(w_nu=d([1.0, np.inf]), w_eta=d(w_eta_bad)), fn + "cluster_contrast_bands: 'w_nu'[0, 1] is not finite"),
            ("contrast w_eta finite + weights", con(w_eta=d(w_eta_bad), weights=d([1.0, -1.0, 1.0])),
             fn + f"cluster_contrast_bands: 'w_eta'[0, 1, {D - 1}] is not finite"),
            ("contrast no weight, w_eta zero", con(w_nu=d([0.0, 0.0]), w_eta=d(np.zeros((1, K, D)))),
             fn + "cluster_contrast_bands: contrast 0 has no weight other than zero"),
            ("contrast budget with w_eta", con(w_eta=d(np.ones((1, K, D))), budget=1),
             rows("cluster_contrast_bands", _contrast_shared(True, 1, 3, K * D), _row2(3) + 8)),
        ], keep

    cases = [
        # ---- bfmmm_chain_align
        ("align null", align(Zref=None), fn + "align: 'Zref' is null"),
        ("align null + first_slot", align(perm=None, first_slot=-1), fn + "align: 'perm' is null"),
        ("align first_slot + capacity", align(first_slot=T, n_slots=1, capacity=0), fn + "align: " + first),
        ("align n_slots + capacity", align(first_slot=1, capacity=0), fn + "align: " + slots),
        ("align capacity + Zref", align(capacity=CS * K - 1, Zref=d(bad_zref)), fn + f"align: 'capacity' below {CS * K} entries"),
        ("align Zref", align(Zref=d(bad_zref)), fn + "align: 'Zref'[1, 1] is not finite"),
        # ---- bfmmm_chain_aligned_summary
        ("aligned_summary null + first_slot", asum(perm=None, first_slot=T), fn + "aligned_summary: 'perm' is null"),
        ("aligned_summary first_slot + budget", asum(first_slot=-1, n_slots=1, budget=-1), fn + "aligned_summary: " + first),
        ("aligned_summary budget + name", asum(name=b"nope", budget=-1), fn + "aligned_summary: " + neg),
        ("aligned_summary name + capacity", asum(name=b"nope", capacity=0), fn + "aligned_summary: unknown name 'nope'"),
        ("aligned_summary capacity + nq", asum(capacity=K * P - 1, nq=17), fn + f"aligned_summary(nu): 'capacity' below {K * P} entries"),
        ("aligned_summary nq + perm", asum(nq=-1, perm=i(bad_perm)), fn + "aligned_summary: 'nq' outside 0 .. 16"),
        ("aligned_summary quant null + perm", asum(quant=None, perm=i(bad_perm)), fn + "aligned_summary: 'quant' is null"),
        ("aligned_summary probs + perm", asum(probs=bad_pp, nq=2, perm=i(bad_perm)), fn + "aligned_summary: 'probs'[1] outside [0, 1]"),
        ("aligned_summary perm + budget", asum(perm=i(bad_perm), budget=1), fn + "aligned_summary: " + not_perm),
        ("aligned_summary perm of a slot range", asum(perm=i(bad_range), first_slot=1, n_slots=2), fn + "aligned_summary: " + not_perm),
        ("aligned_summary budget", asum(budget=_row7(3) - 1), one_row("aligned_summary", _row7(3))),
        ("aligned_summary budget, no quantiles", asum(nq=0, probs=None, quant=None, budget=1), one_row("aligned_summary", _row7(0))),
        # ---- bfmmm_chain_rescaled_summary
        ("rescaled_summary null + first_slot", rsum(mix_inv=None, first_slot=T), fn + "rescaled_summary: 'mix_inv' is null"),
        ("rescaled_summary n_slots + budget", rsum(n_slots=0, budget=-1), fn + "rescaled_summary: " + slots),
        ("rescaled_summary budget + name", rsum(name=b"pi", budget=-1), fn + "rescaled_summary: " + neg),
        ("rescaled_summary no rescale + capacity", rsum(name=b"pi", capacity=0),
         fn + "rescaled_summary: the reference defines no rescale for 'pi' (only for nu, Phi, eta, xi and Z)"),
        ("rescaled_summary no array + capacity", rsum(name=b"eta", capacity=0),
         fn + "rescaled_summary: no array 'eta' (covariate arrays exist once covariates were set)"),
        ("rescaled_summary capacity + nq", rsum(name=b"Z", capacity=N * K - 1, nq=17), fn + f"rescaled_summary(Z): 'capacity' below {N * K} entries"),
        ("rescaled_summary nq + budget", rsum(nq=17, budget=1), fn + "rescaled_summary: 'nq' outside 0 .. 16"),
        ("rescaled_summary probs null + budget", rsum(probs=None, budget=1), fn + "rescaled_summary: 'probs' is null"),
        ("rescaled_summary probs + budget", rsum(probs=bad_pp, nq=2, budget=1), fn + "rescaled_summary: 'probs'[1] outside [0, 1]"),
        ("rescaled_summary budget", rsum(budget=_row7(3) - 1), one_row("rescaled_summary", _row7(3))),
        # ---- bfmmm_chain_cluster_mean_bands
        ("mean_bands null + G", mb(E=None, G=0), fn + "cluster_mean_bands: 'E' is null"),
        ("mean_bands G + first_slot", mb(G=0, first_slot=T), fn + "cluster_mean_bands: 'G' must be at least 1"),
        ("mean_bands first_slot + budget", mb(first_slot=T, n_slots=1, budget=-1), fn + "cluster_mean_bands: " + first),
        ("mean_bands budget + capacity", mb(budget=-1, capacity=0), fn + "cluster_mean_bands: " + neg),
        ("mean_bands capacity + nq", mb(capacity=K * G - 1, nq=17), fn + f"cluster_mean_bands: 'capacity' below {K * G} rows"),
        ("mean_bands nq + perm", mb(nq=17, perm=i(bad_perm)), fn + "cluster_mean_bands: 'nq' outside 0 .. 16"),
        ("mean_bands probs + perm", mb(probs=bad_pp, nq=2, perm=i(bad_perm)), fn + "cluster_mean_bands: 'probs'[1] outside [0, 1]"),
        ("mean_bands perm + budget", mb(perm=i(bad_perm), budget=1), fn + "cluster_mean_bands: " + not_perm),
        ("mean_bands budget", mb(budget=_row2(3) - 1), one_row("cluster_mean_bands", _row2(3))),
        # ---- bfmmm_chain_cluster_mean_bands_rescaled
        ("mean_bands_rescaled null + G", mbr(mix=None, G=0), fn + "cluster_mean_bands_rescaled: 'mix' is null"),
        ("mean_bands_rescaled G + n_slots", mbr(G=-1, n_slots=T + 1), fn + "cluster_mean_bands_rescaled: 'G' must be at least 1"),
        ("mean_bands_rescaled n_slots + budget", mbr(n_slots=T + 1, budget=-1), fn + "cluster_mean_bands_rescaled: " + slots),
        ("mean_bands_rescaled budget + x", mbr(budget=-1, x=x_ok), fn + "cluster_mean_bands_rescaled: " + neg),
        ("mean_bands_rescaled x + capacity", mbr(x=x_ok, capacity=0), fn + "cluster_mean_bands_rescaled: 'x' is given but the sampler has no covariates"),
        ("mean_bands_rescaled capacity + nq", mbr(capacity=K * G - 1, nq=17), fn + f"cluster_mean_bands_rescaled: 'capacity' below {K * G} rows"),
        ("mean_bands_rescaled nq + budget", mbr(nq=17, budget=1), fn + "cluster_mean_bands_rescaled: 'nq' outside 0 .. 16"),
        ("mean_bands_rescaled quant null + budget", mbr(quant=None, budget=1), fn + "cluster_mean_bands_rescaled: 'quant' is null"),
        ("mean_bands_rescaled budget", mbr(budget=_row2(3) - 1), one_row("cluster_mean_bands_rescaled", _row2(3))),
        # ---- bfmmm_chain_cluster_cov_bands and its rescaled form
        ("cov_bands null + G1", cc(perm=None, G1=0), fn + "cluster_cov_bands: 'perm' is null"),
        ("cov_bands_rescaled null + G1", ccr(mix=None, G1=0), fn + "cluster_cov_bands_rescaled: 'mix' is null"),
        ("cov_bands G1 + G2", cc(G1=0, E2=pe2, G2=0), fn + "cluster_cov_bands: 'G1' must be at least 1"),
        ("cov_bands G2 + diagonal", cc(E2=pe2, G2=0, diagonal=1), fn + "cluster_cov_bands: 'G2' must be at least 1 where 'E2' is given"),
        ("cov_bands diagonal + n_pairs", cc(E2=pe2, G2=G, diagonal=1, n_pairs=-1), fn + "cluster_cov_bands: 'diagonal' requires 'E2' to be null"),
        ("cov_bands n_pairs + pairs", cc(pairs=i([0, K]), n_pairs=-1), fn + "cluster_cov_bands: 'n_pairs' must not be negative"),
        ("cov_bands pairs + x", cc(pairs=i([0, 1, -1, 0]), n_pairs=2, x=x_ok), fn + f"cluster_cov_bands: 'pairs'[1] = (-1, 0) outside 0 .. {K - 1}"),
        ("cov_bands x + first_slot", cc(x=x_ok, first_slot=T), fn + "cluster_cov_bands: 'x' is given but the sampler is not covariance-adjusted"),
        ("cov_bands_rescaled x + first_slot", ccr(x=x_ok, first_slot=T),
         fn + "cluster_cov_bands_rescaled: 'x' is given but the sampler is not covariance-adjusted"),
        ("cov_bands first_slot + budget", cc(first_slot=T, n_slots=1, budget=-1), fn + "cluster_cov_bands: " + first),
        ("cov_bands budget + capacity", cc(budget=-1, capacity=0), fn + "cluster_cov_bands: " + neg),
        ("cov_bands capacity + nq", cc(capacity=3 * G * G - 1, nq=17), fn + f"cluster_cov_bands: 'capacity' below {3 * G * G} entries"),
        ("cov_bands capacity, diagonal of one pair", cc(diagonal=1, pairs=i([1, 0]), n_pairs=1, capacity=G - 1),
         fn + f"cluster_cov_bands: 'capacity' below {G} entries"),
        ("cov_bands nq + band", cc(nq=17, crit=None), fn + "cluster_cov_bands: 'nq' outside 0 .. 16"),
        ("cov_bands probs + band", cc(probs=bad_pp, nq=2, upper=None), fn + "cluster_cov_bands: 'probs'[1] outside [0, 1]"),
        ("cov_bands band + alpha", cc(lower=None, alpha=0.0), fn + "cluster_cov_bands: 'crit', 'lower' and 'upper' must be all null or all set"),
        ("cov_bands band, crit alone + alpha", cc(lower=None, upper=None, alpha=0.0),
         fn + "cluster_cov_bands: 'crit', 'lower' and 'upper' must be all null or all set"),
        ("cov_bands alpha + perm", cc(alpha=1.0, perm=i(bad_perm)), fn + "cluster_cov_bands: 'alpha' must be inside (0, 1)"),
        ("cov_bands_rescaled alpha + budget", ccr(alpha=0.0, budget=1), fn + "cluster_cov_bands_rescaled: 'alpha' must be inside (0, 1)"),
        ("cov_bands perm + budget", cc(perm=i(bad_perm), budget=1), fn + "cluster_cov_bands: " + not_perm),
        ("cov_bands perm without the band, alpha not read", cc(perm=i(bad_perm), crit=None, lower=None, upper=None, alpha=7.0),
         fn + "cluster_cov_bands: " + not_perm),
        ("cov_bands budget", cc(budget=_ccov_shared(True) + _row2(3) - 1), rows("cluster_cov_bands", _ccov_shared(True), _row2(3))),
        ("cov_bands budget without the band", cc(budget=1, crit=None, lower=None, upper=None, nq=0, probs=None, quant=None),
         rows("cluster_cov_bands", _ccov_shared(False), _row2(0))),
        ("cov_bands budget, two tables and one pair", cc(budget=1, E2=pe2, G2=G, pairs=i([0, 1]), n_pairs=1),
         rows("cluster_cov_bands", _ccov_shared(True, two=True, m=1), _row2(3))),
        ("cov_bands_rescaled budget", ccr(budget=_ccov_shared(True, True) + _row2(3) - 1),
         rows("cluster_cov_bands_rescaled", _ccov_shared(True, True), _row2(3))),
        # ---- bfmmm_chain_rescale
        ("rescale null + first_slot", resc(rcond=None, first_slot=T), fn + "rescale: 'rcond' is null"),
        ("rescale first_slot + capacity", resc(first_slot=-1, n_slots=1, capacity=0), fn + "rescale: " + first),
        ("rescale n_slots + capacity", resc(n_slots=T + 1, capacity=0), fn + "rescale: " + slots),
        ("rescale capacity + perm", resc(capacity=CS * K * K - 1, perm=i(bad_perm)), fn + f"rescale: 'capacity' below {CS * K * K} entries"),
        ("rescale perm", resc(perm=i(bad_perm)), fn + "rescale: " + not_perm),
        # ---- bfmmm_chain_cluster_contrast_bands
        ("contrast null + G", con(w_nu=None, G=0), fn + "cluster_contrast_bands: 'w_nu' is null"),
        ("contrast G + R", con(G=0, R=0), fn + "cluster_contrast_bands: 'G' must be at least 1"),
        ("contrast R + w_eta", con(R=65, w_eta=o[8]), fn + "cluster_contrast_bands: 'R' = 65 outside 1 .. 64"),
        ("contrast w_eta + w_nu", con(w_eta=o[8], w_nu=d([np.nan, 1.0])), fn + "cluster_contrast_bands: 'w_eta' is given but the sampler has no covariates"),
        ("contrast w_nu + weights", con(w_nu=d([1.0, np.nan]), weights=d([1.0, -1.0, 1.0])), fn + "cluster_contrast_bands: 'w_nu'[0, 1] is not finite"),
        ("contrast no weight + weights", con(R=2, w_nu=d([1.0, -1.0, 0.0, 0.0]), weights=d([1.0, -1.0, 1.0]), capacity=2 * G),
         fn + "cluster_contrast_bands: contrast 1 has no weight other than zero"),
        ("contrast weights + band", con(weights=d([1.0, 1.0, np.inf]), crit=None), fn + "cluster_contrast_bands: 'weights'[2] is negative or not finite"),
        ("contrast band + alpha", con(n_exceed=None, alpha=0.0),
         fn + "cluster_contrast_bands: 'crit', 'lower', 'upper' and 'n_exceed' must be all null or all set"),
        ("contrast band, n_exceed alone + alpha", con(crit=None, lower=None, upper=None, alpha=0.0),
         fn + "cluster_contrast_bands: 'crit', 'lower', 'upper' and 'n_exceed' must be all null or all set"),
        ("contrast alpha + capacity", con(alpha=1.0, capacity=0), fn + "cluster_contrast_bands: 'alpha' must be inside (0, 1)"),
        ("contrast capacity + first_slot", con(capacity=G - 1, first_slot=T), fn + f"cluster_contrast_bands: 'capacity' below {G} rows"),
        ("contrast first_slot + budget", con(first_slot=T, n_slots=1, budget=-1), fn + "cluster_contrast_bands: " + first),
        ("contrast budget + nq", con(budget=-1, nq=17), fn + "cluster_contrast_bands: " + neg),
        ("contrast nq + norm_quant", con(nq=17, norm_quant=None), fn + "cluster_contrast_bands: 'nq' outside 0 .. 16"),
        ("contrast quant null + norm_quant", con(quant=None, norm_quant=None), fn + "cluster_contrast_bands: 'quant' is null"),
        ("contrast norm_quant + budget", con(norm_quant=None, budget=1), fn + "cluster_contrast_bands: 'norm_quant' is null"),
        ("contrast budget", con(budget=_contrast_shared(True, 1, 3) + _row2(3) + 8 - 1),
         rows("cluster_contrast_bands", _contrast_shared(True, 1, 3), _row2(3) + 8)),
        ("contrast budget, two contrasts without band and quantiles",
         con(R=2, w_nu=d([1.0, -1.0, 0.0, 1.0]), capacity=2 * G, budget=1, crit=None, lower=None, upper=None, n_exceed=None, nq=0, probs=None,
             quant=None, norm_quant=None),
         rows("cluster_contrast_bands", _contrast_shared(False, 2, 0), _row2(0) + 8)),
        # ---- bfmmm_chain_cluster_eigen
        ("eigen null + G", eig(max_sweeps=None, G=0), fn + "cluster_eigen: 'max_sweeps' is null"),
        ("eigen G + n_functions", eig(G=0, n_functions=M + 1), fn + "cluster_eigen: 'G' must be at least 1"),
        ("eigen n_functions + w", eig(n_functions=M + 1, w=d([1.0, -1.0, 1.0])), fn + f"cluster_eigen: 'n_functions' = {M + 1} outside 0 .. {M} (n_eigen)"),
        ("eigen w + x", eig(w=d([1.0, 1.0, np.nan]), x=x_ok), fn + "cluster_eigen: 'w'[2] is negative or not finite"),
        ("eigen x + fn_mean", eig(x=x_ok, fn_mean=None), fn + "cluster_eigen: 'x' is given but the sampler is not covariance-adjusted"),
        ("eigen fn_sd null + ref", eig(fn_sd=None, ref=d([0.0] * 5 + [np.inf])), fn + "cluster_eigen: 'fn_sd' is null"),
        ("eigen ref + first_slot", eig(ref=d([0.0] * 5 + [np.inf]), first_slot=T), fn + "cluster_eigen: 'ref'[5] is not finite"),
        ("eigen first_slot + budget", eig(first_slot=T, n_slots=1, budget=-1), fn + "cluster_eigen: " + first),
        ("eigen budget + capacity", eig(budget=-1, capacity=0), fn + "cluster_eigen: " + neg),
        ("eigen capacity + nq", eig(capacity=K * G - 1, nq=17), fn + f"cluster_eigen: 'capacity' below {K * G} rows"),
        ("eigen nq + pve_quant", eig(nq=17, pve_quant=None), fn + "cluster_eigen: 'nq' outside 0 .. 16"),
        ("eigen val_quant null + pve_quant", eig(val_quant=None, pve_quant=None), fn + "cluster_eigen: 'quant' is null"),
        ("eigen tot_quant null + perm", eig(tot_quant=None, perm=i(bad_perm)), fn + "cluster_eigen: 'tot_quant' is null"),
        ("eigen fn_quant null + perm", eig(fn_quant=None, perm=i(bad_perm)), fn + "cluster_eigen: 'fn_quant' is null"),
        ("eigen perm + budget", eig(perm=i(bad_perm), budget=1), fn + "cluster_eigen: " + not_perm),
        ("eigen budget", eig(budget=_eigen_shared(1, 3) + _row2(3) - 1), rows("cluster_eigen", _eigen_shared(1, 3), _row2(3))),
        ("eigen budget, two functions with ref and w", eig(n_functions=2, ref=d(np.ones(K * 2 * G)), w=d([1.0, 2.0, 0.0]), capacity=K * 2 * G, budget=1),
         rows("cluster_eigen", _eigen_shared(2, 3, with_ref=True, w=True), _row2(3))),
        ("eigen budget, no functions", eig(n_functions=0, fn_mean=None, fn_sd=None, fn_quant=None, capacity=0, budget=1),
         fn + f"cluster_eigen: 'max_workspace_bytes' below the {_eigen_shared(0, 3)} bytes one row needs ({_eigen_shared(0, 3)} shared by all rows + 0 per row)"),
    ]
    return cases, keep


def _run_cases(lib, cases):
    assert len({label for label, _, _ in cases}) == len(cases)
    wrong = []
    for label, call, want in cases:
        rc = call()
        got = lib.bfmmm_last_error().decode() if rc else "(the call succeeded)"
        if got != want:
            wrong.append((label, got, want))
    assert not wrong, wrong


def test_full_messages_of_the_cluster_level_calls(smp):
    cases, keep = _cluster_cases(smp, 0)
    _run_cases(smp.lib, cases)


def test_full_messages_of_the_cluster_level_calls_with_covariates():
    """the checks that only a sampler with covariates reaches: the same tiny sampler with D = 2, covariance-adjusted"""
    s = make_tiny(D=2, covariance_adj=True, run=True)
    try:
        cases, keep = _cluster_cases(s, 2)
        _run_cases(s.lib, cases)
    finally:
        s.close()


def test_full_messages(smp):
    cases, keep = _cases(smp)
    assert len({label for label, _, _ in cases}) == len(cases)
    wrong = []
    for label, call, want in cases:
        rc = call()
        got = smp.lib.bfmmm_last_error().decode() if rc else "(the call succeeded)"
        if got != want:
            wrong.append((label, got, want))
    assert not wrong, wrong


def test_the_budget_at_the_bound_is_accepted(smp):
    """one byte more than the refused budgets above: the calls run, one curve (one row) per chunk"""
    E = basis_rows(smp, G)
    smp.curve_bands(E, max_workspace_bytes=_fit_shared(N) + 8 * G * 5)
    assert smp.timing("curve_fit_rows")[1] == N
    smp.curve_bands_simultaneous(E, max_workspace_bytes=_fit_shared(N) + 8 * (4 * G + 1))
    assert smp.timing("curve_sim")[1] == N
    smp.curve_cov(E, per_chain=True, max_workspace_bytes=8 * (_cov_table_doubles(G) + G * P) + 8 * G * G * (2 + NCH))
    assert smp.timing("curve_cov")[1] == N
    smp.similarity(max_workspace_bytes=8 * N * 2)
    assert smp.timing("similarity")[1] == N
