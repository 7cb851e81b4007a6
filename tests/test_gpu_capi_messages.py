"""The full text of what the chain-slot entry points (capi_chain.hip, capi_loo.hip) answer to bad calls: one message per check, the first
message of calls that are wrong twice (the order of the checks), and the byte counts of the workspace refusals, worked out here
by the formulas of those files for the shared tiny sampler (n = 6, K = 2, M = 2, P = 5, 2 chains, T = 4)."""
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

    row7 = 8 * CS + 7 * 8                       # seven_stats in the LDS tier: the row and its seven statistics
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
