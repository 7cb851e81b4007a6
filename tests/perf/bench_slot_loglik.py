#!/usr/bin/env python3
"""Times the slot log-likelihood (k_slot_rss + k_slot_ll_reduce) on one MI355X at the config-2 shape (n = 4096
curves of 100 points, K = 3, P = 30, M = 6) with 8 chains x 500 slots, medians of --reps calls after a warm-up:
  - Sampler.slot_loglik end to end (wall) and its two timers ("slot_loglik", "slot_loglik_reduce"; summed over the chunks),
  - k_chain_curve_ll's device time in the same process (Sampler.curve_loglik; PT_CURVE_LL), the sibling it shares its geometry with,
  - get_chain and set_chain of Z and Phi of one chain, in bytes per second,
next to what one read of the slots the kernel reads (Z, chi, nu, Phi, sigma^2 of every chain and slot) costs at 6.3 TB/s, and the
largest difference to the "loglik" the run stored.  Not the bench line.  One JSON line.

  python tests/perf/bench_slot_loglik.py [--n 4096] [--chains 8] [--slots 500] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    w = bench.make_config2(n=args.n)
    C, S, n, K, P, M = args.chains, args.slots, w["n"], w["K"], w["P"], w["M"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    for q in range(C):
        st = dict(w["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        smp.select_chain(q)
        smp.set_state(**st)
    smp.run(bf.SWEEP_WARM, S, seed=1)

    wall, kern, red, launches = [], [], [], 0
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        ll = smp.slot_loglik()
        wall.append((time.perf_counter() - t0) * 1e3)
        k, launches = smp.timing("slot_loglik")
        kern.append(k)
        red.append(smp.timing("slot_loglik_reduce")[0])
    stored = []
    for q in range(C):
        smp.select_chain(q)
        stored.append(smp.get_chain("loglik"))
    stored = np.stack(stored)
    N_obs = int(sum(len(y) for y in w["y"]))
    cll = []
    for _ in range(args.reps + 1):
        smp.curve_loglik()
        cll.append(float(smp.debug("curve_ll_ms", 8)[0]))

    smp.select_chain(0)
    copies = {}
    for nm in ("Z", "Phi"):
        get_ms, set_ms = [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            a = smp.get_chain(nm)
            get_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            smp.set_chain(nm, a)
            set_ms.append((time.perf_counter() - t0) * 1e3)
        copies[nm] = {"bytes": int(a.nbytes), "get_chain_GBps": a.nbytes / (_median(get_ms[1:]) * 1e-3) / 1e9,
                      "set_chain_GBps": a.nbytes / (_median(set_ms[1:]) * 1e-3) / 1e9}

    read = 8.0 * C * S * (n * K + n * M + K * P + K * P * M + 1)
    print(json.dumps({"what": "slot_loglik", "n": n, "chains": C, "slots": S, "K": K, "P": P, "M": M,
                      "end_to_end_ms_median": _median(wall[1:]), "k_slot_rss_ms_median": _median(kern[1:]),
                      "k_slot_ll_reduce_ms_median": _median(red[1:]), "chunks": int(launches),
                      "k_chain_curve_ll_ms_median": _median(cll[1:]),
                      "ns_per_curve_draw": _median(kern[1:]) * 1e6 / (n * C * S),
                      "slots_read_once_at_6.3TBps_ms": read / 6.3e12 * 1e3,
                      "worst_abs_diff_to_stored_loglik": float(np.abs(ll - stored).max()),
                      "worst_diff_in_units_of_1e-10_(|ll|+N_obs)": float((np.abs(ll - stored) / (1e-10 * (np.abs(stored) + N_obs))).max()),
                      "copies": copies}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
