#!/usr/bin/env python3
"""Times the observation-level PSIS-LOO (kernels_loo_pointwise.hip) on one MI355X at the config-2 shape of 7d: n = 4096
curves of 100 points, K = 3, P = 30, M = 6, 8 chains x 500 slots = 4000 draws, 409 600 observations.  The chains start from the
generating state.  Reports the device time of "loo_pointwise" (the dense basis rows, k_loo_pointwise) and of "loo_pointwise_psis"
(the PSIS pass with its three expectations; HIP events, Sampler.timing) with their launch counts, the end-to-end time of
Sampler.loo_pointwise, the time the bytes of the four matrices take written once and read once at 6.3 TB/s, the distribution of
pareto_k over the observations (median, 0.9 and 0.99 quantiles, largest, share above the threshold) next to that of Sampler.loo()
over the curves of the same chains, elpd_loo of both, and the calibration of the LOO-PIT (its deciles' counts and the largest
distance of its empirical distribution from the uniform one).  Medians of --reps calls after one warm-up call on a few curves.
Not the bench line.  One JSON line.

  python tests/perf/bench_loo_pointwise.py [--n 4096] [--chains 8] [--slots 500] [--reps 3] [--max-workspace-mb 0]
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

HBM_BYTES_PER_S = 6.3e12


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def khat(res):
    k = np.asarray(res["pareto_k"])
    fin = k[np.isfinite(k)]
    return {"units": int(k.size), "median_pareto_k": float(np.median(fin)), "q90_pareto_k": float(np.quantile(fin, 0.9)),
            "q99_pareto_k": float(np.quantile(fin, 0.99)), "max_pareto_k": float(np.max(k)), "n_khat_above": int(res["n_khat_above"]),
            "share_khat_above": float(res["n_khat_above"]) / k.size, "khat_threshold": float(res["khat_threshold"]),
            "elpd_loo": float(res["elpd_loo"]), "p_loo": float(res["p_loo"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-workspace-mb", type=int, default=0)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    w2 = bench.make_config2(n=args.n)
    n, C, S, K, M, P = args.n, args.chains, args.slots, w2["K"], w2["M"], w2["P"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w2["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w2["y"], w2["t"], w2["internal_knots"], w2["boundary_knots"], n_chains=C)
    for q in range(C):
        smp.select_chain(q)
        smp.set_state(**w2["state"])
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    n_obs = int(smp.offsets[-1])
    budget = args.max_workspace_mb << 20
    smp.loo_pointwise(curves=range(8), n_slots=min(S, 24))      # warm-up: the kernels are loaded
    wall, dev, dev_psis = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = smp.loo_pointwise(max_workspace_bytes=budget)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(smp.timing("loo_pointwise")[0])
        dev_psis.append(smp.timing("loo_pointwise_psis")[0])
    matrix_bytes = 4 * 8 * n_obs * C * S
    pit = np.sort(res["pit"])
    out = {"what": "loo_pointwise", "reps": args.reps, "n": n, "K": K, "M": M, "P": P, "chains": C, "slots": S, "draws": C * S,
           "observations": n_obs, "observation_draws": n_obs * C * S, "max_workspace_bytes": budget,
           "device_ms": med(dev), "launches": smp.timing("loo_pointwise")[1], "psis_device_ms": med(dev_psis),
           "psis_launches": smp.timing("loo_pointwise_psis")[1], "end_to_end_ms": med(wall),
           "matrix_bytes": matrix_bytes, "write_once_read_once_ms_at_hbm_rate": 2 * matrix_bytes / HBM_BYTES_PER_S * 1e3,
           "pointwise": khat(res),
           "pit_decile_counts": [int(v) for v in np.histogram(pit, bins=10, range=(0.0, 1.0))[0]],
           "pit_max_distance_from_uniform": float(np.max(np.abs(pit - (np.arange(n_obs) + 0.5) / n_obs))),
           "mean_loo_sd": float(np.mean(res["sd"]))}
    t0 = time.perf_counter()
    cond = smp.loo()
    out["loo_over_curves"] = dict(khat(cond), end_to_end_ms=(time.perf_counter() - t0) * 1e3)
    smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
