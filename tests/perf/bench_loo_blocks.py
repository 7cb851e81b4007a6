#!/usr/bin/env python3
"""Times the leave-block-out PSIS cross-validation within curves (kernels_loo_blocks.hip) on one MI355X at the config-2
shape of 7d: n = 4096 curves of 100 points, K = 3, P = 30, M = 6, 8 chains x 500 slots = 4000 draws.  The chains start from the
generating state.  For block_size 1, 10 and 50 and for horizon 20 it reports the device time of "loo_blocks" (the dense basis rows,
k_loo_blocks) and of "loo_blocks_psis" (the PSIS pass with its three expectations; HIP events, Sampler.timing) with their launch
counts, the end-to-end time of Sampler.loo_blocks, the distribution of pareto_k over the blocks (median, 0.9 and 0.99 quantiles,
largest, share above the threshold), elpd_loo per listed observation and the largest distance of the pooled PIT from the uniform
distribution; and, as the yardstick, the same times of Sampler.loo_pointwise in the same session.  Medians of --reps calls after one
warm-up call on a few curves.  Not the bench line.  One JSON line.

  python tests/perf/bench_loo_blocks.py [--n 4096] [--chains 8] [--slots 500] [--reps 3] [--max-workspace-mb 0]
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

SETTINGS = (("block_size_1", {"block_size": 1}), ("block_size_10", {"block_size": 10}), ("block_size_50", {"block_size": 50}),
            ("horizon_20", {"horizon": 20}))


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
    budget = args.max_workspace_mb << 20
    out = {"what": "loo_blocks", "reps": args.reps, "n": n, "K": K, "M": M, "P": P, "chains": C, "slots": S, "draws": C * S,
           "max_workspace_bytes": budget}
    smp.loo_blocks(block_size=7, curves=range(8), n_slots=min(S, 24))      # warm-up: the kernels are loaded
    smp.loo_pointwise(curves=range(8), n_slots=min(S, 24))
    for name, kw in SETTINGS:
        wall, dev, dev_psis = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = smp.loo_blocks(max_workspace_bytes=budget, **kw)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(smp.timing("loo_blocks")[0])
            dev_psis.append(smp.timing("loo_blocks_psis")[0])
        rows = int(res["offsets"][-1])
        pit = np.sort(res["pit"])
        out[name] = dict(khat(res), rows=rows, row_draws=rows * C * S, device_ms=med(dev), launches=smp.timing("loo_blocks")[1],
                         psis_device_ms=med(dev_psis), psis_launches=smp.timing("loo_blocks_psis")[1], end_to_end_ms=med(wall),
                         device_ns_per_row_draw=med(dev) * 1e6 / (rows * C * S), elpd_loo_per_observation=float(res["elpd_loo"]) / rows,
                         pit_max_distance_from_uniform=float(np.max(np.abs(pit - (np.arange(rows) + 0.5) / rows))),
                         mean_sd=float(np.mean(res["sd"])))
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    wall, dev, dev_psis = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = smp.loo_pointwise(max_workspace_bytes=budget)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(smp.timing("loo_pointwise")[0])
        dev_psis.append(smp.timing("loo_pointwise_psis")[0])
    rows = int(res["offsets"][-1])
    out["loo_pointwise"] = dict(khat(res), rows=rows, device_ms=med(dev), psis_device_ms=med(dev_psis), end_to_end_ms=med(wall),
                                device_ns_per_row_draw=med(dev) * 1e6 / (rows * C * S), elpd_loo_per_observation=float(res["elpd_loo"]) / rows)
    smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
