#!/usr/bin/env python3
"""Times the per-curve marginal log-density of chain slots (k_chain_curve_ll) on one MI355X at the config-2
shape (n = 4096 curves of 100 points, K = 3, P = 30, M = 6) with 8 chains x 500 slots:
  - the device time of k_chain_curve_ll alone (HIP events around the launch, median of --reps after a warm-up),
  - Sampler.loo end to end (kernel + PSIS pass + the per-curve results to the host),
  - the route without it on the same draws: the get_chain copies of every chain plus api.post_curve_loglik per chain (wall
    time, and its kernel time through bfmmm_post_last_kernel_ms),
next to the time of moving Z in and the matrix out once at 6.3 TB/s.  Not the bench line.  One JSON line.

  python tests/perf/bench_curve_ll.py [--n 4096] [--chains 8] [--slots 500] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import api
    import bench
    w = bench.make_config2(n=args.n)
    C, S, n, K = args.chains, args.slots, w["n"], w["K"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=w["M"], basis_degree=w["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    for q in range(C):
        st = dict(w["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        smp.select_chain(q)
        smp.set_state(**st)
    smp.run(bf.SWEEP_WARM, S, seed=1)

    kern, wall = [], []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        loo = smp.loo()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(float(smp.debug("curve_ll_ms", 8)[0]))
    kern, wall = sorted(kern[1:]), sorted(wall[1:])

    # the route without the kernel: every chain's draws to the host, then the observation-walking pass per chain
    lib = api._lib_entry()
    B = smp.get_basis()
    t0 = time.perf_counter()
    copies_ms, post_kernel_ms = 0.0, 0.0
    mats = []
    for q in range(C):
        smp.select_chain(q)
        tc = time.perf_counter()
        ch = {nm: smp.get_chain(nm) for nm in ("nu", "Phi", "Z", "chi", "sigma_sq")}
        copies_ms += (time.perf_counter() - tc) * 1e3
        mats.append(api.post_curve_loglik(w["y"], B, ch["nu"], ch["Phi"], ch["Z"], ch["chi"], ch["sigma_sq"]))
        post_kernel_ms += lib.bfmmm_post_last_kernel_ms()
    old_ms = (time.perf_counter() - t0) * 1e3
    ll = smp.curve_loglik()
    old = np.stack(mats, axis=1)
    agree = float(np.max(np.abs(ll - old) / np.maximum(1.0, np.abs(old))))

    moved = 8.0 * n * C * S * (K + 1)
    print(json.dumps({"what": "k_chain_curve_ll", "n": n, "chains": C, "slots": S, "K": K, "P": w["P"], "M": w["M"],
                      "kernel_ms_min": kern[0], "kernel_ms_median": kern[len(kern) // 2],
                      "Z_in_matrix_out_at_6.3TBps_ms": moved / 6.3e12 * 1e3,
                      "ns_per_curve_draw": kern[len(kern) // 2] * 1e6 / (n * C * S),
                      "loo_end_to_end_ms_median": wall[len(wall) // 2],
                      "host_route_wall_ms": old_ms, "host_route_get_chain_ms": copies_ms, "host_route_kernel_ms": post_kernel_ms,
                      "worst_rel_diff_to_host_route": agree, "elpd_loo": loo["elpd_loo"], "n_khat_above": loo["n_khat_above"]}),
          flush=True)
    smp.close()


if __name__ == "__main__":
    main()
