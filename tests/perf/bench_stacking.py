#!/usr/bin/env python3
"""Times the stacking of predictive distributions (kernels_stacking.hip) on one MI355X on simulated columns: n = 409 600
units (the observations of the config-2 shape of 7d) and n = 4096 (its curves), Q = 8 candidates.  Per shape: the device time per
iteration (HIP events around the launches of k_stack_em, bfmmm_post_last_kernel_ms, over --iters iterations with tol = 0 and
check_every = --iters, so that the host reads nothing in between) and the wall time of that call, which also copies, prepares and
finishes; the end-to-end
time of api.stacking with its defaults (copy in, prepare, the loop to tol = 1e-8 with a read every 16 launches, pointwise, copy
back) with its iteration count; the time of reading P (n x Q doubles) once at 6.3 TB/s, what an iteration would take if bytes set
it; and the float64 numpy restatement of the same loop on the host (tests/stacking_ref.em, forward sums), per iteration and end to
end.  Medians of --reps calls after one warm-up call.  Not the bench line.  One JSON line.

  python tests/perf/bench_stacking.py [--n 409600 4096] [--Q 8] [--iters 512] [--reps 5]
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


def columns(n, Q, seed):
    """Q candidates of differing quality: a shared per-unit level, each candidate's own noise and bias"""
    rng = np.random.default_rng(seed)
    return (-1.0 + 0.5 * rng.standard_normal((n, 1))) + rng.standard_normal((n, Q)) * rng.uniform(0.2, 1.0, size=Q) - rng.uniform(0.0, 0.3, size=Q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[409600, 4096])
    ap.add_argument("--Q", type=int, default=8)
    ap.add_argument("--iters", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from bayesfmmm_amd import api
    import stacking_ref as R
    lib = api._lib_entry()
    api.stacking(columns(1024, args.Q, 0), max_iter=32)      # warm-up: the kernels are loaded
    shapes = []
    for n in args.n:
        L = columns(n, args.Q, n)
        wall_fixed, dev_fixed, wall_e2e = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            api.stacking(L, max_iter=args.iters, check_every=args.iters, tol=0.0)
            wall_fixed.append((time.perf_counter() - t0) * 1e3)
            dev_fixed.append(lib.bfmmm_post_last_kernel_ms())
            t0 = time.perf_counter()
            res = api.stacking(L)
            wall_e2e.append((time.perf_counter() - t0) * 1e3)
        launches = args.iters + 2      # launch j forms w_j; the launch after the last iterate reports its gap
        t0 = time.perf_counter()
        ref = R.em(L, dtype=np.float64, row_sum=R.sum_forward)
        host_ms = (time.perf_counter() - t0) * 1e3
        p_bytes = 8 * n * args.Q
        shapes.append({"n": n, "Q": args.Q, "iters_timed": args.iters,
                       "device_us_per_iteration": med(dev_fixed) * 1e3 / launches,
                       "device_ms_fixed_count": med(dev_fixed), "wall_ms_fixed_count": med(wall_fixed),
                       "end_to_end_ms": med(wall_e2e), "n_iter": int(res["n_iter"]), "converged": bool(res["converged"]), "gap": float(res["gap"]),
                       "P_bytes": p_bytes, "read_P_once_us_at_hbm_rate": p_bytes / HBM_BYTES_PER_S * 1e6,
                       "host_numpy_ms": host_ms, "host_numpy_n_iter": int(ref["n_iter"]),
                       "host_numpy_us_per_iteration": host_ms * 1e3 / max(1, int(ref["n_iter"])),
                       "largest_weight_difference_to_host": float(np.max(np.abs(res["weights"] - ref["weights"])))})
    print(json.dumps({"what": "stacking", "reps": args.reps, "shapes": shapes}), flush=True)


if __name__ == "__main__":
    main()
