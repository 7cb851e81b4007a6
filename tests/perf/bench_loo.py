#!/usr/bin/env python3
"""Times the PSIS-LOO / WAIC pass (k_post_psis, through bfmmm_post_last_kernel_ms: device time of the kernel alone) on one
MI355X at n = 4096 curves and S kept draws, next to one read of the n x S matrix at 6.3 TB/s and the numpy restatement
(tests/psis_ref.py, one host core, on --cpu-rows rows scaled to n).  Not the bench line.  One JSON line per S.

  python tests/perf/bench_loo.py [--n 4096] [--draws 1000,4000,20000] [--reps 5] [--cpu-rows 64]
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
    ap.add_argument("--draws", default="1000,4000,20000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=64)
    args = ap.parse_args()
    from bayesfmmm_amd import api
    import psis_ref
    lib = api._lib_entry()
    rng = np.random.default_rng(1)
    for S in [int(s) for s in args.draws.split(",")]:
        # marginal log-densities of curves: a per-curve level, draw-to-draw spread, a heavy right tail of the ratios in some
        ll = -50.0 + rng.standard_normal((args.n, 1)) * 5.0 + rng.standard_normal((args.n, S)) * rng.uniform(0.2, 2.0, (args.n, 1))
        ll = np.ascontiguousarray(ll)
        ms = []
        for _ in range(args.reps + 1):
            api.psis_loo(ll)
            ms.append(lib.bfmmm_post_last_kernel_ms())
        ms = sorted(ms[1:])
        rows = min(args.cpu_rows, args.n)
        t0 = time.perf_counter()
        for i in range(rows):
            psis_ref.psis_row(ll[i])
        cpu_ms = (time.perf_counter() - t0) * 1e3 * args.n / rows
        hbm_ms = ll.nbytes / 6.3e12 * 1e3
        print(json.dumps({"what": "k_post_psis", "n": args.n, "S": S, "kernel_ms_min": ms[0], "kernel_ms_median": ms[len(ms) // 2],
                          "one_read_at_6.3TBps_ms": hbm_ms, "numpy_one_core_ms": cpu_ms, "cpu_rows_timed": rows}), flush=True)


if __name__ == "__main__":
    main()
