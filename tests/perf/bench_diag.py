#!/usr/bin/env python3
"""Times the convergence diagnostics (k_diag through bfmmm_post_diagnostics; bfmmm_post_last_kernel_ms: device time of the
kernels alone) on one MI355X for two shapes, next to one read of the draws at 6.3 TB/s.  Not the bench line.  One JSON
line per case.

  Z-shaped rows: 12288 rows x 8 chains x 1000 draws (the LDS tier)
  long rows:     16 rows x 32 chains x 20000 draws (the global tier)

  python tests/perf/bench_diag.py [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _draws(S, C, P, rng):
    """(S, C, P): AR(1) rows with rho spread over [0, 0.95] (the truncation lag grows with rho)"""
    rho = np.linspace(0.0, 0.95, P)
    e = rng.standard_normal((S, C, P))
    x = np.empty_like(e)
    x[0] = e[0]
    for t in range(1, S):
        x[t] = rho * x[t - 1] + e[t]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from bayesfmmm_amd import api
    lib = api._lib_entry()
    rng = np.random.default_rng(1)
    for what, P, C, S in (("Z-shaped rows", 12288, 8, 1000), ("long rows", 16, 32, 20000)):
        x = _draws(S, C, P, rng)
        ms = []
        for _ in range(args.reps + 1):
            api.diagnostics(x)
            ms.append(lib.bfmmm_post_last_kernel_ms())
        ms = sorted(ms[1:])
        print(json.dumps({"what": what, "rows": P, "chains": C, "draws": S, "kernel_ms_min": ms[0], "kernel_ms_median": ms[len(ms) // 2],
                          "one_read_at_6.3TBps_ms": x.nbytes / 6.3e12 * 1e3}), flush=True)


if __name__ == "__main__":
    main()
