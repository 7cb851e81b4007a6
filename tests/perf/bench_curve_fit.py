#!/usr/bin/env python3
"""Times the pooled per-curve credible bands of chain slots (kernels_curve_fit.hip) on one MI355X at the
config-2 shape (n = 4096 curves, K = 3, P = 30, M = 6) with 8 chains x 500 slots and G = 50 points of a common time grid:
204 800 rows of 4000 draws.
  - device time of each kernel (HIP events on the sampler's stream, Sampler.timing) and Sampler.curve_bands end to end:
    medians of --reps calls after a warm-up call,
  - the same rows through the workspace route (k_fit_values + the band kernels of the long rows; bfmmm_set_curve_fit_route),
  - the route without it on the same draws: get_chain of every chain plus the numpy restatement (tests/curve_fit_ref.py) on
    --host-curves curves, scaled to n,
next to two floors: one read of Z and chi of the slots at 6.3 TB/s, and the multiply-adds of the values at the vector fp64
rate (78.6 Tflop/s).  Not the bench line.  One JSON line.

  python tests/perf/bench_curve_fit.py [--n 4096] [--chains 8] [--slots 500] [--grid 50] [--reps 5]
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

KERNELS = ("curve_fit_project", "curve_fit_rows", "curve_fit_values", "curve_fit_reduce", "curve_fit")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(smp, E, reps, **kw):
    wall, dev, out = [], {k: [] for k in KERNELS}, None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = smp.curve_bands(E, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in KERNELS:
            dev[k].append(smp.timing(k)[0])
    return out, med(wall[1:]), {k: med(v[1:]) for k, v in dev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-curves", type=int, default=64)
    ap.add_argument("--workspace-mib", type=int, default=2048, help="max_workspace_bytes of the workspace route")
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import api
    import bench
    import curve_fit_ref as R
    w = bench.make_config2(n=args.n)
    C, S, n, K, M, P, G = args.chains, args.slots, w["n"], w["K"], w["M"], w["P"], args.grid
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    for q in range(C):
        st = dict(w["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        smp.select_chain(q)
        smp.set_state(**st)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    bk = w["boundary_knots"]
    grid = np.linspace(bk[0], bk[1], G).reshape(-1, 1)
    E = np.ascontiguousarray(api.TensorBSpline(grid, [w["degree"]], [list(bk)], [w["internal_knots"]]))

    fused, wall, dev = timed(smp, E, args.reps)
    lib = smp.lib
    lib.bfmmm_set_curve_fit_route(1)
    ws, ws_wall, ws_dev = timed(smp, E, args.reps, max_workspace_bytes=args.workspace_mib << 20)
    lib.bfmmm_set_curve_fit_route(0)
    same = {k: bool(fused[k].tobytes() == ws[k].tobytes()) for k in ("mean", "sd", "quantiles")}
    qdiff = float(np.max(np.abs(fused["quantiles"] - ws["quantiles"]) / np.maximum(1.0, np.abs(fused["quantiles"]))))

    # the route without the kernels: every chain's draws to the host, then numpy, on a few curves
    hc = min(args.host_curves, n)
    t0 = time.perf_counter()
    chains = []
    for q in range(C):
        smp.select_chain(q)
        chains.append({nm: smp.get_chain(nm) for nm in ("nu", "Phi", "Z", "chi")})
    copies_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    v = R.values(chains, E, "fit", 0, S, curves=np.arange(hc)).reshape(hc, G, C * S)
    hq = R.quantiles(v, fused["probs"])
    hm, hs = R.moments(v)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    agree = float(np.max(np.abs(hq - fused["quantiles"][:hc]) / np.maximum(1.0, np.abs(hq))))

    NJ = K * (M + 1)
    z_chi = 8.0 * n * C * S * (K + M)
    flops = 2.0 * n * G * C * S * NJ + 2.0 * G * NJ * P * C * S
    print(json.dumps({"what": "curve_bands fit", "n": n, "chains": C, "slots": S, "G": G, "K": K, "P": P, "M": M, "rows": n * G,
                      "draws_per_row": C * S,
                      "fused_end_to_end_ms": wall, "fused_device_ms": dev,
                      "workspace_route_end_to_end_ms": ws_wall, "workspace_route_device_ms": ws_dev,
                      "workspace_route_equals_fused_bitwise": same, "workspace_route_quantiles_worst_rel_diff": qdiff,
                      "ns_per_row_fused": dev["curve_fit_rows"] * 1e6 / (n * G),
                      "floor_Z_chi_once_at_6.3TBps_ms": z_chi / 6.3e12 * 1e3,
                      "floor_multiply_adds_at_78.6Tflops_ms": flops / 78.6e12 * 1e3,
                      "host_route_get_chain_ms": copies_ms, "host_route_numpy_ms_on_host_curves": numpy_ms, "host_curves": hc,
                      "host_route_scaled_to_n_ms": copies_ms + numpy_ms * n / hc,
                      "worst_rel_diff_to_host_route_quantiles": agree}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
