#!/usr/bin/env python3
"""Times the simultaneous credible bands of the pooled per-curve fits (k_fit_sim in kernels_curve_fit.hip) on
one MI355X at the config-2 shape (n = 4096 curves, K = 3, P = 30, M = 6) with 8 chains x 500 slots and G = 50 points of a
common time grid, for both `which`:
  - device time of k_fit_sim (HIP events on the sampler's stream, Sampler.timing("curve_sim")) and
    Sampler.curve_bands_simultaneous end to end: medians of --reps calls after a warm-up call,
  - Sampler.curve_bands (pointwise) on the same input next to it,
  - the same call at --small-grid (8) grid points: Z and chi of a draw are re-read once per tile of 8 grid points and pass, so
    the difference between the two grids, per grid point, is what a tile costs with its re-read,
  - the route without the kernel: curve_fit of --host-curves curves to the host plus the numpy restatement
    (tests/curve_sim_ref.py), scaled to n,
next to two floors: three formations of the values (3 x 2 n G N NJ flop at the vector fp64 rate, 78.6 Tflop/s) and one read of
Z and chi of the slots at 6.3 TB/s.  Not the bench line.  One JSON line per `which`.

  python tests/perf/bench_curve_sim.py [--n 4096] [--chains 8] [--slots 500] [--grid 50] [--reps 5]
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


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(call, timing, names, reps):
    wall, dev, out = [], {k: [] for k in names}, None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in names:
            dev[k].append(timing(k)[0])
    return out, med(wall[1:]), {k: med(v[1:]) for k, v in dev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--small-grid", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-curves", type=int, default=16)
    ap.add_argument("--alpha", type=float, default=0.05)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import api
    import bench
    import curve_sim_ref as SR
    w = bench.make_config2(n=args.n)
    C, S, n, K, M, G = args.chains, args.slots, w["n"], w["K"], w["M"], args.grid
    N = C * S
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

    def basis(g):
        grid = np.linspace(bk[0], bk[1], g).reshape(-1, 1)
        return np.ascontiguousarray(api.TensorBSpline(grid, [w["degree"]], [list(bk)], [w["internal_knots"]]))

    E, Es = basis(G), basis(args.small_grid)
    sim_names = ("curve_sim", "curve_sim_reduce", "curve_fit_project")
    pw_names = ("curve_fit", "curve_fit_rows", "curve_fit_project")
    for which in ("mean", "fit"):
        sim, wall, dev = timed(lambda: smp.curve_bands_simultaneous(E, which=which, alpha=args.alpha), smp.timing, sim_names, args.reps)
        _, wall_s, dev_s = timed(lambda: smp.curve_bands_simultaneous(Es, which=which, alpha=args.alpha), smp.timing, sim_names, args.reps)
        pw, pw_wall, pw_dev = timed(lambda: smp.curve_bands(E, which=which), smp.timing, pw_names, args.reps)
        same = bool(sim["mean"].tobytes() == pw["mean"].tobytes() and sim["sd"].tobytes() == pw["sd"].tobytes())
        # the route without the kernel, on a few curves
        hc = min(args.host_curves, n)
        t0 = time.perf_counter()
        vals = smp.curve_fit(E, which=which, curves=np.arange(hc)).reshape(hc, G, N)
        copy_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = SR.sim_bands(vals, args.alpha)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        agree = float(np.max(np.abs(host["crit"] - sim["crit"][:hc]) / host["crit"]))
        NJ = K * (M + 1 if which == "fit" else 1)
        per_point = (dev["curve_sim"] - dev_s["curve_sim"]) / (G - args.small_grid)
        print(json.dumps({"what": "curve_bands_simultaneous " + which, "n": n, "chains": C, "slots": S, "G": G, "K": K, "P": w["P"],
                          "M": M, "draws_per_row": N, "alpha": args.alpha,
                          "sim_end_to_end_ms": wall, "sim_device_ms": dev,
                          "sim_small_grid": args.small_grid, "sim_small_grid_end_to_end_ms": wall_s, "sim_small_grid_device_ms": dev_s,
                          "curve_sim_ms_per_grid_point_between_the_grids": per_point,
                          "curve_sim_ms_at_zero_grid_points_extrapolated": dev_s["curve_sim"] - per_point * args.small_grid,
                          "pointwise_curve_bands_end_to_end_ms": pw_wall, "pointwise_curve_bands_device_ms": pw_dev,
                          "mean_and_sd_equal_curve_bands_bitwise": same,
                          "floor_three_formations_at_78.6Tflops_ms": 3 * 2.0 * n * G * N * NJ / 78.6e12 * 1e3,
                          "floor_Z_chi_once_at_6.3TBps_ms": 8.0 * n * N * (K + (M if which == "fit" else 0)) / 6.3e12 * 1e3,
                          "host_route_curve_fit_ms": copy_ms, "host_route_numpy_ms": numpy_ms, "host_curves": hc,
                          "host_route_scaled_to_n_ms": (copy_ms + numpy_ms) * n / hc,
                          "worst_rel_diff_of_crit_to_host_route": agree}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
