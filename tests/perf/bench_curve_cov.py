#!/usr/bin/env python3
"""Times the pooled per-curve covariance surfaces from chain slots (kernels_curve_cov.hip) on one MI355X at the
config-2 shape (n = 4096 curves, K = 3, P = 30, M = 6) with 8 chains x 500 slots on a time grid of G = 48 points:
  - the full G x G surface of every curve, mean only (one pass) and mean + sd (two passes), the diagonal (the variance function)
    of every curve, and the surface of 16 selected curves: device time of k_curve_cov and of the projection (HIP events on the
    sampler's stream, Sampler.timing) and Sampler.curve_cov end to end, medians of --reps calls after a warm-up call,
  - the only other route: get_chain("Z") and get_chain("Phi") of every chain plus the numpy restatement (tests/curve_cov_ref.py)
    on --host-curves curves, scaled to n curves in proportion,
next to two floors: the MFMAs, n N ceil(G / 16)^2 ceil(M / 4) per pass at bench.py's fp64 matrix peak, and one read of Z, of the
slots' Phi and of the projection table at bench.py's HBM peak.  Not the bench line.  One JSON line.

  python tests/perf/bench_curve_cov.py [--n 4096] [--chains 8] [--slots 500] [--grid 48] [--reps 5] [--host-curves 16]
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


def timed(smp, E, reps, **kw):
    wall, dev, proj, out = [], [], [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = smp.curve_cov(E, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(smp.timing("curve_cov")[0])
        proj.append(smp.timing("curve_cov_project")[0])
    return out, {"device_ms": med(dev[1:]), "project_ms": med(proj[1:]), "end_to_end_ms": med(wall[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--grid", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-curves", type=int, default=16)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import api
    import bench
    import curve_cov_ref as R
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

    res = {}
    _, res["full_mean_only"] = timed(smp, E, args.reps, sd=False)
    full, res["full_mean_sd"] = timed(smp, E, args.reps)
    dg, res["diagonal_mean_sd"] = timed(smp, E, args.reps, diagonal=True)
    res["diagonal_mean_sd"]["equals_surface_diagonal_bitwise"] = bool(all(
        dg[k].tobytes() == np.ascontiguousarray(np.einsum("igg->ig", full[k])).tobytes() for k in ("mean", "sd")))
    sel = rng.permutation(n)[:min(16, n)]
    got, res["rows_16_mean_sd"] = timed(smp, E, args.reps, curves=sel)
    res["rows_16_mean_sd"]["equals_full_rows_bitwise"] = bool(all(got[k].tobytes() == np.ascontiguousarray(full[k][sel]).tobytes()
                                                                  for k in ("mean", "sd")))

    # the route without the kernels: every chain's Z and Phi to the host, then numpy, on a few curves
    hc = min(args.host_curves, n)
    t0 = time.perf_counter()
    chains = []
    for q in range(C):
        smp.select_chain(q)
        chains.append({nm: smp.get_chain(nm) for nm in ("Z", "Phi")})
    copies_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = R.surfaces(chains, E, None, 0, S, curves=np.arange(hc))
    numpy_ms = (time.perf_counter() - t0) * 1e3 / 2.0      # surfaces() also forms the absolute-valued expression of the bounds
    ratio = {k: float(np.max(np.abs(full[k][:hc] - host[k]) / host["bound_" + k])) for k in ("mean", "sd")}
    host_scaled = copies_ms + numpy_ms * n / hc

    N = C * S
    tiles, MB = (G + 15) // 16, (M + 3) // 4
    mfma_ms = float(n) * N * tiles * tiles * MB * 2048.0 / (bench.FP64_MFMA_PEAK_TF * 1e12) * 1e3
    read_bytes = 8.0 * N * (n * K + K * P * M + K * G * M)
    print(json.dumps({"what": "curve_cov", "n": n, "K": K, "P": P, "M": M, "G": G, "chains": C, "slots": S, "draws": N, **res,
                      "floor_mfma_per_pass_ms": mfma_ms, "fp64_matrix_peak_Tflops": bench.FP64_MFMA_PEAK_TF,
                      "floor_one_read_at_hbm_peak_ms": read_bytes / (bench.HBM_PEAK_GBS * 1e9) * 1e3, "hbm_peak_GBps": bench.HBM_PEAK_GBS,
                      "mean_pass_over_mfma_floor": res["full_mean_only"]["device_ms"] / mfma_ms,
                      "mean_sd_over_mfma_floor_of_two_passes": res["full_mean_sd"]["device_ms"] / (2.0 * mfma_ms),
                      "host_route_get_chain_ms": copies_ms, "host_route_numpy_ms_on_host_curves": numpy_ms, "host_curves": hc,
                      "host_route_scaled_to_n_curves_ms": host_scaled,
                      "host_route_over_device_end_to_end": host_scaled / res["full_mean_sd"]["end_to_end_ms"],
                      "worst_device_minus_host_over_bound": ratio}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
