#!/usr/bin/env python3
"""Times the pooled co-membership matrix of curves from chain slots (kernels_similarity.hip) on one MI355X at
the config-2 shape (n = 4096 curves, K = 3) with 8 chains x 500 slots: the full 4096 x 4096 matrix over 4000 draws.
  - device time of the mean pass alone (sd=False) and of mean + sd (HIP events on the sampler's stream, Sampler.timing) and
    Sampler.similarity end to end: medians of --reps calls after a warm-up call,
  - the same for `curves` of 16 and of 256 rows, and for the full matrix with each block shape forced,
  - the only other route: get_chain("Z") of every chain plus the numpy restatement (tests/similarity_ref.py) on --host-curves
    rows (in blocks of 8 rows, so that the draws' d fit in memory), scaled to n rows in proportion,
next to two floors: one read of Z of the slots at bench.py's HBM peak, and n^2 C S / 256 MFMAs per pass (x ceil(K / 4)) at
bench.py's fp64 matrix peak.  Not the bench line.  One JSON line.

  python tests/perf/bench_similarity.py [--n 4096] [--chains 8] [--slots 500] [--reps 5] [--host-curves 64]
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


def timed(smp, reps, **kw):
    wall, dev, out = [], [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = smp.similarity(**kw)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(smp.timing("similarity")[0])
    return out, {"device_ms": med(dev[1:]), "end_to_end_ms": med(wall[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-curves", type=int, default=64)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    import similarity_ref as R
    w = bench.make_config2(n=args.n)
    C, S, n, K, M = args.chains, args.slots, w["n"], w["K"], w["M"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    for q in range(C):
        st = dict(w["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        smp.select_chain(q)
        smp.set_state(**st)
    smp.run(bf.SWEEP_WARM, S, seed=1)

    res = {}
    _, res["full_mean_only"] = timed(smp, args.reps, sd=False)
    full, res["full_mean_sd"] = timed(smp, args.reps)
    for block, name in ((1, "full_mean_sd_blocks_64x64"), (2, "full_mean_sd_blocks_16x64")):
        smp.lib.bfmmm_set_similarity_block(block)
        other, res[name] = timed(smp, 2)
        res[name]["equals_default_bitwise"] = bool(all(other[k].tobytes() == full[k].tobytes() for k in ("mean", "sd")))
    smp.lib.bfmmm_set_similarity_block(0)
    for m in (16, 256):
        sel = rng.permutation(n)[:min(m, n)]
        got, res[f"rows_{m}_mean_sd"] = timed(smp, args.reps, curves=sel)
        res[f"rows_{m}_mean_sd"]["equals_full_rows_bitwise"] = bool(all(got[k].tobytes() == np.ascontiguousarray(full[k][sel]).tobytes()
                                                                        for k in ("mean", "sd")))

    # the route without the kernel: every chain's Z to the host, then numpy, on a few rows
    hc = min(args.host_curves, n)
    t0 = time.perf_counter()
    chains = []
    for q in range(C):
        smp.select_chain(q)
        chains.append(smp.get_chain("Z"))
    copies_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = [R.similarity(chains, 0, S, curves=np.arange(r, min(r + 8, hc))) for r in range(0, hc, 8)]
    numpy_ms = (time.perf_counter() - t0) * 1e3
    hmean, hsd = np.concatenate([h["mean"] for h in host]), np.concatenate([h["sd"] for h in host])
    N = C * S
    ratio_mean = float(np.max(np.abs(full["mean"][:hc] - hmean) / R.mean_bound(hmean, N, K)))
    ratio_sd = float(np.max(np.abs(full["sd"][:hc] - hsd) / R.sd_bound(hsd, N, K)))
    host_scaled = copies_ms + numpy_ms * n / hc

    z_bytes = 8.0 * n * K * C * S
    mfmas = float(n) * n * C * S / 256.0 * ((K + 3) // 4)
    mfma_ms = mfmas * 2048.0 / (bench.FP64_MFMA_PEAK_TF * 1e12) * 1e3
    print(json.dumps({"what": "similarity", "n": n, "K": K, "chains": C, "slots": S, "draws": N, **res,
                      "floor_Z_once_at_hbm_peak_ms": z_bytes / (bench.HBM_PEAK_GBS * 1e9) * 1e3, "hbm_peak_GBps": bench.HBM_PEAK_GBS,
                      "floor_mfma_per_pass_ms": mfma_ms, "fp64_matrix_peak_Tflops": bench.FP64_MFMA_PEAK_TF,
                      "mean_pass_over_mfma_floor": res["full_mean_only"]["device_ms"] / mfma_ms,
                      "mean_sd_over_mfma_floor_of_two_passes": res["full_mean_sd"]["device_ms"] / (2.0 * mfma_ms),
                      "host_route_get_chain_ms": copies_ms, "host_route_numpy_ms_on_host_curves": numpy_ms, "host_curves": hc,
                      "host_route_scaled_to_n_rows_ms": host_scaled,
                      "host_route_over_device_end_to_end": host_scaled / res["full_mean_sd"]["end_to_end_ms"],
                      "worst_device_minus_host_over_bound": {"mean": ratio_mean, "sd": ratio_sd}}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
