#!/usr/bin/env python3
"""Times the least-squares loss of every draw against the pooled co-membership matrix (k_similarity_loss) on one
MI355X at the config-2 shape (n = 4096 curves, K = 3) with 8 chains x 500 slots: 2080 blocks of the upper triangle over 4000 draws.
  - device time of the block kernel and of the reduce kernel (HIP events on the sampler's stream, Sampler.timing) and
    Sampler.similarity_loss end to end, with and without the diagnostics: medians of --reps calls after a warm-up call,
  - in the same process on the same build, Sampler.similarity(sd=True) on the full matrix, which makes the same two passes over
    all n^2 / 256 tiles where the loss visits only those of the blocks with rb <= cb,
  - Sampler.representative_draw(("Z", "nu", "Phi")) end to end,
next to the floor of the loss: the MFMAs of its two passes over the upper triangle at bench.py's fp64 matrix peak.  Checks that
sum(loss) and (N - 1) sum(sd^2) agree.  Not the bench line.  One JSON line.

  python tests/perf/bench_similarity_loss.py [--n 4096] [--chains 8] [--slots 500] [--reps 5]
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


def timed(call, timers, reps):
    wall, dev, out = [], {nm: [] for nm in timers}, None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for nm, read in timers.items():
            dev[nm].append(read())
    return out, {**{nm: med(v[1:]) for nm, v in dev.items()}, "end_to_end_ms": med(wall[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
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
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)

    loss_timers = {"device_ms": lambda: smp.timing("similarity_loss")[0], "reduce_device_ms": lambda: smp.timing("similarity_loss_reduce")[0]}
    res = {}
    full, res["similarity_mean_sd"] = timed(lambda: smp.similarity(), {"device_ms": lambda: smp.timing("similarity")[0]}, args.reps)
    loss, res["loss"] = timed(lambda: smp.similarity_loss(diagnostics=False), loss_timers, args.reps)
    _, res["loss_with_diagnostics"] = timed(lambda: smp.similarity_loss(), loss_timers, args.reps)
    rep, res["representative_draw_Z_nu_Phi"] = timed(lambda: smp.representative_draw(("Z", "nu", "Phi")), loss_timers, args.reps)
    res["loss"]["launches"] = smp.timing("similarity_loss")[1]

    N = C * S
    a, b = float(loss["loss"].sum()), float((N - 1) * (full["sd"] ** 2).sum())
    nbk = (n + 63) // 64
    blocks = nbk * (nbk + 1) // 2
    mfmas = 2.0 * blocks * 16.0 * N * ((K + 3) // 4)       # two passes, 16 tiles a block
    mfma_ms = mfmas * 2048.0 / (bench.FP64_MFMA_PEAK_TF * 1e12) * 1e3
    print(json.dumps({"what": "similarity_loss", "n": n, "K": K, "chains": C, "slots": S, "draws": N, "blocks": blocks, **res,
                      "floor_mfma_two_passes_upper_triangle_ms": mfma_ms, "fp64_matrix_peak_Tflops": bench.FP64_MFMA_PEAK_TF,
                      "loss_over_mfma_floor": res["loss"]["device_ms"] / mfma_ms,
                      "loss_over_similarity_mean_sd": res["loss"]["device_ms"] / res["similarity_mean_sd"]["device_ms"],
                      "best": [loss["chain"], loss["slot"]], "min_loss": loss["min"], "max_loss": float(loss["loss"].max()),
                      "representative_draw_is_best": bool((rep["chain"], rep["slot"]) == (loss["chain"], loss["slot"])),
                      "sum_loss_vs_pooled_variance_rel": abs(a - b) / b,
                      "sum_loss_vs_pooled_variance_tol": 4.0 * (n * n + N + 2) * 2.0 ** -52}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
