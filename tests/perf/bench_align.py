#!/usr/bin/env python3
"""Times the label alignment against a pivot and the pooled cluster summaries (kernels_align.hip) on one MI355X
at the config-2 shape (n = 4096 curves, K = 3) with 8 chains x 500 slots = 4000 draws, the chains started from the generating
state with their labels permuted:
  - device time of k_align_gram, k_align_gather and k_align_project (HIP events on the sampler's stream, Sampler.timing) and
    Sampler.align / aligned_summary("nu") / aligned_summary("Z") / cluster_mean_bands end to end: medians of --reps calls after a
    warm-up call,
  - the route without them: get_chain("Z") and get_chain("nu") of every chain to the host, the Gram and the enumeration in numpy,
    timed once,
next to the floor of k_align_gram: one read of the Z slots at bench.py's HBM peak.  Checks the device's permutations against
numpy's float64 ones.  Not the bench line.  One JSON line.

  python tests/perf/bench_align.py [--n 4096] [--chains 8] [--slots 500] [--reps 5] [--G 100]
"""
import argparse
import itertools
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
    ap.add_argument("--G", type=int, default=100)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    w = bench.make_config2(n=args.n)
    C, S, n, K, M = args.chains, args.slots, w["n"], w["K"], w["M"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    all_perms = list(itertools.permutations(range(K)))
    for q in range(C):
        p = list(all_perms[q % len(all_perms)])
        st = dict(w["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
            st[nm] = np.asarray(st[nm])[p]
        st["Z"] = np.asarray(st["Z"])[:, p]
        smp.select_chain(q)
        smp.set_state(**st)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:args.G])
    pivot = (0, S - 1)

    res = {}
    a, res["align"] = timed(lambda: smp.align(pivot=pivot), {"gram_device_ms": lambda: smp.timing("align_gram")[0]}, args.reps)
    gather = {"gather_device_ms": lambda: smp.timing("align_gather")[0]}
    _, res["aligned_summary_nu"] = timed(lambda: smp.aligned_summary("nu", a["perm"]), gather, args.reps)
    _, res["aligned_summary_Z"] = timed(lambda: smp.aligned_summary("Z", a["perm"]), gather, args.reps)
    res["aligned_summary_Z"]["gather_launches"] = smp.timing("align_gather")[1]
    _, res["diagnostics_Z_unaligned"] = timed(lambda: smp.diagnostics("Z"), {}, args.reps)
    _, res["cluster_mean_bands"] = timed(lambda: smp.cluster_mean_bands(E, a["perm"]), {"project_device_ms": lambda: smp.timing("align_project")[0]},
                                         args.reps)

    # the host route: the chains to the host, then numpy
    t0 = time.perf_counter()
    zs, nus = [], []
    for q in range(C):
        smp.select_chain(q)
        zs.append(smp.get_chain("Z"))
        nus.append(smp.get_chain("nu"))
    smp.select_chain(0)
    t1 = time.perf_counter()
    Zref = a["pivot"]["Z"]
    perms = np.array(all_perms)
    host = np.zeros((C, S, K), dtype=np.int32)
    for q in range(C):
        A = np.einsum("ict,il->tcl", zs[q], Zref)                                  # (S, K, K)
        sc = sum(A[:, perms[:, l], l] for l in range(K))                           # (S, K!)
        host[q] = perms[np.argmax(sc, axis=1)]
    t2 = time.perf_counter()
    v = np.stack([np.einsum("gp,tkp->kgt", E, np.stack([nus[q][host[q, t], :, t] for t in range(S)])) for q in range(C)], axis=2)
    np.quantile(v.reshape(K, E.shape[0], -1), (0.025, 0.5, 0.975), axis=-1)
    t3 = time.perf_counter()
    res["host_route"] = {"get_chain_Z_nu_ms": (t1 - t0) * 1e3, "numpy_align_ms": (t2 - t1) * 1e3, "numpy_cluster_bands_ms": (t3 - t2) * 1e3}

    z_bytes = 8.0 * n * K * C * S
    floor_ms = z_bytes / (bench.HBM_PEAK_GBS * 1e9) * 1e3
    print(json.dumps({"what": "align", "n": n, "K": K, "chains": C, "slots": S, "draws": C * S, "G": int(E.shape[0]), **res,
                      "z_slot_bytes": z_bytes, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "floor_one_read_of_Z_ms": floor_ms,
                      "gram_over_floor": res["align"]["gram_device_ms"] / floor_ms,
                      "gram_achieved_GBs": z_bytes / (res["align"]["gram_device_ms"] * 1e-3) / 1e9,
                      "perm_equals_numpy_float64": float(np.mean(np.all(host == a["perm"], axis=-1))),
                      "chain_perm": a["chain_perm"].tolist(), "modal_share": a["modal_share"].tolist()}), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
