#!/usr/bin/env python3
"""Times the cluster covariance surfaces with bands (kernels_cluster_cov.hip) on one MI355X at the shape of 7j
(n = 4096 curves, K = 3, config 2's M) with 8 chains x 500 slots = 4000 draws on a grid of G = 48 points, the chains started from
the generating state with their labels permuted:
  - Sampler.cluster_cov_bands of all six pairs on the full G x G surface and of the variance functions (diagonal), each with and
    without the simultaneous band, under the default workspace budget (256 MiB: the full surface takes two chunks, and with the
    band a second sweep) and under one that holds the call in a single chunk: medians of --reps calls after a warm-up call of the
    end-to-end time and of the device times of k_ccov_project, k_ccov_values and k_ccov_maxdev (HIP events on the sampler's
    stream, Sampler.timing); the same call without quantiles tells how much of the time is the unchanged quantile sort,
  - the route without it: get_chain("Phi") of every chain to the host, the relabelling, an einsum and np.quantile, timed once,
next to the floor of k_ccov_values: the 8 rows N bytes it writes at bench.py's HBM peak.  Checks the device's mean against
numpy's.  Not the bench line.  One JSON line.

  python tests/perf/bench_cluster_cov.py [--n 4096] [--chains 8] [--slots 500] [--reps 3] [--G 48]
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

TIMERS = ("cluster_cov_project", "cluster_cov", "cluster_cov_maxdev")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(smp, call, reps):
    wall, dev, launches = [], {nm: [] for nm in TIMERS}, {}
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for nm in TIMERS:
            ms, launches[nm] = smp.timing(nm)
            dev[nm].append(ms)
    out = {nm + "_device_ms": med(v[1:]) for nm, v in dev.items()}
    out.update({nm + "_launches": launches[nm] for nm in TIMERS})
    out["end_to_end_ms"] = med(wall[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--G", type=int, default=48)
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
    G, N = args.G, C * S
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:G])
    perm = smp.align(pivot=(0, S - 1))["perm"]
    pairs = [(k, l) for k in range(K) for l in range(k, K)]
    one_chunk = 8 * (len(pairs) * G * G + 64) * (N + 16) + (64 << 20)

    res = {}
    for name, kw in (("surface", {}), ("diagonal", dict(diagonal=True))):
        for band in (None, 0.05):
            for budget_name, budget in (("default_budget", 0), ("one_chunk", one_chunk)):
                key = f"{name}{'_simultaneous' if band else ''}_{budget_name}"
                res[key] = timed(smp, lambda: smp.cluster_cov_bands(E, perm, simultaneous=band, max_workspace_bytes=budget, **kw), args.reps)
        # the same without the quantile sort: what is left is the new kernels, the moments and the copies
        res[name + "_no_quantiles_one_chunk"] = timed(smp, lambda: smp.cluster_cov_bands(E, perm, probs=(), max_workspace_bytes=one_chunk, **kw), args.reps)
    dev = smp.cluster_cov_bands(E, perm, max_workspace_bytes=one_chunk)

    # the host route: the chains to the host, then numpy
    t0 = time.perf_counter()
    phis = []
    for q in range(C):
        smp.select_chain(q)
        phis.append(smp.get_chain("Phi"))                                         # (K, P, M, S)
    smp.select_chain(0)
    t1 = time.perf_counter()
    Wk = np.stack([np.einsum("gp,kpms->kgms", E, phis[q])[perm[q].T, :, :, np.arange(S)[None, :]] for q in range(C)])      # (C, K, S, G, M)
    host_mean = np.zeros((len(pairs), G, G))
    for r, (k, l) in enumerate(pairs):
        v = np.einsum("csgm,cshm->ghcs", Wk[:, k], Wk[:, l]).reshape(G, G, N)
        host_mean[r] = v.mean(axis=-1)
        np.quantile(v, (0.025, 0.5, 0.975), axis=-1)
    t2 = time.perf_counter()
    res["host_route"] = {"get_chain_Phi_ms": (t1 - t0) * 1e3, "numpy_surfaces_and_quantiles_ms": (t2 - t1) * 1e3}

    out = {"what": "cluster_cov", "n": n, "K": K, "M": M, "P": int(E.shape[1]), "chains": C, "slots": S, "draws": N, "G": G, "pairs": len(pairs), **res,
           "hbm_peak_GBs": bench.HBM_PEAK_GBS, "max_abs_mean_minus_numpy": float(np.max(np.abs(dev["mean"] - host_mean))),
           "max_abs_mean": float(np.max(np.abs(host_mean)))}
    for name, rows in (("surface", len(pairs) * G * G), ("diagonal", len(pairs) * G)):
        floor_ms = 8.0 * rows * N / (bench.HBM_PEAK_GBS * 1e9) * 1e3
        t = res[name + "_one_chunk"]["cluster_cov_device_ms"]
        out[name + "_floor_ms"] = floor_ms
        out[name + "_values_over_floor"] = t / floor_ms
        out[name + "_values_achieved_GBs"] = 8.0 * rows * N / (t * 1e-3) / 1e9
    print(json.dumps(out), flush=True)
    smp.close()


if __name__ == "__main__":
    main()
