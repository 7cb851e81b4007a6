#!/usr/bin/env python3
"""Times the contrasts of cluster mean functions and covariate effects (kernels_cluster_contrast.hip) on one MI355X at
the shape of 7r (n = 4096 curves, K = 3, P = 30, M = 6) with 8 chains x 500 slots = 4000 draws and G = 48 grid points, the chains
started from the generating state with their labels permuted:
  - Sampler.cluster_contrast_bands under a rescale dict, "pairwise" (R = 3) on a sampler without covariates and "effects" (R = 6) on
    one with D = 2, each with and without simultaneous=: end to end and the device time of its three timers (HIP events on the
    sampler's stream, Sampler.timing): medians of --reps calls after a warm-up call,
  - the nearest existing call from the same session, cluster_mean_bands(E, rescale=r) (K G rows: as many as "pairwise" at K = 3),
    with the device time of k_rescale_project, and both kernels' device time per result row,
  - the route without the call: get_chain of nu (and eta) of every chain to the host, then the values, their moments and
    quantiles, prob_positive, the band and the norm in numpy, timed once.
Checks the device's means against numpy's.  Not the bench line.  One JSON line.

  python tests/perf/bench_cluster_contrast.py [--n 4096] [--chains 8] [--slots 500] [--reps 5] [--G 48]
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

TIMERS = ("contrast_coef", "contrast_values", "contrast_norm")


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


def host_route(smp, E, A, w_nu, w_eta, alpha):
    """get_chain plus numpy: the same results on the host; returns (its times, the means)"""
    C = smp.n_chains
    t0 = time.perf_counter()
    nus, etas = [], []
    for q in range(C):
        smp.select_chain(q)
        nus.append(smp.get_chain("nu"))
        if w_eta is not None:
            etas.append(smp.get_chain("eta"))
    smp.select_chain(0)
    t1 = time.perf_counter()
    a = np.einsum("rk,qskc->qsrc", w_nu, A)
    b = np.einsum("qsrc,qcps->qsrp", a, np.stack(nus))
    if w_eta is not None:
        b = b + np.einsum("rkd,qskc,qpdcs->qsrp", w_eta, A, np.stack(etas), optimize=True)
    R, G = w_nu.shape[0], E.shape[0]
    v = np.einsum("gp,qsrp->rgqs", E, b).reshape(R, G, -1)
    mean, sd = v.mean(axis=-1), v.std(axis=-1, ddof=1)
    np.quantile(v, (0.025, 0.5, 0.975), axis=-1)
    (v > 0).mean(axis=-1)
    dev = np.max(np.abs(v - mean[..., None]) / sd[..., None], axis=1)
    crit = np.quantile(dev, 1.0 - alpha, axis=-1)
    (dev >= np.max(np.abs(mean) / sd, axis=-1)[:, None]).mean(axis=-1)
    norm = np.sqrt((v * v).mean(axis=1))
    np.quantile(norm, (0.025, 0.5, 0.975), axis=-1)
    t2 = time.perf_counter()
    return {"get_chain_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "crit": [float(c) for c in crit]}, mean


def one(args, D, contrasts):
    import bayesfmmm_amd as bf
    import bench
    w = bench.make_config2(n=args.n)
    C, S, K, M = args.chains, args.slots, w["K"], w["M"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w["y"], w["t"], w["internal_knots"], w["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    if D:
        smp.set_covariates(rng.standard_normal((w["n"], D)), covariance_adj=False)
    all_perms = list(itertools.permutations(range(K)))
    for q in range(C):
        p = list(all_perms[q % len(all_perms)])
        st = dict(w["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
            st[nm] = np.asarray(st[nm])[p]
        st["Z"] = np.asarray(st["Z"])[:, p]
        if D:
            st["eta"] = 0.1 * rng.standard_normal(smp._draw_shape("eta"))      # stays as set: the sweep below does not update it
        smp.select_chain(q)
        smp.set_state(**st)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:args.G])
    G = int(E.shape[0])
    perm = smp.align(pivot=(0, S - 1))["perm"]
    r = smp.rescale(perm=perm)
    tim = {nm + "_device_ms": (lambda nm=nm: smp.timing(nm)[0]) for nm in TIMERS}
    res = {"D": D, "contrasts": contrasts, "n_singular": r["n_singular"]}
    got, res["pointwise"] = timed(lambda: smp.cluster_contrast_bands(E, contrasts, rescale=r), tim, args.reps)
    res["pointwise"]["values_launches"] = smp.timing("contrast_values")[1]
    _, res["simultaneous"] = timed(lambda: smp.cluster_contrast_bands(E, contrasts, rescale=r, simultaneous=0.05), tim, args.reps)
    res["simultaneous"]["values_launches"] = smp.timing("contrast_values")[1]
    x = None if not D else np.zeros(D)
    _, res["cluster_mean_bands_rescaled"] = timed(lambda: smp.cluster_mean_bands(E, rescale=r, x=x),
                                                  {"project_device_ms": lambda: smp.timing("rescale_project")[0]}, args.reps)
    R = got["mean"].shape[0]
    res["R"] = R
    res["values_us_per_row"] = 1e3 * res["pointwise"]["contrast_values_device_ms"] / (R * G)
    res["coef_plus_values_us_per_row"] = 1e3 * (res["pointwise"]["contrast_values_device_ms"] + res["pointwise"]["contrast_coef_device_ms"]) / (R * G)
    res["rescale_project_us_per_row"] = 1e3 * res["cluster_mean_bands_rescaled"]["project_device_ms"] / (K * G)
    res["host_route"], mean = host_route(smp, E, r["transform"], got["w_nu"], got["w_eta"], 0.05)
    res["mean_max_abs_diff_vs_numpy"] = float(np.max(np.abs(got["mean"] - mean)))
    res["P"] = int(E.shape[1])
    res["G"] = G
    smp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--G", type=int, default=48)
    args = ap.parse_args()
    out = {"what": "cluster_contrast", "n": args.n, "chains": args.chains, "slots": args.slots, "draws": args.chains * args.slots,
           "pairwise": one(args, 0, "pairwise"), "effects": one(args, 2, "effects")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
