#!/usr/bin/env python3
"""Times the reference's rescale step per draw and the summaries under it (kernels_rescale.hip, k_ccov_mix) on one
MI355X at the shape of 7j (n = 4096 curves, K = 3, P = 30, M = 6) with 8 chains x 500 slots = 4000 draws, the chains started
from the generating state with their labels permuted:
  - Sampler.rescale and, with rescale=, aligned_summary("Z"), cluster_mean_bands and cluster_cov_bands (all pairs, G x G) end to
    end and the device time of their own kernels (HIP events on the sampler's stream, Sampler.timing): medians of --reps calls
    after a warm-up call,
  - the route without them: get_chain of Z, nu and Phi of every chain to the host, then the transform, Z A^-1, A nu and the
    covariance values with their quantiles in numpy, timed once,
next to the transform kernel one read of the Z slots: k_align_gram's device time, a kernel that reads them once, and the floor
at bench.py's HBM peak.  Checks the device's pure curves against numpy's.  Not the bench line.  One JSON line.

  python tests/perf/bench_rescale.py [--n 4096] [--chains 8] [--slots 500] [--reps 5] [--G 48]
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
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:args.G])
    G = int(E.shape[0])

    res = {}
    a, res["align"] = timed(lambda: smp.align(pivot=(0, S - 1)), {"gram_device_ms": lambda: smp.timing("align_gram")[0]}, args.reps)
    perm = a["perm"]
    r, res["rescale"] = timed(lambda: smp.rescale(perm=perm), {"transform_device_ms": lambda: smp.timing("rescale_transform")[0]}, args.reps)
    _, res["rescaled_summary_Z"] = timed(lambda: smp.aligned_summary("Z", rescale=r), {"gather_device_ms": lambda: smp.timing("rescale_gather")[0]},
                                         args.reps)
    res["rescaled_summary_Z"]["gather_launches"] = smp.timing("rescale_gather")[1]
    _, res["aligned_summary_Z"] = timed(lambda: smp.aligned_summary("Z", perm), {"gather_device_ms": lambda: smp.timing("align_gather")[0]},
                                        args.reps)
    _, res["cluster_mean_bands_rescaled"] = timed(lambda: smp.cluster_mean_bands(E, rescale=r),
                                                  {"project_device_ms": lambda: smp.timing("rescale_project")[0]}, args.reps)
    _, res["cluster_mean_bands"] = timed(lambda: smp.cluster_mean_bands(E, perm), {"project_device_ms": lambda: smp.timing("align_project")[0]},
                                         args.reps)
    ctim = {nm + "_device_ms": (lambda nm=nm: smp.timing(nm)[0]) for nm in ("cluster_cov_project", "cluster_cov")}
    _, res["cluster_cov_bands_rescaled"] = timed(lambda: smp.cluster_cov_bands(E, rescale=r), ctim, args.reps)
    _, res["cluster_cov_bands"] = timed(lambda: smp.cluster_cov_bands(E, perm), ctim, args.reps)

    # the host route: the chains to the host, then numpy
    t0 = time.perf_counter()
    zs, nus, phis = [], [], []
    for q in range(C):
        smp.select_chain(q)
        zs.append(smp.get_chain("Z"))
        nus.append(smp.get_chain("nu"))
        phis.append(smp.get_chain("Phi"))
    smp.select_chain(0)
    t1 = time.perf_counter()
    Z = np.stack(zs)                                                                   # (C, n, K, S)
    cols = np.take_along_axis(Z, perm.transpose(0, 2, 1)[:, None, :, :], axis=2)       # column k: raw component perm[k]
    curve = np.argmax(cols, axis=1)                                                    # (C, K, S): the first maximum
    A = np.take_along_axis(Z, curve[:, :, None, :], axis=1).transpose(0, 3, 1, 2)      # (C, S, K, K): A[k][c] = Z[curve[k], c]
    Ainv = np.linalg.inv(A)
    t2 = time.perf_counter()
    zt = np.einsum("qics,qsck->iksq", Z, Ainv)
    np.quantile(zt.reshape(n, K, -1), (0.025, 0.5, 0.975), axis=-1)
    t3 = time.perf_counter()
    nut = np.einsum("qskc,qcps->qskp", A, np.stack(nus))
    v = np.einsum("gp,qskp->kgqs", E, nut)
    np.quantile(v.reshape(K, G, -1), (0.025, 0.5, 0.975), axis=-1)
    t4 = time.perf_counter()
    W = np.einsum("qskc,gp,qcpms->qskgm", A, E, np.stack(phis), optimize=True)
    pairs = [(k, l) for k in range(K) for l in range(k, K)]
    cv = np.stack([np.einsum("qsgm,qshm->ghqs", W[:, :, k], W[:, :, l]) for k, l in pairs])
    np.quantile(cv.reshape(len(pairs), G, G, -1), (0.025, 0.5, 0.975), axis=-1)
    t5 = time.perf_counter()
    res["host_route"] = {"get_chain_Z_nu_Phi_ms": (t1 - t0) * 1e3, "numpy_transform_ms": (t2 - t1) * 1e3, "numpy_Z_summary_ms": (t3 - t2) * 1e3,
                         "numpy_mean_bands_ms": (t4 - t3) * 1e3, "numpy_cov_bands_ms": (t5 - t4) * 1e3}

    z_bytes = 8.0 * n * K * C * S
    floor_ms = z_bytes / (bench.HBM_PEAK_GBS * 1e9) * 1e3
    tr = res["rescale"]["transform_device_ms"]
    print(json.dumps({"what": "rescale", "n": n, "K": K, "M": M, "P": int(E.shape[1]), "chains": C, "slots": S, "draws": C * S, "G": G, **res,
                      "z_slot_bytes": z_bytes, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "floor_one_read_of_Z_ms": floor_ms,
                      "one_read_of_Z_by_align_gram_ms": res["align"]["gram_device_ms"], "transform_reads_of_Z": 2,
                      "transform_over_two_reads_floor": tr / (2 * floor_ms), "transform_achieved_GBs": 2 * z_bytes / (tr * 1e-3) / 1e9,
                      "curve_equals_numpy": float(np.mean(curve.transpose(0, 2, 1) == r["curve"])),
                      "n_singular": r["n_singular"], "rcond_min": float(np.min(r["rcond"])), "z_min_min": float(np.nanmin(r["z_min"]))}),
          flush=True)
    smp.close()


if __name__ == "__main__":
    main()
