#!/usr/bin/env python3
"""Times the Laplace mixture proposal (kernels_predict_laplace.hip) on one MI355X at the per-pair shape of 7m and 7o:
curves of 100 points, K = 3, P = 30, M = 6, J = 256 samples, the chains started from the generating state -- next to Sampler.predict
and Sampler.loo_marginal at their defaults in the same session.  The mode search runs one thread a start, so the full shape of 7o
(4096 curves x 4000 draws) is not the default here: --n, --chains and --slots choose the number of (curve, draw) pairs and the times
are also given per million pairs.  For predict (the first --new training curves as new curves) and loo_marginal, both proposals: the
device time (HIP events, Sampler.timing) and the end-to-end time, medians of --reps calls after a warm-up; for the mixture the
share of the device time that is not the sampling pass, estimated as 1 - (device time of the staged call with one stage, which is
one such pass) / (device time of the mixture call); n_modes; the median of ess_mean, the least ess_min and n_below; pareto_k and
elpd_loo of the marginal rows; and the iterations per start of the reference's search (tests/predict_laplace_ref.py) on the draws of
--probe pairs, which the device does not return.  Not the bench line.  One JSON line.

  python tests/perf/bench_predict_laplace.py [--n 256] [--chains 8] [--slots 64] [--new 64] [--J 256] [--reps 5] [--probe 24]
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


def timed(reps, call, timers):
    wall, dev = [], {k: [] for k in timers}
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, fn in timers.items():
            dev[k].append(fn())
    return res, med(wall), {k: med(v) for k, v in dev.items()}


def loo_row(res, pairs):
    k = np.asarray(res["pareto_k"])
    return {"share_below_floor": float(np.sum(res["n_below"], dtype=np.int64)) / pairs, "curves_with_pairs_below": int(np.sum(res["n_below"] > 0)),
            "median_ess_mean": float(np.median(res["ess_mean"])), "min_ess_min": float(np.min(res["ess_min"])),
            "median_pareto_k": float(np.median(k)), "max_pareto_k": float(np.max(k)), "n_khat_above": int(res["n_khat_above"]),
            "elpd_loo": float(res["elpd_loo"]), "p_loo": float(res["p_loo"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--J", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe", type=int, default=24)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    import predict_laplace_ref as Lr
    import predict_ref as R
    w2 = bench.make_config2(n=args.n)
    n, C, S, K, M, P, J = args.n, args.chains, args.slots, w2["K"], w2["M"], w2["P"], args.J
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w2["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w2["y"], w2["t"], w2["internal_knots"], w2["boundary_knots"], n_chains=C)
    for q in range(C):
        smp.select_chain(q)
        smp.set_state(**w2["state"])
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    m = min(args.new, n)
    yn, tn = w2["y"][:m], w2["t"][:m]
    out = {"what": "predict_laplace", "reps": args.reps, "n": n, "n_new": m, "K": K, "M": M, "P": P, "chains": C, "slots": S, "draws": C * S,
           "points": int(len(w2["y"][0])), "J": J, "predict_pairs": m * C * S, "loo_pairs": n * C * S}
    smp.predict(yn[:2], tn[:2], n_samples=J, n_slots=min(S, 4))      # warm-up: the kernels are loaded
    smp.predict(yn[:2], tn[:2], n_samples=J, n_slots=min(S, 4), proposal="laplace")
    dev = lambda name: (lambda: smp.timing(name)[0])
    for label, kw, tm in (("dirichlet_R3", {}, "predict"), ("dirichlet_R1", {"n_stages": 1}, "predict"), ("laplace", {"proposal": "laplace"}, "predict_laplace")):
        res, wall, d = timed(args.reps, lambda: smp.predict(yn, tn, n_samples=J, seed=1, **kw), {"device_ms": dev(tm)})
        row = {"end_to_end_ms": wall, "device_ms": d["device_ms"], "device_ms_per_million_pairs": d["device_ms"] / (m * C * S) * 1e6,
               "median_ess_mean": float(np.median(res["ess_mean"])), "min_ess_min": float(np.min(res["ess_min"])), "elpd": res["elpd"]}
        if "n_modes_mean" in res:
            row["n_modes_mean"] = float(np.mean(res["n_modes_mean"]))
        out["predict_" + label] = row
        print(json.dumps({"predict_" + label: row}), file=sys.stderr, flush=True)
    out["predict_laplace"]["search_share_estimate"] = 1.0 - out["predict_dirichlet_R1"]["device_ms"] / out["predict_laplace"]["device_ms"]
    pairs = n * C * S
    for label, kw, tm in (("dirichlet_default", {}, "loo_marginal"), ("laplace", {"proposal": "laplace"}, "loo_marginal_laplace")):
        res, wall, d = timed(args.reps, lambda: smp.loo_marginal(n_samples=J, seed=1, **kw), {"device_ms": dev(tm), "psis_device_ms": dev("loo_marginal_psis")})
        row = dict(loo_row(res, pairs), end_to_end_ms=wall, device_ms_per_million_pairs=d["device_ms"] / pairs * 1e6, **d)
        if "n_modes_mean" in res:
            row["n_modes_mean"] = float(np.mean(res["n_modes_mean"]))
        out["loo_marginal_" + label] = row
        print(json.dumps({"loo_marginal_" + label: row}), file=sys.stderr, flush=True)
    # iterations per start, from the reference's search on the draws of a few pairs
    B = smp.get_basis()
    rng = np.random.default_rng(0)
    iters, conv = [], []
    for _ in range(args.probe):
        i, q, s = int(rng.integers(n)), int(rng.integers(C)), int(rng.integers(S))
        smp.select_chain(q)
        th = R.directions(smp.get_chain("nu")[..., s], smp.get_chain("Phi")[..., s])
        case = Lr.make_case(B[i], np.asarray(w2["y"][i], dtype=np.float64), th, float(smp.get_chain("sigma_sq")[s]),
                            smp.get_chain("alpha_3")[s] * smp.get_chain("pi")[:, s])
        for e in Lr.starts(case["alpha"]):
            r = Lr.search(case, e)
            iters.append(r["iters"])
            conv.append(bool(r["conv"]))
    smp.select_chain(0)
    if iters:
        out["reference_search"] = {"pairs": args.probe, "starts": len(iters), "converged": int(np.sum(conv)), "median_iterations": float(np.median(iters)),
                                   "mean_iterations": float(np.mean(iters)), "max_iterations": int(np.max(iters))}
    smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
