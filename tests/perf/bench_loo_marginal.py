#!/usr/bin/env python3
"""Times the marginal PSIS-LOO over curves (kernels_loo_marginal.hip) on one MI355X at the config-2 shape of 7m: n = 4096
training curves of 100 points, K = 3, P = 30, M = 6, 8 chains x 500 slots = 4000 draws, J = 256 samples.  The chains start from the
generating state.  For R = 1 and R = 3 first-pass stages, without and with the refinement at its defaults (ess_floor = 10, 4 J
samples, 2 stages): the device time of "loo_marginal" (first pass, counting, list and refinement kernels) and of "loo_marginal_psis"
(HIP events, Sampler.timing), the end-to-end time of Sampler.loo_marginal, the share of the (curve, draw) pairs refined and still
below the floor, the median of ess_mean and the least ess_min (without the refinement: before it; with it: after it), the median and
the largest pareto_k and the count above the threshold, and elpd_loo; next to them pareto_k and elpd_loo of Sampler.loo() on the same
slots (conditional on the memberships), and the time of the composed route the call replaces at the same shape:
Sampler.predict(Y, time, trace=True) on the training data plus api.psis_loo on its lpd_trace.  Medians of --reps calls (default 1:
a call takes seconds) after one warm-up call on a few slots.  Not the bench line.  One JSON line.

  python tests/perf/bench_loo_marginal.py [--n 4096] [--chains 8] [--slots 500] [--J 256] [--reps 1] [--no-composed]
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


def khat(res):
    k = np.asarray(res["pareto_k"])
    return {"median_pareto_k": float(np.median(k)), "max_pareto_k": float(np.max(k)), "n_khat_above": int(res["n_khat_above"]),
            "khat_threshold": float(res["khat_threshold"]), "elpd_loo": float(res["elpd_loo"]), "p_loo": float(res["p_loo"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--J", type=int, default=256)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--no-composed", action="store_true")
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    from bayesfmmm_amd import api
    import bench
    w2 = bench.make_config2(n=args.n)
    n, C, S, K, M, P = args.n, args.chains, args.slots, w2["K"], w2["M"], w2["P"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w2["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w2["y"], w2["t"], w2["internal_knots"], w2["boundary_knots"], n_chains=C)
    for q in range(C):
        smp.select_chain(q)
        smp.set_state(**w2["state"])
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    pairs = n * C * S
    out = {"what": "loo_marginal", "reps": args.reps, "n": n, "K": K, "M": M, "P": P, "chains": C, "slots": S, "draws": C * S,
           "points": int(len(w2["y"][0])), "J": args.J, "pairs": pairs}
    smp.loo_marginal(n_slots=min(S, 24), n_samples=args.J, n_stages=1)      # warm-up: the kernels are loaded
    for R in (1, 3):
        for refine in (False, True):
            wall, dev, dev_psis = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                res = smp.loo_marginal(n_samples=args.J, n_stages=R, seed=1, refine=refine)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms, launches = smp.timing("loo_marginal")
                dev.append(ms)
                dev_psis.append(smp.timing("loo_marginal_psis")[0])
            row = {"device_ms": med(dev), "launches": launches, "psis_device_ms": med(dev_psis), "psis_launches": smp.timing("loo_marginal_psis")[1],
                   "end_to_end_ms": med(wall), "share_refined": float(np.sum(res["n_refined"], dtype=np.int64)) / pairs,
                   "share_below_floor": float(np.sum(res["n_below"], dtype=np.int64)) / pairs,
                   "curves_with_pairs_below": int(np.sum(res["n_below"] > 0)),
                   "median_ess_mean": float(np.median(res["ess_mean"])), "min_ess_min": float(np.min(res["ess_min"])),
                   "refine_samples": res["refine_samples"], "refine_stages": res["refine_stages"], "ess_floor": res["ess_floor"]}
            row.update(khat(res))
            out[f"R{R}_{'refined' if refine else 'first_pass'}"] = row
            print(json.dumps({f"R{R}_refine{int(refine)}": row}), file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    cond = smp.loo()
    out["loo_conditional"] = dict(khat(cond), end_to_end_ms=(time.perf_counter() - t0) * 1e3)
    if not args.no_composed:
        for R in (1, 3):
            t0 = time.perf_counter()
            pr = smp.predict(w2["y"], w2["t"], n_samples=args.J, n_stages=R, seed=1, trace=True)
            t1 = time.perf_counter()
            ps = api.psis_loo(pr["lpd_trace"].reshape(n, -1))
            t2 = time.perf_counter()
            out[f"composed_R{R}"] = {"predict_trace_ms": (t1 - t0) * 1e3, "psis_loo_ms": (t2 - t1) * 1e3, "end_to_end_ms": (t2 - t0) * 1e3,
                                     "predict_device_ms": smp.timing("predict")[0], "elpd_loo": float(ps["elpd_loo"])}
            del pr, ps
    smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
