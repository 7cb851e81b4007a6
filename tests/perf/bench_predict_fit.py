#!/usr/bin/env python3
"""Times the fitted function of held-out curves (kernels_predict_fit.hip) on one MI355X at the shape of
tests/perf/bench_predict.py (K = 3, P = 30, M = 6, 8 chains x 500 slots = 4000 draws, n_new = 256 new curves of 100 points, J = 256
samples) on a grid of G = 48 rows, at R = 1 and R = 3 stages, and `Sampler.predict` at the same shape in the same session: for
each, medians of --reps calls after a warm-up call of the device time ("predict_fit": k_predict_fit, the two pooling kernels and the
quantiles of the paths; "predict": k_predict and k_predict_pool; HIP events on the sampler's stream, Sampler.timing) and of the
end-to-end time of the call, and the ratio predict_fit / predict of both.  The chains start from the generating state.  Not the
bench line.  One JSON line.

  python tests/perf/bench_predict_fit.py [--n-train 512] [--n-new 256] [--chains 8] [--slots 500] [--J 256] [--G 48] [--reps 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=512)
    ap.add_argument("--n-new", type=int, default=256)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--J", type=int, default=256)
    ap.add_argument("--G", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    w2 = bench.make_config2(n=args.n_train + args.n_new)
    nt, C, S, K, M, P = args.n_train, args.chains, args.slots, w2["K"], w2["M"], w2["P"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w2["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w2["y"][:nt], w2["t"][:nt], w2["internal_knots"], w2["boundary_knots"], n_chains=C)
    st = dict(w2["state"])
    st["Z"], st["chi"] = np.asarray(st["Z"])[:nt], np.asarray(st["chi"])[:nt]
    for q in range(C):
        smp.select_chain(q)
        smp.set_state(**st)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    yn, tn = w2["y"][nt:], w2["t"][nt:]
    Bfull = np.asarray(w2["B"][0])
    E = Bfull[np.linspace(0, Bfull.shape[0] - 1, args.G).astype(int)]
    out = {"what": "predict_fit", "reps": args.reps, "K": K, "M": M, "P": P, "chains": C, "slots": S, "draws": C * S, "n_new": args.n_new,
           "points": int(len(yn[0])), "J": args.J, "G": args.G, "n_train": nt}
    for R in (1, 3):
        row = {}
        for what in ("predict", "predict_fit"):
            wall, dev = [], []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                if what == "predict":
                    res = smp.predict(yn, tn, n_samples=args.J, n_stages=R, seed=1)
                else:
                    res = smp.predict_fit(yn, E, tn, n_samples=args.J, n_stages=R, seed=1)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms, launches = smp.timing(what)
                dev.append(ms)
            row[what] = {"device_ms": med(dev[1:]), "launches": launches, "end_to_end_ms": med(wall[1:]), "elpd": res["elpd"]}
        row["same_elpd_bits"] = row["predict"]["elpd"] == row["predict_fit"]["elpd"]
        row["ratio_device"] = row["predict_fit"]["device_ms"] / row["predict"]["device_ms"]
        row["ratio_end_to_end"] = row["predict_fit"]["end_to_end_ms"] / row["predict"]["end_to_end_ms"]
        row["median_sd"] = float(np.median(res["sd"]))
        out[f"R{R}"] = row
    smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
