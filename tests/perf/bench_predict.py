#!/usr/bin/env python3
"""Times the prediction of held-out curves (kernels_predict.hip) on one MI355X at the config-2 shape: K = 3, P = 30,
M = 6, 8 chains x 500 slots = 4000 draws, n_new = 256 new curves of 100 points, J = 256 samples, R = 1 and R = 3 stages, and one
stage on given samples (z_samples), which is the work of R = 1 without its gamma variates.  The sampler
is fitted to --n-train curves of the same data (the cost of a prediction does not depend on it); the chains start from the
generating state.  For each R, medians of --reps calls after a warm-up call of the device time of "predict" (k_predict and
k_predict_pool) and of "predict_stats" (HIP events on the sampler's stream, Sampler.timing) and of the end-to-end time of
Sampler.predict; the arithmetic of the call counted from the shape and set against the vector and matrix fp64 rates of the device
(78.6 TFLOP/s each); and the numpy reference of tests/predict_ref.py (dense l at J samples, one stage) timed on --ref-pairs
(curve, draw) pairs and scaled to the n_new x 4000 x R of the call.  Not the bench line.  One JSON line.

  python tests/perf/bench_predict.py [--n-train 512] [--n-new 256] [--chains 8] [--slots 500] [--J 256] [--reps 5] [--ref-pairs 4]
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

PEAK_TFLOPS = 78.6      # fp64, vector and matrix alike


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def flops(K, M, P, BW, J, R):
    """multiply-adds x 2 of one (curve, draw): the band product and tau (vector), Gamma's upper-triangle tiles as the MFMA runs them
    (padding included), and per sample the K^2 + K multiply-adds of each of the (M + 1)(M + 2) / 2 table sums and the Cholesky"""
    A = K * (M + 1)
    AT, PP = (A + 15) // 16, (P + 3) // 4 * 4
    vec_draw = 2.0 * A * P * (2 * BW + 1) + 2.0 * A * P
    mat_draw = 2.0 * (AT * (AT + 1) // 2) * 256 * PP
    per_sample = 2.0 * ((M + 1) * (M + 2) // 2) * (K * K + K) + 2.0 * (M ** 3 / 3.0 + M * M)
    return vec_draw + R * J * per_sample, mat_draw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=512)
    ap.add_argument("--n-new", type=int, default=256)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--J", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-pairs", type=int, default=4)
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    import predict_ref as PR
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
    out = {"what": "predict", "reps": args.reps, "K": K, "M": M, "P": P, "chains": C, "slots": S, "draws": C * S, "n_new": args.n_new,
           "points": int(len(yn[0])), "J": args.J, "n_train": nt}
    pairs = args.n_new * C * S
    zs = np.random.default_rng(2).dirichlet(np.full(K, 2.0), size=(C, S, args.J))
    for R in (1, 3, 0):          # 0: one stage on given samples (the deterministic hook): the same work without the variates
        wall, dev, dev_stats = [], [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            res = smp.predict(yn, tn, n_samples=args.J, n_stages=max(R, 1), seed=1, z_samples=zs if R == 0 else None)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, launches = smp.timing("predict")
            dev.append(ms)
            dev_stats.append(smp.timing("predict_stats")[0])
        vec, mat = flops(K, M, P, w2["degree"], args.J, max(R, 1))
        d = med(dev[1:])
        out[f"R{R}" if R else "R1_given_samples"] = {"predict_device_ms": d, "predict_launches": launches, "predict_stats_device_ms": med(dev_stats[1:]),
                        "end_to_end_ms": med(wall[1:]), "vector_gflop": vec * pairs / 1e9, "matrix_gflop": mat * pairs / 1e9,
                        "vector_share_of_peak": vec * pairs / (d * 1e-3) / (PEAK_TFLOPS * 1e12),
                        "matrix_share_of_peak": mat * pairs / (d * 1e-3) / (PEAK_TFLOPS * 1e12),
                        "elpd": res["elpd"], "median_ess_mean": float(np.median(res["ess_mean"])), "min_ess_min": float(np.min(res["ess_min"]))}
    # the numpy reference on a few (curve, draw) pairs: the dense l at J prior samples and the stage rule, scaled
    chains = {nm: smp.get_chain(nm) for nm in ("nu", "Phi", "sigma_sq", "pi", "alpha_3")}
    rng = np.random.default_rng(1)
    B = w2["B"][nt:]
    t0 = time.perf_counter()
    for i in range(args.ref_pairs):
        r, s = i % args.n_new, (i * 97) % S
        th = PR.directions(chains["nu"][..., s], chains["Phi"][..., s])
        prior = chains["alpha_3"][s] * chains["pi"][:, s]
        z = np.maximum(rng.dirichlet(prior, size=args.J), PR.TINY)
        PR.stage(PR.ell_dense_batch(B[r], yn[r], th, z, float(chains["sigma_sq"][s])), z)
    per_pair = (time.perf_counter() - t0) / max(args.ref_pairs, 1)
    out["numpy_reference"] = {"pairs_timed": args.ref_pairs, "ms_per_pair_and_stage": per_pair * 1e3,
                              "scaled_s_R1": per_pair * pairs, "scaled_s_R3": per_pair * pairs * 3}
    smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
