#!/usr/bin/env python3
"""Times the cluster eigenvalues and eigenfunctions (kernels_cluster_eig.hip) on one MI355X in two settings:
  - the README shape: n = 4096 curves, K = 3, config 2's P = 30 and M = 6, 8 chains x 500 slots = 4000 draws, a grid of G = 48
    points with weights 1 / G and the J = 2 leading eigenfunctions, the chains started from the generating state with their labels
    permuted;
  - the limits: the multivariate model at P = 64, M = 16 with E = I (G = 64), 4 chains x 250 slots = 1000 draws, J = 2, at K = 3:
    the kernels here take K = 8, but the sampler's own sweep kernel holds 5 K (M + 1) P doubles in LDS and runs no more
    components than that at this P and M, so no chain with more exists to be read.
For each, medians of --reps calls after a warm-up call of the end-to-end time of Sampler.cluster_eigen with a given reference
(ref as an array: the call itself, no host eigh of the mean surface) and of the device times of k_ceig_gram, k_ceig_solve and
k_ceig_values (HIP events on the sampler's stream, Sampler.timing); the same call with ref="mean", without quantiles, with
n_functions = 0 and with either form of S_k in k_ceig_solve (plain multiplies and additions, MFMA) set explicitly; and the route
without it, timed once: get_chain("Phi") of every chain to the host, the relabelling, einsum and numpy.linalg.eigh of W^1/2 E Theta Theta' E' W^1/2 per draw and component.  Checks the device's mean eigenvalues against numpy's.
Not the bench line.  One JSON line.

  python tests/perf/bench_cluster_eig.py [--n 4096] [--chains 8] [--slots 500] [--reps 3] [--G 48] [--J 2] [--skip-limits]
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

TIMERS = ("cluster_eig_gram", "cluster_eig", "cluster_eig_values")


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


def setting(smp, E, w, J, reps):
    """the timings of one sampler that has run; perm from the last slot of chain 0"""
    C, S, K = smp.n_chains, smp.T, smp.K
    N, G = C * S, E.shape[0]
    perm = smp.align(pivot=(0, S - 1))["perm"]
    first = smp.cluster_eigen(E, perm, weights=w, n_functions=J)               # ref="mean": also the warm-up
    ref = first["ref"]
    res = {"ref_array": timed(smp, lambda: smp.cluster_eigen(E, perm, weights=w, n_functions=J, ref=ref), reps),
           "ref_mean": timed(smp, lambda: smp.cluster_eigen(E, perm, weights=w, n_functions=J), reps),
           "ref_none": timed(smp, lambda: smp.cluster_eigen(E, perm, weights=w, n_functions=J, ref=None), reps),
           "no_quantiles": timed(smp, lambda: smp.cluster_eigen(E, perm, weights=w, n_functions=J, ref=ref, probs=()), reps),
           "values_only": timed(smp, lambda: smp.cluster_eigen(E, perm, weights=w, n_functions=0, ref=None), reps)}
    # the two forms of S_k in k_ceig_solve, each set explicitly (0 afterwards: the launcher's choice, which the rows above ran)
    for name, form in (("form_fma", 1), ("form_mfma", 2)):
        smp.lib.bfmmm_set_cluster_eig_form(form)
        try:
            res[name] = timed(smp, lambda: smp.cluster_eigen(E, perm, weights=w, n_functions=J, ref=ref), reps)
        finally:
            smp.lib.bfmmm_set_cluster_eig_form(0)
    # the host route: the chains to the host, then numpy
    t0 = time.perf_counter()
    phis = []
    for q in range(C):
        smp.select_chain(q)
        phis.append(smp.get_chain("Phi"))                                      # (K, P, M, S)
    smp.select_chain(0)
    t1 = time.perf_counter()
    sw = np.sqrt(w)
    lam = np.zeros((K, smp.M, N))
    for q in range(C):
        W = np.einsum("g,gp,kpms->skgm", sw, E, phis[q])[np.arange(S)[:, None], perm[q]]       # (S, K, G, M), aligned
        A = np.einsum("skgm,skhm->skgh", W, W)
        val, vec = np.linalg.eigh(A)
        lam[:, :, q * S:(q + 1) * S] = np.transpose(val[:, :, ::-1][:, :, :smp.M], (1, 2, 0))
    t2 = time.perf_counter()
    res["host_route"] = {"get_chain_Phi_ms": (t1 - t0) * 1e3, "numpy_einsum_eigh_ms": (t2 - t1) * 1e3}
    res["max_abs_mean_lambda_minus_numpy"] = float(np.max(np.abs(first["values"]["mean"] - lam.mean(axis=-1))))
    res["max_mean_lambda"] = float(np.max(first["values"]["mean"]))
    res["max_sweeps"] = first["max_sweeps"]
    res.update(K=K, M=smp.M, P=int(E.shape[1]), chains=C, slots=S, draws=N, G=G, J=J)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--slots", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--G", type=int, default=48)
    ap.add_argument("--J", type=int, default=2)
    ap.add_argument("--lim-chains", type=int, default=4)
    ap.add_argument("--lim-slots", type=int, default=250)
    ap.add_argument("--skip-limits", action="store_true")
    args = ap.parse_args()
    import bayesfmmm_amd as bf
    import bench
    out = {"what": "cluster_eig", "reps": args.reps}

    w2 = bench.make_config2(n=args.n)
    C, S, K, M = args.chains, args.slots, w2["K"], w2["M"]
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=K, n_eigen=M, basis_degree=w2["degree"], tot_mcmc_iters=S)
    smp = bf.Sampler(cfg, w2["y"], w2["t"], w2["internal_knots"], w2["boundary_knots"], n_chains=C)
    rng = np.random.default_rng(3)
    all_perms = list(itertools.permutations(range(K)))
    for q in range(C):
        p = list(all_perms[q % len(all_perms)])
        st = dict(w2["state"])
        st["nu"] = st["nu"] + 0.05 * rng.standard_normal(st["nu"].shape)
        for nm in ("nu", "Phi", "pi", "delta", "A", "gamma", "tau"):
            st[nm] = np.asarray(st[nm])[p]
        st["Z"] = np.asarray(st["Z"])[:, p]
        smp.select_chain(q)
        smp.set_state(**st)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, S, seed=1)
    E = np.ascontiguousarray(np.concatenate(smp.get_basis(), axis=0)[:args.G])
    out["readme_shape"] = dict(setting(smp, E, np.full(args.G, 1.0 / args.G), args.J, args.reps), n=w2["n"])
    smp.close()

    if not args.skip_limits:
        n, P, K, M = 256, 64, 3, 16
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=M, tot_mcmc_iters=args.lim_slots)
        smp = bf.Sampler(cfg, np.random.default_rng(4).standard_normal((n, P)), n_chains=args.lim_chains)
        for q in range(args.lim_chains):
            smp.select_chain(q)
            smp.init_state(1, 17, chain=q)
        smp.select_chain(0)
        smp.run(bf.SWEEP_WARM, args.lim_slots, seed=17)
        out["limits"] = dict(setting(smp, np.eye(P), np.ones(P), args.J, args.reps), n=n)
        smp.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
