"""k_factor on its own, on every instantiation (PP = 32 / 64 x band widths 0-5, BWMID, BWWIDE): C_a = Prec_a^-1 and L_a z_a as the
kernel leaves them (bfmmm_debug_get "Cmat", "Lz") against the longdouble inverse of tests/factor_ref.py, direction by direction,
in the equilibrated frame and under the bounds derived there (err <= g P 2^-53 kappa_s; the diagonal model to 16 units of
2^-53 per entry; the pseudo-inverse route against pinv_ld).

Every case (factor_ref.CASES: n = 24 ragged curves, A <= 9 directions) pushes a state, runs ONE iteration with the mask
U_NU | U_PHI -- every input of Prec_a is then the pushed state and H the contraction of the pushed Z, chi -- asserts the
instantiation through dims(), builds Prec_a from the device's own band rows of H_aa and compares.  Regimes: benign
(random_state's scales, kappa_s 3 .. 560), stiff (sigma^2 = 1e-5, tau 1e2 .. 1e4, tilde_tau to ~1e3, gamma over six decades,
rank-deficient data: the largest kappa_s of a case 1.0e6 .. 2.9e7), prior-dominated (one cluster with Z_ik = 1e-4) and a cluster
without members (pseudo-inverse route, kappa+ 27 .. 650); one two-chain case pins chain_ctx's offsets into Cmat / Lz.
z comes from the oracle's keyed generator with k_factor's index layout (factor_ref.normals; the layout itself is asserted in
tests/test_factor_ref.py and below).  r_a = t_a - sum_b H_ab theta_b and H_aa theta_a, which k_factor writes and the sweep only
copies, are checked per entry on the cubic cases with (A (2 BW + 1) + 4) 2^-53 S_abs."""
import numpy as np
import pytest

import factor_ref as F

pytestmark = pytest.mark.gpu


def make_sampler(c):
    import bayesfmmm_amd as bf
    d = F.case_data(c)
    if c.kind == "mv":
        cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=c.K, n_eigen=c.M, tot_mcmc_iters=2)
        return bf.Sampler(cfg, d["Y"], n_chains=c.nch)
    if c.kind == "spline":
        cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=c.deg, tot_mcmc_iters=2)
        return bf.Sampler(cfg, d["y"], d["t"], d["ik"], d["bk"], n_chains=c.nch)
    cfg = bf.default_config(model=bf.MODEL_FUNCTIONAL, K=c.K, n_eigen=c.M, basis_degree=max(c.degs), tot_mcmc_iters=2)
    return bf.Sampler(cfg, d["y"], basis=d["B"], band=c.band, penalty=d["Pmat"], penalty_band=c.pen_band, n_chains=c.nch)


def run_case(c):
    """one iteration; per chain: (state, H, tvec, Cmat, Lz, rvec, hq)"""
    import bayesfmmm_amd as bf
    S = bf.sampler
    smp = make_sampler(c)
    states = [F.case_state(c, q) for q in range(c.nch)]
    for q, st in enumerate(states):
        smp.select_chain(q)
        smp.set_state(**st)
    smp.run(S.U_NU | S.U_PHI, 1, seed=F.SEED, chain=0)
    d = smp.dims()
    # the instantiation the case was written for
    assert (d["n"], d["K"], d["P"], d["M"], d["MD"], d["A"]) == (c.n, c.K, c.P, c.M, c.MD, c.A), d
    assert (d["BW"], d["BWP"]) == (c.BW, c.BWP), f"{c.name}: dims report BW {d['BW']}, BWP {d['BWP']}; written for {c.BW}, {c.BWP}"
    assert (32 if d["P"] <= 32 else 64) == c.PP and d["LG"] == (c.BW + 1) * c.P
    out = []
    A, P = c.A, c.P
    for q, st in enumerate(states):
        smp.select_chain(q)
        assert np.array_equal(smp.get_state("Z"), st["Z"]) and np.array_equal(smp.get_state("sigma_sq").ravel(), st["sigma_sq"])
        out.append((st, smp.debug("H").reshape(d["R"], d["LG"]), smp.debug("tvec").reshape(A, P), smp.debug("Cmat").reshape(A, P, P),
                    smp.debug("Lz").reshape(A, P), smp.debug("rvec").reshape(A, P), smp.debug("hq").reshape(A, P)))
    smp.close()
    return out


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_factor_against_longdouble_inverse(name):
    import oracle_lib as O
    c = F.BY_NAME[name]
    # the generator's element i is the variate of counter index i whatever the count: what normals()' slicing relies on
    assert np.array_equal(O.fill(1, c.P + 3, seed=F.SEED, upd=F.UPD_NU)[c.P:], O.fill(1, c.K * c.P, seed=F.SEED, upd=F.UPD_NU)[c.P:c.P + 3])
    worst = []
    out = run_case(c)
    for q, (st, H, tv, Cm, Lz, rv, hq) in enumerate(out):
        z = F.normals(c, q)
        hb = F.hbands_from_H(c, H)
        assert np.isfinite(Cm).all() and np.isfinite(Lz).all(), f"{name}, chain {q}: Cmat / Lz not finite"
        precs = F.precisions(c, hb, st)
        for a in range(c.A):
            r = F.check_direction(c, a, precs[a], Cm[a], Lz[a], z[a])
            print(f"chain {q}: {r['msg']}  [error / bound: C {r['rC']:.3g}, Lz {r['rL']:.3g}]")
            worst.append((max(r["rC"], r["rL"]), q, r))
            # Cmat[a] holds C(p, q) at [p, q] and at [q, p]: the Cholesky route computes both triangles from separate MFMA tiles
            # in the same order of k (bit-equal), the diagonal branch stores zeros; the pseudo-inverse route multiplies in
            # another order per triangle and is held to the bound only
            asym = np.abs(Cm[a] - Cm[a].T).max()
            if r["route"] != "pinv":
                assert asym == 0.0, f"chain {q}: {r['msg']}: C is not symmetric bit for bit (largest difference {asym:.3g})"
            else:
                print(f"   pseudo-inverse route: largest |C - C'| = {asym:.3g}")
        bad = [(w, q2, r) for w, q2, r in worst if not r["ok"]]
        assert not bad, "\n".join(f"chain {q2}: {r['msg']}" for _, q2, r in bad)
    if c.nch > 1:       # the chains hold different states: a chain offset into Cmat / Lz would have compared the wrong one
        assert not np.array_equal(out[0][3], out[1][3])


@pytest.mark.parametrize("name", ["cubic_P30-benign", "cubic_P30-stiff"])
def test_rvec_and_hq_entry_by_entry(name):
    c = F.BY_NAME[name]
    st, H, tv, Cm, Lz, rv, hq = run_case(c)[0]
    r, ra, h, ha = F.rvec_ref(c, H, tv, st)
    for nm, got, ref, sabs in (("rvec", rv, r, ra), ("hq", hq, h, ha)):
        err = np.asarray(np.abs(got.astype(F.LD) - ref), dtype=np.float64)
        b = F.rvec_bound(c, sabs)
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(got == 0.0, 0.0, np.inf))
        a, p = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"{name}: {nm}: worst error / bound {ratio[a, p]:.3g} at a {a}, p {p}")
        assert ratio[a, p] <= 1.0, (f"{name}: {nm}[a {a} = (j {a // c.MD}, mt {a % c.MD}), p {p}] = {got[a, p]!r}, reference "
                                    f"{float(ref[a, p])!r}: error / bound {ratio[a, p]:.3g}, bound (A (2 BW + 1) + 4) 2^-53 S_abs")
