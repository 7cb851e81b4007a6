"""High-precision restatement of the eta / Xi covariate block (csrc/kernels_cov.hip: k_cov_prep, k_cov_w2, k_cov_factor,
k_cov_group, k_cov_hyper), its per-entry checks, bounds, two float64 emulations and the case list shared by
tests/test_cov_ref.py (CPU) and tests/test_gpu_cov.py (device).  (Test infrastructure.)

Directions.  a2 = 0 .. A2 - 1 in the order of the sweep (dir2_of): eta first, d outer and j inner (a2 = d K + j; UpdateEta.h:28-94),
then Xi in (j, m, d) order (a2 = K D + (j M + m) D + d; UpdateXi.h:26-93).  D consecutive directions are a GROUP (one k_cov_group
launch); in-group pair (u <= v) of group g is row g D(D+1)/2 + v(v+1)/2 + u of "H2aa".  The weight of curve i in direction
a = (j, mt, d) is w_{a,i} = Z_ij x_id (mt = 0) or (Z_ij x_id) chi_{i,mt-1}.  u = 2^-53; everything below is np.longdouble.

Which sigma^2 the block reads.  An iteration launches k_curve_z, the pair-Gram kernels, k_factor, the SWEEP (whose scalar job draws
sigma^2 when the mask has U_SIGMA and stores it in Dyn and the chain slot), k_curve_chi and then launch_cov_block; k_loglik follows
it.  So f = beta / sigma^2 of the block is the sigma^2 of the SAME iteration's slot -- the pushed one when the mask has no U_SIGMA.

Inputs are the device's own arrays: rec_i = [G_i band rows | s_i | yy_i], the block's intermediates ("Wdir", "H2aa", "C2", "Lz2"),
the theta it started from (the pushed state or a chain slot) and the theta it committed, and c_i^0, g_i^0: "cfull" / "gfull" as
k_curve_chi left them, read after a run of the same state whose mask has neither U_ETA nor U_XI (the residual-only pass stores
nothing behind k_curve_chi), or restated from the chain slots for a full sweep.  Every quantity is judged alone.

Wdir (check_wdir): bit-equal to the float64 product (Z_ij x_id) chi_im -- pure products, nothing to contract.

H2aa (check_h2aa): every in-group pair of every updated group, every band element e, against sum_i w_u,i w_v,i G_i[e] from the
device's Wdir and rec under  G_H c_H u S_abs[e],  S_abs the sum of absolute terms, c_H = 2 + 128 + 1 + NB2: a term is two products
(w_v r, then w_u (w_v r): the second may be fused into the addition, which only removes a rounding), passes at most 128 additions
of its chunk (64 and the merge of the two halves in the two-half form) and the NB2 additions of the chunk sums.

C2, Lz2 (check_factor): factor_ref's references and bounds unchanged (k_cov_factor calls the same factor_core / factor_pinv):
Prec_a = f band(H_aa) + Prior_a with the DEVICE's diagonal pair block; Prior: eta tau_eta(j, d) P_mat, multivariate model
(1 / tau_eta) I; Xi diag(prod_{m' <= m} delta_xi(j, m', d) gamma_xi_j(., d, m)).  Cholesky route: err_C <= G_C P u kappa_s and
err_Lz <= G_L P u kappa_s + (32 + 4 sqrt(P) / |z|) u, the last term the AS241 allowance of curve_update_ref.check_chi_norm (the
device's normal against the oracle's keyed rnorm, UPD_ETA index (d K + j) P + p, UPD_XI index ((j M + m) D + d) P + p) carried
through L in the scaled frame.  Diagonal model (multivariate): factor_ref.check_diag, 16 u entrywise (Lz: + 36 u for the normal).
Pseudo-inverse route (an eta direction of a cluster without members): err_C <= G_J P u kappa+ and
the null component of Lz as in factor_ref.check_direction.

Each draw alone (check_steps).  With delta_a' = theta_new,a' - theta_old,a' of the device for the directions visited before a
(earlier groups and earlier directions of the same group alike: the check does not depend on the off-diagonal pair blocks),
    dc_i = sum_{a' before a} w_{a',i} delta_a',   r_a = sum_i w_a,i (s_i - g_i^0 - G_i dc_i),
    rhs = f (r_a + H_aa theta_old,a),   theta_ref = Cbar_a rhs + Lz_a,   Cbar = (C + C') / 2
under G_STEP times
    sum_q |Cbar_pq| (f c_r u S_q + (P + 3) u |rhs_q|) + sum_q |C_pq - C_qp| |rhs_q| + 2 u (|Lz_p| + |theta_ref,p|)
    S_q = sum_i |w_a,i| (|s_i| + |g_i^0| + |G_i| |dc|_i)[q] + (|H_aa| |theta_old,a|)[q],   |dc|_i = sum |w_a',i| |delta_a'|
    c_r = (k + 1)(2 BW + 2 + D) + GPB + NBS + 48
k the number of groups applied before a's.  Derivation: the device's g_i is updated once per applied group: v_i = sum_s w_s delta_s
(a product and at most D additions per term, the delta itself a rounded difference), G_i v_i (2 BW + 1 additions and a product) and
the addition to g_i: 2 BW + 2 + D roundings per group at most, and one more group's worth for the in-group terms H_su delta_u
(a band product, the subtraction, the split over the lanes of a row).  w (s - g): a subtraction and a product; the COV_CPG curves
of a lane group, the GPB lane groups of a workgroup and the NBS block sums (32 segments, then the segments) in any order: at most
2 + GPB + NBS + 32 additions; r + H_aa theta (a band product), f and its division: 14 spare in the 48.  The mat-vec part is the
sweep's (sweep_ref, parts iii-v).  Nothing is scaled by a global maximum; directions outside the mask come back BIT-EQUAL.

Final cfull, gfull (check_final): cfull against c^0 + sum_a w_a,i delta_a under G_CF (D + 1 + n_g) u (|c^0| + |dc|) + u |c_ref|; gfull
against g^0 + G_i (c_ref - c^0) -- G_i c up to the error of the input g^0, which test_gpu_curve_update bounds -- under
G_GF (2 BW + 2 + D + n_g) u (|g^0| + |G| |dc|) + u |g_ref|; n_g the number of groups applied.  A mask without U_ETA and U_XI must
leave both bit-equal.

Full sweeps (theta, Z, chi move in the same iteration): c^0, g^0 are restated in longdouble from the chain slots (restate_c0), and
the bounds curve_update_ref.check_cfull holds k_curve_chi's cfull / gfull to against exactly those values, e_c and e_g, are carried:
f sum_q |Cbar_pq| sum_i |w_a,i| e_g,i[q] joins the step bound, e_c and e_g the bounds of the final cfull and gfull.

rss_part (check_rss): entry b of workgroup b of the closing k_cov_group launch (CPB = 2 * 1024 / LPC curves) against
sum_{i in b} (yy_i - 2 c_i's_i + c_i'g_i) from the device's final cfull and gfull under G_RSS2 c_R u S_abs, c_R = LPC + GPB + 8
(two LPC-lane sums in any order, their products, the three-term sum, COV_CPG curves, GPB lane groups); entries NBS .. nblk_curve - 1
are exactly 0; Dyn::rss, sigma_sq / loglik by curve_update_ref.check_total_and_loglik.

Hyper parameters (check_hyper), from the device's committed eta / xi and "gstd2":
    tau_eta(j, d)   = g / (beta_eta + eta_jd'P_mat eta_jd / 2)      (multivariate: the quadratic form is eta'eta, and the stored value 1 / that)
    delta_xi(j, i, d): the sequential recursion of UpdateDelta.h:76-124 within a (d, j) cell, the cell's NEW delta for i' < i
    gamma_xi(p, d, m, j) = g 2 / (nu_1 + prod_{m' <= m} delta_xi,new(j, m', d) xi^2)
each under a few u of its sum of absolute terms, with a constant of its own and no term count (the errors these operations show
do not grow with P or M): tau_eta G_TAU u |value| amp, amp = (beta_eta + |eta|'|P_mat| |eta| / 2) / (beta_eta + eta'P_mat eta / 2), the
cancellation inside the quadratic form (P_mat is positive semi-definite but its entries are not); delta_xi G_DELTA u |value| and gamma_xi
G_GAMMA u |value| (every term of their sums is non-negative).  Entries whose
mask bit is off come back bit-equal, and the chain slot equals the working state bit for bit.  "gstd2" itself is held to the oracle's
keyed standard gamma variates (check_gstd2) and the A_xi step cell by cell to the oracle's keyed proposal and a longdouble
acceptance value (check_axi); their tolerances follow from the AS241 allowance and are derived in the docstrings.

Constants.  As everywhere in DESIGN.md section 2: 4 x the largest error / (bound at G = 1) that two float64 emulations show over
every case of CPU_CASES -- `kernel` follows the kernels' order (128-curve chunks in two halves, chunk sums; per-workgroup partial
sums over lane groups, 32 segments over workgroups; in-group pair blocks with the band product diagonal first; g_i updated
incrementally), `plain` a plainly different one (BLAS products, g_i = G_i c_i recomputed from c_i at every direction, sums over all
curves at once).  Measured by tests/test_cov_ref.py::test_emulations_pass_and_constants_hold, never from a device run:

    H2aa:     kernel 0.058 (cubic_P30_D2_n129-benign),  plain 0.0556 (cubic_P30_D2_n257-benign)   ->  G_H = 0.232
    step:     kernel 0.0177 (mv_P7_D2-benign),          plain 0.0161 (lin_P33_D2-benign)          ->  G_STEP = 0.071
    cfull:    kernel 0.45, plain 0.399 (cubic_P30_D2-benign)                                      ->  G_CF = 1.8
    gfull:    kernel 0.188 (mv_P40_D3-benign),          plain 0.637 (cubic_P30_D2-stiff)          ->  G_GF = 2.55
    rss_part: kernel 0.0339, plain 0.0349 (cubic_P30_D2_n129-benign)                              ->  G_RSS2 = 0.14
    tau_eta:  kernel 4.0 u (cubic_P30_D2_n129-benign),  plain 3.66 u (quint_P47_D8-benign)        ->  G_TAU = 16
    delta_xi: kernel 4.15 u (cubic_P30_D2_n128-benign), plain 2.56 u (cubic_P40_D2-benign)        ->  G_DELTA = 16.6
    gamma_xi: kernel 2.74 u (cubic_P25_D8-benign),      plain 2.46 u (step_P10_pen1_D2-benign)    ->  G_GAMMA = 11

The largest step bound is 1.07e-8 of the |delta| it judges (cubic_P30_D2-stiff: kappa_s 8.31e6, smallest pivot ratio 1.75e-8).  Every step bound must stay below 1e-3 of the |delta| it judges (NONVACUOUS).
"""
import zlib

import numpy as np

import curve_update_ref as R
import factor_ref as F
import sweep_ref as S

U, LD = F.U, F.LD
SEED = F.SEED
UPD_ETA, UPD_XI = 16, 18            # update ids of the keyed generator (oracle/oracle.h, csrc/rng.hpp)
U_SIGMA, U_LOGLIK = 1 << 9, 1 << 17
U_ETA, U_TAU_ETA, U_XI, U_DELTA_XI, U_A_XI, U_GAMMA_XI = (1 << i for i in range(11, 17))
COV_MEAN = U_ETA | U_TAU_ETA
COV_XI = U_XI | U_DELTA_XI | U_A_XI | U_GAMMA_XI
W2_CH, GT, COV_CPG = 128, 1024, 2   # csrc/kernels_cov.hip
NONVACUOUS = 1e-3

# measured by tests/test_cov_ref.py::test_emulations_pass_and_constants_hold (largest error / bound at G = 1 over CPU_CASES)
MEASURED_H = {"kernel": 0.058, "plain": 0.0556}
MEASURED_STEP = {"kernel": 0.0177, "plain": 0.0161}
MEASURED_CF = {"kernel": 0.45, "plain": 0.399}
MEASURED_GF = {"kernel": 0.188, "plain": 0.637}
MEASURED_RSS2 = {"kernel": 0.0339, "plain": 0.0349}
MEASURED_TAU = {"kernel": 4.0, "plain": 3.66}          # (these three in units of u: the bounds carry no term count)
MEASURED_DELTA = {"kernel": 4.15, "plain": 2.56}
MEASURED_GAMMA = {"kernel": 2.74, "plain": 2.46}
G_H, G_STEP, G_CF, G_GF, G_RSS2 = 0.232, 0.071, 1.8, 2.55, 0.14
G_TAU, G_DELTA, G_GAMMA = 16.0, 16.6, 11.0


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class CovCase(R.CurveCase):
    """curve_update_ref.CurveCase with n of its own, the multivariate / empty-cluster / stiff states of the covariate block"""
    def __init__(self, name, n=R.N_CURVES, D=2, cov_adj=True, **kw):
        super().__init__(name=name, D=D, **kw)
        self.n = n
        self.nblk = -(-self.n // self.GPB)
        self.cov_adj = cov_adj
        self.A2 = self.K * D * (1 + (self.M if cov_adj else 0))
        self.CPB = COV_CPG * GT // self.LPC
        self.NBS = -(-self.nblk // (4 * COV_CPG))
        self.NB2 = -(-self.n // W2_CH)
        self.NPG = D * (D + 1) // 2
        self.LG = (self.BW + 1) * self.P


def _case(inst, D=2, regime="benign", special=None, suffix="", **kw):
    d = dict(R._INST[inst]) if inst in R._INST else dict(name=inst)
    d.update(kw)
    nm = f"{inst}_D{D}{suffix}-{special or regime}"
    d.pop("name", None)
    return CovCase(name=nm, D=D, regime=regime, special=special, **d)


def _cases():
    kw2 = dict(K=2, M=2)
    out = [_case(i, **kw2) for i in ("lin_P6", "lin_P33", "quad_P29", "quad_P64", "cubic_P30", "cubic_P40", "quart_P32", "quart_P50",
                                     "quint_P27", "quint_P47", "mid_5x5", "wide_7x7")]
    out.append(_case("step_P10_pen1", kind="step", P=10, pen_band=1, **kw2))
    out += [_case(i, D=D, **kw2) for i in ("cubic_P30", "cubic_P40") for D in (1, 3, 4, 5, 6, 7, 8)]
    # (P 30 at D = 7, 8 is refused, see REFUSED: the 32-lane instances of D = 7, 8 and D P = 200 > 192 at 32 lanes are reached at P = 25)
    out += [_case("cubic_P25", D=D, kind="spline", deg=3, P=25, **kw2) for D in (7, 8)]
    out += [_case("quad_P29", D=3, **kw2), _case("quint_P27", D=1, **kw2), _case("quint_P47", D=8, **kw2), _case("quint_P64", D=2, kind="spline", deg=5, P=64, **kw2)]
    out += [_case("cubic_P30", n=n, suffix=f"_n{n}", **kw2) for n in (128, 129, 257)]
    out += [_case("lin_P33", D=1, n=4128, suffix="_n4128", K=2, M=1), _case("lin_P6", D=1, n=8200, suffix="_n8200", K=2, M=1)]
    out += [_case("cubic_P30", suffix="_M1", K=2, M=1), _case("cubic_P30", suffix="_M5", K=2, M=5), _case("cubic_P30", suffix="_K7", K=7, M=2),
            _case("cubic_P30", suffix="_noadj", cov_adj=False, **kw2)]
    out += [_case("mv_P7", **kw2), _case("mv_P40", D=3, kind="mv", P=40, **kw2)]
    out += [_case("cubic_P30", regime="stiff", **kw2), _case("mv_P7", regime="stiff", **kw2), _case("cubic_P30", special="empty", **kw2),
            _case("cubic_P30", suffix="_4chains", nch=4, **kw2)]
    return out


CASES = _cases()
# Shapes bfmmm_set_covariates refuses through cov_block_fits' host-side message (k_cov_group's LDS: 91 648 bytes static at 32
# lanes, + (NPG LG + D P^2 + 4) doubles there, against 160 KiB): P 30 at D = 7 needs 168 960 bytes, at D = 8 more; P 47 with BW 5 at
# D = 8 stages 36 x 282 doubles of pair blocks.  The device test asserts the message for these and for no other case.
REFUSED = ("cubic_P30_D7-benign", "cubic_P30_D8-benign", "quint_P47_D8-benign")
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), [c.name for c in CASES]
# the cases the emulations are measured on (the CPU test): everything but the two large-n ones, whose longdouble loops take minutes
CPU_CASES = [c for c in CASES if c.n <= 300 and c.nch == 1]


def expected_route(c, mask, exact=True, pcz=False):
    """what "cov_route" must report after a run of `mask` on case c"""
    do_eta = bool(mask & U_ETA)
    do_xi = bool(mask & U_XI) and c.cov_adj and not pcz
    ng = c.A2 // c.D
    return dict(BW=c.BW, LPC=c.LPC, DX=c.D if (exact and c.BW == 3) else 0, W2D=c.D, PP=c.PP, NB2=c.NB2, NBS=c.NBS, NPG=c.NPG,
                launches=1 + (c.K if do_eta else 0) + (ng - c.K if do_xi else 0), do_eta=do_eta, do_xi=do_xi)


def case_state(c, q=0):
    """curve_update_ref.case_state (eta, xi included) and the hyper parameters of the covariate blocks"""
    st = R.case_state(c, q)
    rng = np.random.default_rng(zlib.crc32(("cov" + c.name).encode()) + 53 * q)
    K, M, P, D = c.K, c.M, c.P, c.D
    if c.regime == "benign":
        st.update(tau_eta=rng.gamma(3.0, 0.5, size=(K, D)), delta_xi=rng.gamma(2.0, 1.0, size=(K, M, D)),
                  gamma_xi=rng.gamma(2.0, 0.7, size=(P, D, M, K)))
    else:       # tau_eta to 1e4, gamma_xi over six decades, sigma^2 = 1e-5 (factor_ref's stiff state)
        lu = lambda lo, hi, size: np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))
        st.update(tau_eta=lu(1e2, 1e4, (K, D)), delta_xi=lu(20.0, 45.0, (K, M, D)) if M == 2 else lu(2.0, 5.0, (K, M, D)),
                  gamma_xi=lu(1e-3, 1e3, (P, D, M, K)))
    st["A_xi"] = rng.gamma(2.0, 1.0, size=(K, 2, D)) + 0.5
    return st


def dir2_of(c, a2):
    """(j, mt, d) of direction a2 (kernels_cov.hip: dir2_of)"""
    KD = c.K * c.D
    if a2 < KD:
        return a2 % c.K, 0, a2 // c.K
    q = a2 - KD
    return q // (c.D * c.M), (q // c.D) % c.M + 1, q % c.D


def updated(c, a2, mask, pcz=False):
    return bool(mask & U_ETA) if dir2_of(c, a2)[1] == 0 else (bool(mask & U_XI) and c.cov_adj and not pcz)


def visited(c, mask, pcz=False):
    return [a for a in range(c.A2) if updated(c, a, mask, pcz)]


def theta_of(c, st):
    """(A2, P) rows of the state's eta (P, D, K) and xi (P, D, M, K) in direction order, float64"""
    out = np.zeros((c.A2, c.P))
    for a in range(c.A2):
        j, mt, d = dir2_of(c, a)
        out[a] = st["eta"][:, d, j] if mt == 0 else st["xi"][:, d, mt - 1, j]
    return out


def thetaX_rows(c, thetaX):
    """the device's "thetaX" (row (j (M + 1) + mt) D + d) in direction order"""
    t = np.asarray(thetaX, dtype=np.float64).reshape(-1, c.P)
    return np.stack([t[(dir2_of(c, a)[0] * (c.M + 1) + dir2_of(c, a)[1]) * c.D + dir2_of(c, a)[2]] for a in range(c.A2)])


def wdir64(c, st, X, order=None):
    """Wdir (n, A2) in float64 in the kernel's order of products"""
    W = np.zeros((c.n, c.A2))
    for a in range(c.A2):
        j, mt, d = dir2_of(c, a)
        if order == "j_outer" and mt == 0:
            j, d = a // c.D, a % c.D
        w = st["Z"][:, j] * X[:, d]
        W[:, a] = w if mt == 0 else w * st["chi"][:, mt - 1]
    return W


def normals(c, q=0, it=0, tt=0):
    """z_a (A2, P) of the oracle's keyed generator with k_cov_factor's index formulas"""
    import oracle_lib as O
    ze = O.fill(1, c.K * c.D * c.P, seed=SEED, chain=q, it=it, upd=UPD_ETA, tt=tt).reshape(-1, c.P)
    zx = O.fill(1, c.K * c.M * c.D * c.P, seed=SEED, chain=q, it=it, upd=UPD_XI, tt=tt).reshape(-1, c.P)
    out = np.zeros((c.A2, c.P))
    for a in range(c.A2):
        j, mt, d = dir2_of(c, a)
        out[a] = ze[d * c.K + j] if mt == 0 else zx[(j * c.M + mt - 1) * c.D + d]
    return out


def pair_row(c, a, b):
    """row of H2aa of the in-group pair of directions a <= b (same group)"""
    g, u, v = a // c.D, a % c.D, b % c.D
    assert b // c.D == g and u <= v
    return g * c.NPG + v * (v + 1) // 2 + u


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


_ratio = R._ratio


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
def check_wdir(c, st, X, Wdir):
    got = np.asarray(Wdir, dtype=np.float64).reshape(c.n, c.A2)
    bad = np.argwhere(got != wdir64(c, st, X))
    return [f"{c.name}: k_cov_prep: Wdir of curve {i}, direction {a} (j, mt, d) {dir2_of(c, a)}: {got[i, a]!r} is not the float64 product"
            for i, a in bad[:4]]


def check_h2aa(c, rec, Wdir, H2aa, mask, pcz=False):
    """every band element of every in-group pair of every updated group (module docstring): dict(worst, fails)"""
    Gb, _, _ = R.split_rec(c, rec)
    G = _ld(Gb).reshape(c.n, c.LG)
    W = _ld(Wdir).reshape(c.n, c.A2)
    H = _ld(H2aa).reshape(-1, c.LG)
    cH = 2 + W2_CH + 1 + c.NB2
    worst, fails = 0.0, []
    for g in range(c.A2 // c.D):
        if not updated(c, g * c.D, mask, pcz):
            continue
        for v in range(c.D):
            for u in range(v + 1):
                ww = W[:, g * c.D + u] * W[:, g * c.D + v]
                ref, Sabs = ww @ G, np.abs(ww) @ np.abs(G)
                row = g * c.NPG + v * (v + 1) // 2 + u
                err, bound = np.abs(H[row] - ref), G_H * cH * U * Sabs
                rat = np.array([_ratio(err[e], bound[e]) for e in range(c.LG)])
                e = int(np.argmax(rat))
                worst = max(worst, rat[e])
                if not rat[e] <= 1.0:
                    fails.append(f"{c.name}: k_cov_w2 / k_cov_factor: H2aa of group {g}, pair (u {u}, v {v}) (directions {dir2_of(c, g * c.D + u)}, "
                                 f"{dir2_of(c, g * c.D + v)}), entry {e} (band row {e // c.P}, p {e % c.P}): {float(H[row, e])!r}, reference "
                                 f"{float(ref[e])!r}, error / bound {rat[e]:.3g}")
    return dict(worst=worst, fails=fails)


def prior_ld(c, st, a, dtype=LD, mut=None):
    """Prior_a (P x P) of direction a in `dtype` (module docstring)"""
    j, mt, d = dir2_of(c, a)
    T = dtype
    if mt == 0:
        te = T(st["tau_eta"][j, d])
        if c.kind == "mv":
            return np.diag(np.full(c.P, te if mut == "mv_prior_not_inverted" else T(1.0) / te))
        return te * F.case_data(c)["Pmat"].astype(T)
    tt = T(1.0)
    for m2 in range(mt - 1 if mut == "tilde_tau_short" else mt):
        tt = tt * T(st["delta_xi"][j, m2, d])
    return np.diag(tt * st["gamma_xi"][:, d, mt - 1, j].astype(T))


def band_dense(hb, P, dtype):
    hb = np.asarray(hb, dtype=np.float64).reshape(-1, P).astype(dtype)
    A = np.zeros((P, P), dtype=dtype)
    for t in range(min(hb.shape[0] - 1, P - 1) + 1):
        A[np.arange(P - t), np.arange(t, P)] = hb[t, :P - t]
        A[np.arange(t, P), np.arange(P - t)] = hb[t, :P - t]
    return A


def is_pinv(c, a):
    """eta directions of the cluster without members: Prec = tau_eta P_mat, rank P - 1 (functional model)"""
    j, mt, _ = dir2_of(c, a)
    return c.empty is not None and j == c.empty and mt == 0 and c.kind != "mv"


def check_factor(c, st, H2aa, C2, Lz2, f, mask, q=0, it=0, pcz=False, tt=0):
    """C_a and L_a z_a of every updated direction (module docstring): dict(worst_C, worst_L, kappa, rho, routes, fails)"""
    H = np.asarray(H2aa, dtype=np.float64).reshape(-1, c.LG)
    Cm, Lz = np.asarray(C2, dtype=np.float64).reshape(c.A2, c.P, c.P), np.asarray(Lz2, dtype=np.float64).reshape(c.A2, c.P)
    z = normals(c, q, it, tt)
    out = dict(worst_C=0.0, worst_L=0.0, kappa=0.0, rho=np.inf, routes=set(), fails=[])
    for a in visited(c, mask, pcz):
        Prec = LD(f) * band_dense(H[pair_row(c, a, a)], c.P, LD) + prior_ld(c, st, a)
        head = f"{c.name}: k_cov_factor<{c.PP}>: direction {a} (j, mt, d) {dir2_of(c, a)}"
        if not (np.isfinite(Cm[a]).all() and np.isfinite(Lz[a]).all()):
            out["fails"].append(head + ": not finite")
            continue
        if c.diag:      # the diagonal model (multivariate: G_i = I and a diagonal prior): factor_ref's entrywise check
            eC, eL, off = F.check_diag(Cm[a].T, Lz[a], Prec, z[a])
            rC, rL, route, pq = eC / F.DIAG_TOL, eL / (F.DIAG_TOL + 36 * U), "diag", "-"
            if not off:
                out["fails"].append(head + ": an off-diagonal entry of C is not zero")
        elif is_pinv(c, a):
            Rf = F.pinv_ld(Prec)
            eC, pq = F.err_C(Cm[a].T, Rf.C, Rf.D)
            bC = F.bound(c.P, Rf.kappa_p, F.G_J)
            comp = float(np.abs(Rf.null.T @ Lz[a].astype(LD)).max()) if Rf.n_null else 0.0
            bN = bC * Rf.Lnorm * float(np.linalg.norm(z[a]))
            rC, rL, route = eC / bC, comp / bN, "pinv"
            if Rf.n_null < 1:
                out["fails"].append(head + ": the reference finds no null vector: the case does not reach the pseudo-inverse route")
        else:
            Rf = F.inverse_ld(Prec)
            if not Rf.ok:
                out["fails"].append(head + ": the reference factorisation broke down")
                continue
            eC, pq = F.err_C(Cm[a].T, Rf.C, Rf.D)
            eL, _ = F.err_Lz(Lz[a], Rf.L, z[a], Rf.D)
            bC = F.bound(c.P, Rf.kappa_s, F.G_C)
            bL = F.bound(c.P, Rf.kappa_s, F.G_L) + (32 + 4 * np.sqrt(c.P) / float(np.linalg.norm(z[a]))) * U
            rC, rL, route = eC / bC, eL / bL, "chol"
            out["kappa"], out["rho"] = max(out["kappa"], Rf.kappa_s), min(out["rho"], Rf.rho)
        out["routes"].add((route, "eta" if dir2_of(c, a)[1] == 0 else "xi"))
        out["worst_C"], out["worst_L"] = max(out["worst_C"], rC), max(out["worst_L"], rL)
        if not (rC <= 1.0 and rL <= 1.0):
            out["fails"].append(head + f" ({route}): err_C / bound {rC:.3g} (worst entry {pq}), err_Lz / bound {rL:.3g}")
    return out


def _curve_arrays(c, rec):
    Gb, sv, yy = R.split_rec(c, rec)
    return _ld(Gb), _ld(sv), _ld(yy)


def _band_all(Gb, V, absolute=False):
    """G_i v_i for every curve: Gb (n, BW + 1, P), V (n, P)"""
    if absolute:
        Gb, V = np.abs(Gb), np.abs(V)
    P = V.shape[1]
    out = Gb[:, 0] * V
    for t in range(1, min(Gb.shape[1] - 1, P - 1) + 1):
        g = Gb[:, t, :P - t]
        out[:, :P - t] += g * V[:, t:]
        out[:, t:] += g * V[:, :P - t]
    return out


def restate_c0(c, rec, st, X, pcz=False):
    """c_i^0 and g_i^0 = G_i c_i^0 in longdouble from a state (full sweeps: the chain slots the block started from), with the
    bounds curve_update_ref.check_cfull holds k_curve_chi's cfull / gfull to against exactly these values: (c0, g0, bc, bg).
    The device's inputs differ from the restated ones by at most bc, bg; check_steps and check_final carry that through."""
    M = 0 if pcz else c.M
    Gb, sv, _ = _curve_arrays(c, rec)
    th, tha = R.theta_rows(c, st, X, M)
    Z, chi = _ld(st["Z"]), _ld(st["chi"])[:, :M]
    cn = R.counts(c, M)
    u = np.einsum("ik,ikmp->imp", Z, th[:, :, 1:])
    ua = np.einsum("ik,ikmp->imp", np.abs(Z), tha[:, :, 1:])
    c0 = np.einsum("ik,ikp->ip", Z, th[:, :, 0]) + np.einsum("im,imp->ip", chi, u)
    ca = np.einsum("ik,ikp->ip", np.abs(Z), tha[:, :, 0]) + np.einsum("im,imp->ip", np.abs(chi), ua)
    dle = np.einsum("im,imp->ip", np.abs(chi), ua)
    g0 = _band_all(Gb, c0)
    bc = R.G_CF * (cn["n_c"] + M + 1) * U * ca + U * dle + U * np.abs(c0)
    bg = (R.G_GF * (cn["n_c"] + 2 * c.BW + M + 5) * U * (2 * np.abs(sv) + _band_all(Gb, ca, absolute=True))
          + U * _band_all(Gb, dle, absolute=True) + U * np.abs(g0))
    return c0, g0, bc, bg


def check_steps(c, rec, Wdir, H2aa, C2, Lz2, th_old, th_new, c0, g0, f, mask, pcz=False, e_g=None):
    """every draw against longdouble, each judged alone (module docstring).  th_old, th_new: (A2, P) in direction order.
    Returns dict(worst, where, vacuous, fails)."""
    Gb, sv, _ = _curve_arrays(c, rec)
    W = _ld(Wdir).reshape(c.n, c.A2)
    H = _ld(H2aa).reshape(-1, c.BW + 1, c.P)
    Cm, Lz = _ld(C2).reshape(c.A2, c.P, c.P), _ld(Lz2).reshape(c.A2, c.P)
    t0, t1 = _ld(th_old), _ld(th_new)
    g0l = np.asarray(g0, dtype=LD).reshape(c.n, c.P)
    Eg = 0 if e_g is None else np.asarray(e_g, dtype=LD).reshape(c.n, c.P)      # what the device's g^0 may differ by (restate_c0)
    dc, dca = np.zeros((c.n, c.P), dtype=LD), np.zeros((c.n, c.P), dtype=LD)
    fl = LD(f)
    out = dict(worst=0.0, where=None, vacuous=0.0, fails=[])
    vis = visited(c, mask, pcz)
    groups = sorted({a // c.D for a in vis})
    for a in range(c.A2):
        if a not in vis:
            if not np.array_equal(np.asarray(th_new)[a], np.asarray(th_old)[a]):
                out["fails"].append(f"{c.name}: direction {a} (j, mt, d) {dir2_of(c, a)} is outside the mask and changed")
            continue
        k = groups.index(a // c.D)
        Haa = H[pair_row(c, a, a)]
        res = sv - g0l - _band_all(Gb, dc)
        Sres = np.abs(sv) + np.abs(g0l) + _band_all(Gb, dca, absolute=True)
        r = W[:, a] @ res
        Sq = np.abs(W[:, a]) @ Sres + S.band_mv(Haa, t0[a], absolute=True)
        rhs = fl * (r + S.band_mv(Haa, t0[a]))
        Cst = Cm[a].T                                   # stored column-major: C[p, q] = Cg[p + P q]
        Cbar = (Cst + Cst.T) / 2
        ref = Cbar @ rhs + Lz[a]
        cr = (k + 1) * (2 * c.BW + 2 + c.D) + GT // c.LPC + c.NBS + 48
        Ein = np.abs(W[:, a]) @ Eg if e_g is not None else np.zeros(c.P, dtype=LD)
        bound = G_STEP * (np.abs(Cbar) @ (fl * cr * U * Sq + (c.P + 3) * U * np.abs(rhs)) + np.abs(Cbar) @ (fl * Ein) + np.abs(Cst - Cst.T) @ np.abs(rhs)
                          + 2 * U * (np.abs(Lz[a]) + np.abs(ref)))
        err = np.abs(t1[a] - ref)
        for p in range(c.P):
            rat = _ratio(err[p], bound[p])
            if rat > out["worst"]:
                out["worst"], out["where"] = rat, (a, p)
            if not rat <= 1.0:
                out["fails"].append(f"{c.name}: k_cov_group<{c.BW},{c.LPC}>: direction {a} (j, mt, d) {dir2_of(c, a)} (group {a // c.D}, {k} groups applied), "
                                    f"entry p {p}: theta {float(t1[a, p])!r}, reference {float(ref[p])!r}, error {float(err[p]):.3g}, bound {float(bound[p]):.3g}, "
                                    f"error / bound {rat:.3g}")
        dmax = float(np.abs(ref - t0[a]).max())
        out["vacuous"] = max(out["vacuous"], _ratio(float(bound.max()), dmax))
        dl = t1[a] - t0[a]
        dc += np.outer(W[:, a], dl)
        dca += np.outer(np.abs(W[:, a]), np.abs(dl))
    out["dc"], out["dca"], out["n_groups"] = dc, dca, len(groups)
    return out


def check_final(c, rec, steps, c0, g0, cfull, gfull, e_c=None, e_g=None):
    """the final cfull / gfull entry by entry (module docstring); steps: check_steps' result.  dict(worst, worst_g, fails)"""
    Gb, _, _ = _curve_arrays(c, rec)
    c0l, g0l, cf, gf = (np.asarray(x, dtype=LD).reshape(c.n, c.P) for x in (c0, g0, cfull, gfull))
    out = dict(worst=0.0, worst_g=0.0, fails=[])
    ng = steps["n_groups"]
    if ng == 0 and e_c is None:
        if not (np.array_equal(cf, c0l) and np.array_equal(gf, g0l)):
            out["fails"].append(f"{c.name}: cfull / gfull changed in a run without an eta / Xi step")
        return out
    cref = c0l + steps["dc"]
    gref = g0l + _band_all(Gb, steps["dc"])
    bc = G_CF * (c.D + 1 + ng) * U * (np.abs(c0l) + steps["dca"]) + U * np.abs(cref)
    bg = G_GF * (2 * c.BW + 2 + c.D + ng) * U * (np.abs(g0l) + _band_all(Gb, steps["dca"], absolute=True)) + U * np.abs(gref)
    if e_c is not None:      # restated inputs: the device's own c^0, g^0 are within e_c, e_g of them
        bc, bg = bc + np.asarray(e_c, dtype=LD), bg + np.asarray(e_g, dtype=LD)
    for nm, key, got, ref, b in (("cfull", "worst", cf, cref, bc), ("gfull", "worst_g", gf, gref, bg)):
        for i in range(c.n):
            for p in range(c.P):
                rat = _ratio(abs(got[i, p] - ref[i, p]), b[i, p])
                out[key] = max(out[key], rat)
                if not rat <= 1.0 and len(out["fails"]) < 12:
                    out["fails"].append(f"{c.name}: k_cov_group: {nm} of curve {i} (workgroup {i // c.CPB}), entry p {p}: {float(got[i, p])!r}, reference "
                                        f"{float(ref[i, p])!r}, error / bound {rat:.3g}")
    return out


def check_rss(c, rec, cfull, gfull, rss_part):
    """rss_part of the closing launch from the device's final cfull / gfull (module docstring): dict(worst, fails)"""
    _, sv, yy = _curve_arrays(c, rec)
    cf, gf = _ld(cfull).reshape(c.n, c.P), _ld(gfull).reshape(c.n, c.P)
    got = _ld(rss_part).reshape(-1)
    out = dict(worst=0.0, fails=[])
    if got.shape[0] != c.nblk:
        out["fails"].append(f"{c.name}: {got.shape[0]} entries of rss_part for {c.nblk} curve workgroups")
        return out
    val = yy - 2 * (cf * sv).sum(axis=1) + (cf * gf).sum(axis=1)
    Sab = np.abs(yy) + 2 * (np.abs(cf) * np.abs(sv)).sum(axis=1) + (np.abs(cf) * np.abs(gf)).sum(axis=1)
    cR = c.LPC + GT // c.LPC + 8
    for b in range(c.nblk):
        if b >= c.NBS:
            if got[b] != 0:
                out["fails"].append(f"{c.name}: rss_part[{b}] beyond the {c.NBS} workgroups of k_cov_group is {float(got[b])!r}, not 0")
            continue
        sl = slice(b * c.CPB, min(c.n, (b + 1) * c.CPB))
        ref, bound = val[sl].sum(), G_RSS2 * cR * U * Sab[sl].sum()
        rat = _ratio(abs(got[b] - ref), bound)
        out["worst"] = max(out["worst"], rat)
        if not rat <= 1.0:
            out["fails"].append(f"{c.name}: k_cov_group (closing launch): rss_part of workgroup {b} (curves {sl.start} .. {sl.stop - 1}): {float(got[b])!r}, "
                                f"reference {float(ref)!r}, error / bound {rat:.3g}")
    return out


def gstd2_shapes(c, st_old, hyp):
    """the shape of every standard gamma variate of "gstd2" (k_cov_prep; the reference's integer divisions) and its update id"""
    K, M, P, D = c.K, c.M, c.P, c.D
    sh = [(17, e, hyp["alpha_eta"] + P // 2) for e in range(K * D)]
    for idx in range(K * M * D):      # (d K + k) M + i
        i, k, dd = idx % M, (idx // M) % K, idx // (M * K)
        sh.append((19, idx, st_old["A_xi"][k, 0, dd] + (P * M) * 0.5 if i == 0 else st_old["A_xi"][k, 1, dd] + (P * (M - i)) * 0.5))
    sh += [(22, e, (hyp["nu_1"] + 1) / 2) for e in range(K * D * P * M)]
    return sh


def check_gstd2(c, st_old, gstd2, before, hyp, mask, q=0, it=0, pcz=False, tt=0):
    """ "gstd2" against the oracle's keyed standard gamma variates.  Both are Marsaglia-Tsang draws d (1 + c z)^3 of the same
    uniforms, d = shape - 1/3, c = 1 / sqrt(9 d): the AS241 allowance of the normal, (32 |z| + 4) u, passes through the cube as
    3 c (32 |z| + 4) u / (1 + c z) relative, with z and 1 + c z recovered from the oracle's variate; + 8 u for the products.  Parts
    whose mask bit is off (or, the Xi parts, without the Xi block) must equal `before`, the array before the run.  List of failures."""
    import oracle_lib as O
    K, M, P, D = c.K, c.M, c.P, c.D
    got, before = np.ascontiguousarray(gstd2, dtype=np.float64), np.ascontiguousarray(before, dtype=np.float64)
    xi_on = c.cov_adj and not pcz
    on = {17: bool(mask & U_TAU_ETA), 19: bool(mask & U_DELTA_XI) and xi_on, 22: bool(mask & U_GAMMA_XI) and xi_on}
    sh = gstd2_shapes(c, st_old, hyp)
    ref = np.zeros(len(sh))
    n_tau, n_del = K * D, K * M * D
    if on[17]:
        ref[:n_tau] = O.fill(2, n_tau, seed=SEED, chain=q, it=it, upd=17, p1=sh[0][2], p2=1.0, tt=tt)
    if on[19]:
        for e in range(n_tau, n_tau + n_del):
            ref[e] = O.fill(2, sh[e][1] + 1, seed=SEED, chain=q, it=it, upd=19, p1=sh[e][2], p2=1.0, tt=tt)[-1]
    if on[22]:
        ref[n_tau + n_del:] = O.fill(2, len(sh) - n_tau - n_del, seed=SEED, chain=q, it=it, upd=22, p1=sh[-1][2], p2=1.0, tt=tt)
    fails = []
    for e, (upd, idx, shape) in enumerate(sh):
        if not on[upd]:
            if got[e:e + 1].view(np.int64)[0] != before[e:e + 1].view(np.int64)[0] and len(fails) < 6:
                fails.append(f"{c.name}: k_cov_prep: gstd2[{e}] (update id {upd}) changed although its mask bit is off")
            continue
        d = shape - 1.0 / 3.0
        cc = 1.0 / np.sqrt(9.0 * d)
        t = (ref[e] / d) ** (1.0 / 3.0)
        tol = (3 * cc * (32 * abs((t - 1) / cc) + 4) / t + 8) * U * ref[e]
        if not abs(got[e] - ref[e]) <= tol and len(fails) < 6:
            fails.append(f"{c.name}: k_cov_prep: gstd2[{e}] (update id {upd}, index {idx}, shape {shape!r}): {got[e]!r}, the oracle's keyed variate "
                         f"{ref[e]!r}, error / tolerance {abs(got[e] - ref[e]) / tol:.3g}")
    return fails


def axi_reference(c, st_old, dx_cur, hyp, q=0, it=0, tt=0):
    """the A_xi step (UpdateA.h:137-205) of every cell (j, i, d) from the oracle's keyed proposal (UPD_AXI_PROP, rtruncnorm at 0) and
    uniform (UPD_AXI_ACC), index (j 2 + i) D + d: list of dict(cell, cur, na, sd, logu, acc(na) -> (value, sum of absolute terms))"""
    import oracle_lib as O
    K, M, D = c.K, c.M, c.D
    L = O.lib()
    out = []
    uu = O.fill(0, K * 2 * D, seed=SEED, chain=q, it=it, upd=21, tt=tt)
    for j in range(K):
        for i in range(2):
            for d in range(D):
                idx = (j * 2 + i) * D + d
                sd = hyp["var_epsilon1"] / hyp["beta1l"] if i == 0 else hyp["var_epsilon2"] / hyp["beta2l"]
                cur = float(st_old["A_xi"][j, i, d])
                na = float(O.fill(3, idx + 1, seed=SEED, chain=q, it=it, upd=20, p1=cur, p2=sd, tt=tt)[-1])
                lg = np.log(_ld(dx_cur)[j, :, d])

                def acc(na, cur=cur, sd=sd, i=i, lg=lg):
                    na, cu, s = LD(na), LD(cur), LD(sd)
                    al, be = (hyp["alpha1l"], hyp["beta1l"]) if i == 0 else (hyp["alpha2l"], hyp["beta2l"])
                    kk = 1 if i == 0 else M - 1
                    sl = lg[0] if i == 0 else lg[1:].sum()
                    terms = []
                    for x, sign in ((na, 1), (cu, -1)):
                        terms += [-sign * kk * R.lgamma_ld(x), sign * (x - 1) * sl, sign * (LD(al) - 1) * np.log(x), -sign * x * LD(be)]
                    # the proposal densities: the Gaussian parts cancel ((cur - na)^2 both ways), the normalisations do not
                    terms += [-np.log(LD(L.orc_pnorm(float(na / s)))), np.log(LD(L.orc_pnorm(float(cu / s))))]
                    return sum(terms, LD(0)), sum((abs(t) for t in terms), LD(0)) + ((cu - na) / s) ** 2

                out.append(dict(cell=(j, i, d), cur=cur, na=na, sd=sd, logu=np.log(LD(uu[idx])), acc=acc))
    return out


def check_axi(c, st_old, A_new, dx_cur, hyp, mask, q=0, it=0, pcz=False, tt=0):
    """every cell of A_xi: bit-equal to its old value or (within the AS241 allowance sd (32 |x| + 4) u + 2 u |na|) the oracle's keyed
    proposal, and the decision agrees with the longdouble acceptance value wherever |log u - acc_ref| exceeds its bound
    16 u (sum of absolute terms + 1) + |acc(na +- tolerance) - acc(na)|: the device's log(tgamma), log, erfc and the proposal's own
    allowance.  No cell may be left undecided.  dx_cur: delta_xi as k_cov_hyper holds it at that point (the new one).  Failures."""
    A_new = np.asarray(A_new, dtype=np.float64)
    if not ((mask & U_A_XI) and c.cov_adj and not pcz):
        return [] if np.array_equal(A_new, np.asarray(st_old["A_xi"], dtype=np.float64)) else [f"{c.name}: k_cov_hyper: A_xi changed although its step is off"]
    fails = []
    for r in axi_reference(c, st_old, dx_cur, hyp, q, it, tt):
        j, i, d = r["cell"]
        got, cur, na = float(A_new[j, i, d]), r["cur"], r["na"]
        tol = r["sd"] * (32 * abs((na - cur) / r["sd"]) + 4) * U + 2 * U * abs(na)
        took = got != cur
        if took and not abs(got - na) <= tol:
            fails.append(f"{c.name}: k_cov_hyper: A_xi{r['cell']} {got!r} is neither its old value {cur!r} nor the keyed proposal {na!r}")
            continue
        x = got if took else na
        a0, Sa = r["acc"](x)
        bound = 16 * U * (Sa + 1) + max(abs(r["acc"](x + tol)[0] - a0), abs(r["acc"](x - tol)[0] - a0))
        margin = abs(r["logu"] - a0)
        if not margin > bound:
            fails.append(f"{c.name}: A_xi{r['cell']}: undecided by the reference (|log u - acc| {float(margin):.3g}, bound {float(bound):.3g}): choose another seed")
        elif took != bool(r["logu"] < a0):
            fails.append(f"{c.name}: k_cov_hyper: A_xi{r['cell']} was {'accepted' if took else 'rejected'}; log u {float(r['logu']):.6g}, longdouble acceptance "
                         f"value {float(a0):.6g} (bound {float(bound):.3g})")
    return fails


def _dot(a, b, seq):
    """sum a_p b_p: in index order (seq), or however numpy's dot sums it"""
    if not seq:
        return a @ b
    acc = a.dtype.type(0)
    for x, y in zip(a, b):
        acc = acc + x * y
    return acc


def hyper_ref(c, st_old, th_new, gstd2, hyp, mask, pcz=False, mut=None, dtype=LD, seq=False):
    """tau_eta (K, D), delta_xi (K, M, D), gamma_xi (P, D, M, K) in `dtype` (longdouble: the reference; float64: the emulations,
    sums in index order with seq) from the committed rows th_new (A2, P), the old state and the standard gamma variates:
    dict(name: value) and "tau_amp" (K, D), the sum of absolute terms of tau_eta's denominator over the denominator"""
    K, M, P, D = c.K, c.M, c.P, c.D
    T = dtype

    def cast(x):
        return np.asarray(x, dtype=np.float64).astype(T)

    g, t = cast(gstd2), cast(th_new)
    out = {}

    def row(j, mt, d):
        return t[d * K + j] if mt == 0 else t[K * D + ((j * M) + mt - 1) * D + d]

    if mask & U_TAU_ETA:
        Pm = np.eye(P, dtype=T) if c.kind == "mv" else cast(F.case_data(c)["Pmat"])
        te, amp = np.zeros((K, D), dtype=T), np.zeros((K, D), dtype=T)
        be = T(hyp["beta_eta"])
        for j in range(K):
            for d in range(D):
                e = row(j, 0, d)
                qf = _dot(e, np.array([_dot(Pm[p], e, seq) for p in range(P)], dtype=T), seq)
                if mut == "tau_qf_low_bits" and (j, d) == (0, 0):      # the quadratic form off by 2^-44 of itself
                    qf = qf * (1 + T(2.0) ** -44)
                qa = np.abs(e) @ np.abs(Pm) @ np.abs(e)
                v = g[j * D + d] / (be + qf / 2)
                te[j, d] = 1 / v if c.kind == "mv" else v
                amp[j, d] = (be + qa / 2) / (be + qf / 2)
        out["tau_eta"], out["tau_amp"] = te, amp
    xi_on = c.cov_adj and not pcz
    dx_old = cast(st_old["delta_xi"])
    dx = dx_old.copy()
    if (mask & U_DELTA_XI) and xi_on:
        gx = cast(st_old["gamma_xi"])
        for d in range(D):
            for j in range(K):
                Sk = np.array([_dot(gx[:, d, m, j], row(j, m + 1, d) ** 2, seq) for m in range(M)], dtype=T)
                cur = dx_old[j, :, d].copy()
                for i in range(M):
                    src = dx_old[j, :, d] if mut == "delta_old" else cur
                    p2 = T(1)
                    for m in range(i, M):
                        tt = T(1)
                        for nn in range(m + 1):
                            if nn != i:
                                tt = tt * (src[nn] if nn < i else cur[nn])
                        p2 = p2 + tt * Sk[m] / 2
                    cur[i] = g[K * D + (d * K + j) * M + i] / p2
                dx[j, :, d] = cur
        out["delta_xi"] = dx
    if (mask & U_GAMMA_XI) and xi_on:
        gm = np.zeros((P, D, M, K), dtype=T)
        n0 = K * D + K * M * D
        for k in range(K):
            for d in range(D):
                for m in range(M):
                    ph = np.prod(dx[k, :m + 1, d])
                    for p in range(P):
                        x = row(k, m + 1, d)[p]
                        gm[p, d, m, k] = g[n0 + ((k * D + d) * P + p) * M + m] * (2 / (T(hyp["nu_1"]) + ph * x * x))
        out["gamma_xi"] = gm
    return out


def check_hyper(c, st_old, st_new, th_new, gstd2, hyp, mask, pcz=False):
    """the device's new tau_eta / delta_xi / gamma_xi (st_new) against hyper_ref, each under its own constant (module docstring):
    dict(worst (over the three), worst_tau, worst_delta, worst_gamma, fails)"""
    ref = hyper_ref(c, st_old, th_new, gstd2, hyp, mask, pcz)
    out = dict(worst=0.0, worst_tau=0.0, worst_delta=0.0, worst_gamma=0.0, fails=[])
    for nm, key in (("tau_eta", "worst_tau"), ("delta_xi", "worst_delta"), ("gamma_xi", "worst_gamma")):
        got = _ld(st_new[nm])
        if nm not in ref:
            if not np.array_equal(np.asarray(st_new[nm], dtype=np.float64), np.asarray(st_old[nm], dtype=np.float64)):
                out["fails"].append(f"{c.name}: k_cov_hyper: {nm} changed although its mask bit is off")
            continue
        val = ref[nm]
        G = {"tau_eta": G_TAU, "delta_xi": G_DELTA, "gamma_xi": G_GAMMA}[nm]
        bound = G * U * np.abs(val) * (ref["tau_amp"] if nm == "tau_eta" else 1)
        rat = np.array([_ratio(e, b) for e, b in zip(np.abs(got - val).ravel(), np.broadcast_to(bound, val.shape).ravel())])
        k = int(np.argmax(rat))
        out[key] = rat[k]
        out["worst"] = max(out["worst"], rat[k])
        if not rat[k] <= 1.0:
            idx = np.unravel_index(k, val.shape)
            out["fails"].append(f"{c.name}: k_cov_hyper: {nm}{tuple(int(x) for x in idx)}: {float(got[idx])!r}, reference {float(val[idx])!r}, error / bound {rat[k]:.3g}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 emulations of the block
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # name: (case, mask, beta, which check must reject it)
    "hsu_dropped": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "steps"),
    "pair_q_confused": ("cubic_P30_D3-benign", COV_MEAN | COV_XI, 1.0, "steps"),
    "lower_band_dropped": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "steps"),
    "g_stale": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "steps"),
    "parity_not_flipped": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "steps"),
    "last_curve_dropped": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "steps"),
    "f_without_beta": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 0.37, "steps"),
    "tilde_tau_short": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "factor"),
    "mv_prior_not_inverted": ("mv_P7_D2-benign", COV_MEAN | COV_XI, 1.0, "factor"),
    "j_outer": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "wdir"),
    "cfull_without_gfull": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "final"),
    "yy_left_out": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "rss"),
    "rss_tail_nonzero": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "rss"),
    "delta_old": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "hyper"),
    "tau_qf_low_bits": ("cubic_P30_D2-benign", COV_MEAN | COV_XI, 1.0, "hyper"),
}


def host_c0(c, rec, st, X):
    """c_i^0 and g_i^0 = G_i c_i^0 in float64 from the state (the CPU tests' stand-in for k_curve_chi's cfull / gfull)"""
    Gb, _, _ = R.split_rec(c, rec)
    th, _ = R.theta_rows(c, st, X, c.M, dtype=np.float64)
    u = np.einsum("ik,ikmp->imp", st["Z"], th[:, :, 1:])
    c0 = np.einsum("ik,ikp->ip", st["Z"], th[:, :, 0]) + np.einsum("im,imp->ip", st["chi"], u)
    return c0, _band_all(Gb, c0)


def _seq_sum(rows):
    acc = np.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def emulate(c, rec, st, X, c0, g0, mask, beta, z, gstd2, hyp, variant="kernel", mut=None, pcz=False):
    """the block in float64: dict(Wdir, H2aa, C2, Lz2, th_new (A2, P), cfull, gfull, rss_part, tau_eta, delta_xi, gamma_xi)"""
    n, P, D, A2, BW, LG = c.n, c.P, c.D, c.A2, c.BW, c.LG
    Gb, sv, yy = R.split_rec(c, rec)
    Gf = Gb.reshape(n, LG)
    W = wdir64(c, st, X, order="j_outer" if mut == "j_outer" else None)
    f = (1.0 if mut == "f_without_beta" else beta) / float(np.ravel(st["sigma_sq"])[0])
    vis = visited(c, mask, pcz)
    H = np.zeros((A2 // D * c.NPG, LG))
    for g in sorted({a // D for a in vis}):
        for v in range(D):
            for u in range(v + 1):
                wv, wu = W[:, g * D + v], W[:, g * D + u]
                if variant == "plain":
                    H[g * c.NPG + v * (v + 1) // 2 + u] = (wu * wv) @ Gf
                    continue
                parts = []
                for i0 in range(0, n, W2_CH):
                    nh = 2 if ((LG + 63) // 64) * 64 <= 128 else 1
                    per = W2_CH // nh
                    halves = []
                    for h in range(nh):
                        acc = np.zeros(LG)
                        for i in range(i0 + h * per, min(n, i0 + (h + 1) * per)):
                            acc = acc + wu[i] * (wv[i] * Gf[i])
                        halves.append(acc)
                    parts.append(halves[0] + halves[1] if nh == 2 else halves[0])
                H[g * c.NPG + v * (v + 1) // 2 + u] = _seq_sum(parts)
    Hb = H.reshape(-1, BW + 1, P)
    C2, Lz2 = np.zeros((A2, P, P)), np.zeros((A2, P))
    for a in vis:
        Prec = f * band_dense(Hb[pair_row(c, a, a)], P, np.float64) + prior_ld(c, st, a, np.float64, mut=mut)
        if is_pinv(c, a):
            Cc, lz = F.emulate_pinv(Prec, z[a])
        elif variant == "plain":
            Rf = F.inverse_ld(Prec)
            Cc, lz = np.asarray(Rf.C, dtype=np.float64), np.asarray(Rf.L @ z[a].astype(LD), dtype=np.float64)
        else:
            Cc, lz = F.emulate(Prec, z[a], c.BWP)
        C2[a], Lz2[a] = np.asarray(Cc).T, lz
    t0 = theta_of(c, st)
    t1 = t0.copy()
    cf, gf = np.array(c0, dtype=np.float64).reshape(n, P).copy(), np.array(g0, dtype=np.float64).reshape(n, P).copy()
    CPB = c.CPB
    n_eff = n - 1 if mut == "last_curve_dropped" else n

    def partial_sums(g, gf):    # step_part of group g from the g_i given: (NBS, D, P)
        out = np.zeros((c.NBS, D, P))
        for b in range(c.NBS):
            for s in range(D):
                acc = np.zeros(P)
                for i0 in range(b * CPB, min(n_eff, (b + 1) * CPB), COV_CPG):
                    a2 = np.zeros(P)
                    for i in range(i0, min(n_eff, i0 + COV_CPG)):
                        a2 = a2 + W[i, g * D + s] * (sv[i] - gf[i])
                    acc = acc + a2
                out[b, s] = acc
        return out

    groups = sorted({a // D for a in vis})
    part = [np.zeros((c.NBS, D, P)), np.zeros((c.NBS, D, P))]
    par = 0
    gf_before = gf            # g_i before the previous group was applied
    for gi, g in enumerate(groups):
        if variant == "plain":
            for s in range(D):
                a = g * D + s
                gcur = _band_all(Gb, cf)
                r = W[:, a] @ (sv - gcur)
                rhs = f * (r + S.band_mv(Hb[pair_row(c, a, a)], t0[a]))
                t1[a] = C2[a].T @ rhs + Lz2[a]
                cf = cf + np.outer(W[:, a], t1[a] - t0[a])
            gf = _band_all(Gb, cf)
            continue
        part[par ^ 1] = partial_sums(g, gf_before if mut == "g_stale" else gf)
        par ^= 1
        gf_before = gf
        src = part[par ^ 1] if (mut == "parity_not_flipped" and gi == 1) else part[par]
        segs = [_seq_sum([src[b] for b in range(q, c.NBS, 32)]) for q in range(min(32, c.NBS))]
        sR = _seq_sum(segs)
        dl = np.zeros((D, P))
        for s in range(D):
            a = g * D + s
            tot = np.zeros(P)
            for u in range(s + 1):
                q = s * (s + 1) // 2 + u
                if mut == "pair_q_confused" and s == 2:
                    q = {3: 4, 4: 3}.get(q, q)
                if mut == "hsu_dropped" and gi == 1 and s == 1 and u == 0:
                    continue
                hv = S.band_mv(Hb[g * c.NPG + q], dl[u] if u < s else t0[a], lower=mut != "lower_band_dropped" or u == s)
                tot = tot - hv if u < s else tot + hv
            rhs = f * (sR[s] + tot)
            t1[a] = C2[a].T @ rhs + Lz2[a]
            dl[s] = t1[a] - t0[a]
        v = W[:, g * D:(g + 1) * D] @ dl
        cf = cf + v
        if mut != "cfull_without_gfull":
            gf = gf + _band_all(Gb, v)
    if variant == "plain":
        val = yy - 2 * np.einsum("ip,ip->i", cf, sv) + np.einsum("ip,ip->i", cf, gf)
    else:
        val = np.array([(0.0 if mut == "yy_left_out" else yy[i]) - 2.0 * float(np.sum(cf[i] * sv[i])) + float(np.sum(cf[i] * gf[i])) for i in range(n)])
    rss = np.zeros(c.nblk)
    for b in range(c.NBS):
        rss[b] = _seq_sum(list(val[b * CPB:min(n, (b + 1) * CPB)]))
    if mut == "rss_tail_nonzero" and c.nblk > c.NBS:
        rss[c.NBS] = 1e-300
    out = dict(Wdir=W, H2aa=H, C2=C2, Lz2=Lz2, th_new=t1, cfull=cf, gfull=gf, rss_part=rss, f=f)
    hr = hyper_ref(c, st, t1, gstd2, hyp, mask, pcz, mut=mut, dtype=np.float64, seq=variant == "kernel")
    for nm in ("tau_eta", "delta_xi", "gamma_xi"):
        out[nm] = np.asarray(hr[nm], dtype=np.float64) if nm in hr else np.asarray(st[nm], dtype=np.float64)
    return out


def check_all(c, rec, st, X, c0, g0, mask, beta, dev, hyp, q=0, it=0, pcz=False, gstd2=None, e_c=None, e_g=None, tt=0):
    """every check on one run's arrays `dev` (the keys of emulate's result; sigma2: the block's): dict(check: result)"""
    f = beta / float(dev["sigma2"])
    res = dict(wdir=dict(worst=0.0, fails=check_wdir(c, st, X, dev["Wdir"]) if visited(c, mask, pcz) else []))
    res["h2aa"] = check_h2aa(c, rec, dev["Wdir"], dev["H2aa"], mask, pcz)
    res["factor"] = check_factor(c, st, dev["H2aa"], dev["C2"], dev["Lz2"], f, mask, q, it, pcz, tt)
    res["steps"] = check_steps(c, rec, dev["Wdir"], dev["H2aa"], dev["C2"], dev["Lz2"], theta_of(c, st), dev["th_new"], c0, g0, f, mask, pcz,
                               e_g=e_g)
    res["final"] = check_final(c, rec, res["steps"], c0, g0, dev["cfull"], dev["gfull"], e_c, e_g)
    res["rss"] = check_rss(c, rec, dev["cfull"], dev["gfull"], dev["rss_part"])
    if gstd2 is not None:
        res["hyper"] = check_hyper(c, st, dev, dev["th_new"], gstd2, hyp, mask, pcz)
    return res
