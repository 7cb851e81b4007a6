"""The post-processing primitives (include/bfmmm_post.h: bfmmm_post_pointwise, bfmmm_post_pointwise_joint, bfmmm_post_curve_loglik,
bfmmm_post_cpo, bfmmm_post_sample_paths) entry by entry against the long-double restatement of tests/post_ref.py, under its bounds (derived
and measured there on the CPU, never from device output), on the case list that visits every class of the kernels' launch geometry."""
import ctypes as C
import functools

import numpy as np
import pytest

import post_ref as J

pytestmark = pytest.mark.gpu
U, LD = J.U, J.LD
SEEDS = (5, 6)


def _input(c, d, identity=None):
    from bayesfmmm_amd import api
    inp, keep = api._post_input(d["Y"], d["B"], d["nu"], d["Phi"], d["Z"], d["chi"], d["sigma"], d["X"], d["eta"], d["xi"])
    if c.basis == "identity" if identity is None else identity:      # the multivariate entry points' form: no B, observation j's row is e_j
        inp.B, inp.identity_basis = None, 1
    return inp, keep


def _dp(a):
    from bayesfmmm_amd import api
    return a.ctypes.data_as(api.c_double_p)


def _split(c, v):
    off = np.concatenate([[0], np.cumsum(c.lens)])
    return [v[off[i]:off[i + 1]] for i in range(c.n)]


def dev_pointwise(c, d):
    from bayesfmmm_amd import api
    lib = api._lib_entry()
    inp, keep = _input(c, d)
    n_obs = int(np.sum(c.lens))
    ll, pdf, fit, ll2, joint, fit2 = np.zeros(c.T), np.zeros(n_obs), np.zeros(n_obs), np.zeros(c.T), np.zeros(c.n), np.zeros(n_obs)
    api._check(lib.bfmmm_post_pointwise(C.byref(inp), c.first_kept, _dp(ll), _dp(pdf), _dp(fit)))
    api._check(lib.bfmmm_post_pointwise_joint(C.byref(inp), c.first_kept, _dp(ll2), _dp(joint), _dp(fit2)))
    return dict(llik=ll, pdf=pdf, fit=fit, llik2=ll2, joint=joint, fit2=fit2)


def dev_cpo(c, d):
    from bayesfmmm_amd import api
    lib = api._lib_entry()
    inp, keep = _input(c, d)
    mat, cpo = np.zeros((c.n, c.T - c.first_kept)), np.zeros(c.n)
    api._check(lib.bfmmm_post_curve_loglik(C.byref(inp), c.first_kept, _dp(mat)))
    api._check(lib.bfmmm_post_cpo(C.byref(inp), c.first_kept, _dp(cpo)))
    return dict(mat=mat, cpo=cpo)


def dev_paths(c, d, seed):
    from bayesfmmm_amd import api
    lib = api._lib_entry()
    inp, keep = _input(c, d, identity=False)
    kept, n_obs = c.T - c.first_kept, int(np.sum(c.lens))
    paths, mo = np.zeros(kept * n_obs), np.zeros(kept * n_obs)
    api._check(lib.bfmmm_post_sample_paths(C.byref(inp), c.first_kept, seed, _dp(paths), _dp(mo)))
    # curve i: a kept x n_i block, draw fastest, at kept * offsets[i]  ->  (kept, n_obs)
    return dict(paths=paths.reshape(n_obs, kept).T.copy(), mo=mo.reshape(n_obs, kept).T.copy())


def _before_first_kept(c, d, value, variance):
    """the case's data with nu, Phi and chi of the draws before first_kept set to `value` and their variance to `variance`"""
    d2 = dict(d)
    for nm, val in (("nu", value), ("Phi", value), ("chi", value), ("sigma", variance)):
        a = d[nm].copy()
        a[..., :c.first_kept] = val
        d2[nm] = a
    return d2


def _same_bytes(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in a)


def _note(res, kernel, labels, quantity, r, where):
    """r = error / (bound with its constant): recorded under every geometry class it was judged in; a failure when above 1"""
    for lb in labels:
        key = (kernel, lb)
        res["worst"][key] = max(res["worst"].get(key, 0.0), r)
    if not r <= 1.0:
        res["fails"].append(f"{where}: {quantity} error / bound = {r:.3g}")


@functools.lru_cache(maxsize=None)
def judged_pointwise(name):
    c = J.CASE[name]
    d, ref, g = J.case_data(c), J.ld_pointwise(c), J.case_geometry(c)
    got = dev_pointwise(c, d)
    res = dict(worst={}, fails=[])
    call = sorted(J.classes(c)["pw"])
    r = J.ratio(got["llik"], ref["llik"], ref["b_llik"]) / J.G_LLIK
    print(f"{name}: llik error / bound {r:.3g}")
    _note(res, "k_post_pointwise", call, "llik", r, name)
    pdf, fit = _split(c, got["pdf"]), _split(c, got["fit"])
    for i, q in enumerate(g["pw"]):
        lbs = [f"JW={q['JW']}", f"G={q['G']}", "staged" if q["staged"] else "unstaged", "NCH=1" if g["NCH"] == 1 else "NCH>1"]
        rs = dict(mean_pdf=J.ratio(pdf[i], ref["mean_pdf"][i], ref["b_pdf"][i]) / J.G_PDF,
                  mean_fit=J.ratio(fit[i], ref["mean_fit"][i], ref["b_fit"][i]) / J.G_FIT,
                  joint=J.ratio(got["joint"][i], ref["joint"][i], ref["b_joint"][i]) / J.G_JOINT)
        print(f"{name}: curve {i} (n_i = {q['ni']}): error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in rs.items()))
        for k, v in rs.items():
            _note(res, "k_post_pointwise", lbs, k, v, f"{name} curve {i}")
    if not (np.array_equal(got["llik"].view(np.uint64), got["llik2"].view(np.uint64)) and np.array_equal(got["fit"].view(np.uint64), got["fit2"].view(np.uint64))):
        res["fails"].append(f"{name}: bfmmm_post_pointwise and bfmmm_post_pointwise_joint differ in llik or mean_fit")
    if not _same_bytes(got, dev_pointwise(c, d)):
        res["fails"].append(f"{name}: two calls of the pointwise primitives differ")
    if c.first_kept > 0:      # the draws before first_kept count in llik alone
        other = dev_pointwise(c, _before_first_kept(c, d, 0.5, 2.0))
        if not all(np.array_equal(got[k].view(np.uint64), other[k].view(np.uint64)) for k in ("pdf", "fit", "fit2", "joint")):
            res["fails"].append(f"{name}: the draws before first_kept leak into the per-observation means or the joint density")
        if not np.array_equal(got["llik"][c.first_kept:].view(np.uint64), other["llik"][c.first_kept:].view(np.uint64)) or np.array_equal(got["llik"], other["llik"]):
            res["fails"].append(f"{name}: llik of the kept draws depends on the draws before, or llik of those draws does not see them")
    return res


@functools.lru_cache(maxsize=None)
def judged_cpo(name):
    c = J.CASE[name]
    d, ref, g = J.case_data(c), J.ld_cpo(c), J.case_geometry(c)["cpo"]
    fk = c.first_kept
    got = dev_cpo(c, d)
    res = dict(worst={}, fails=[])
    own, _, b_own = J.ld_harmonic(got["mat"])
    for i, ni in enumerate(c.lens):
        lbs = [f"home={g['home']}", f"Gc={g['gc_class']}", "staged" if g["staged"][i] else "unstaged"] + (["NIP<NIPX"] if g["NIP"][i] < g["NIPX"] else [])
        r = J.ratio(got["mat"][i], ref["ll"][i, fk:], ref["b_ll"][i, fk:]) / J.G_CPO
        # log CPO: against the harmonic mean of the reference matrix with the matrix's bound carried through, and against the
        # harmonic mean of the device's own matrix to a few ulp
        r2 = J.ratio(got["cpo"][i], ref["cpo"][i], J.G_CPO * ref["b_cpo_carry"][i] + ref["b_cpo_own"][i])
        r3 = J.ratio(got["cpo"][i], own[i], b_own[i])
        print(f"{name}: curve {i} (n_i = {ni}): error / bound matrix {r:.3g}, log CPO {r2:.3g}, log CPO of the device's own matrix {r3:.3g}")
        _note(res, "k_post_cpo", lbs, "ll", r, f"{name} curve {i}")
        _note(res, "k_post_cpo_reduce", lbs, "log CPO", r2, f"{name} curve {i}")
        _note(res, "k_post_cpo_reduce", lbs, "log CPO of the device's own matrix", r3, f"{name} curve {i}")
    if not _same_bytes(got, dev_cpo(c, d)):
        res["fails"].append(f"{name}: two calls of the CPO primitives differ")
    if fk > 0 and not _same_bytes(got, dev_cpo(c, _before_first_kept(c, d, np.nan, -1.0))):
        res["fails"].append(f"{name}: the draws before first_kept leak into the CPO pass")
    return res


@functools.lru_cache(maxsize=None)
def judged_paths(name):
    c = J.CASE[name]
    d, ref = J.case_data(c), J.ld_pointwise(c)
    fk = c.first_kept
    res = dict(worst={}, fails=[])
    got = {s: dev_paths(c, d, s) for s in SEEDS}
    mean = np.concatenate([ref["fit"][i][fk:] for i in range(c.n)], axis=1)
    b_mean = J.G_PATH * np.concatenate([ref["b_fit_e"][i][fk:] for i in range(c.n)], axis=1)
    mo = np.concatenate([ref["mo"][i][fk:] for i in range(c.n)], axis=1)
    b_mo = J.G_PATH * np.concatenate([ref["b_mo_e"][i][fk:] for i in range(c.n)], axis=1)
    sd = np.sqrt(d["sigma"][fk:].astype(LD))[:, None]
    for s in SEEDS:
        noise, z = J.keyed_noise(c, d, s)
        allow = sd * (32 * np.abs(z) + 4) * U + 2 * U * np.abs(noise) + U * np.abs(mean + noise)
        r1 = J.ratio(got[s]["mo"], mo, b_mo)
        r2 = J.ratio(got[s]["paths"].astype(LD) - noise, mean, b_mean + allow)              # paths - noise: the mean under its bound
        print(f"{name}: seed {s}: error / bound mean_only {r1:.3g}, paths - noise {r2:.3g}")
        _note(res, "k_post_paths", ["all"], "mean_only", r1, name)
        _note(res, "k_post_paths", ["all"], "paths - noise", r2, name)
        if c.M == 0:      # mean_only is then the path's own mean, bit for bit: the noise alone, under the allowance alone
            r3 = J.ratio(got[s]["paths"].astype(LD) - got[s]["mo"].astype(LD), noise, allow)
            print(f"{name}: seed {s}: error / allowance of the noise alone {r3:.3g}")
            _note(res, "k_post_paths", ["noise"], "noise", r3, name)
    a, b = got[SEEDS[0]], got[SEEDS[1]]
    if not np.array_equal(a["mo"].view(np.uint64), b["mo"].view(np.uint64)):
        res["fails"].append(f"{name}: mean_only depends on the seed")
    if np.array_equal(a["paths"], b["paths"]):
        res["fails"].append(f"{name}: the paths do not depend on the seed")
    if not _same_bytes(a, dev_paths(c, d, SEEDS[0])):
        res["fails"].append(f"{name}: two calls of bfmmm_post_sample_paths differ")
    if fk > 0 and not _same_bytes(a, dev_paths(c, _before_first_kept(c, d, np.nan, -1.0), SEEDS[0])):
        res["fails"].append(f"{name}: the draws before first_kept leak into the sample paths")
    return res


def _cases(p):
    return [c.name for c in J.CASES if p in c.passes]


@pytest.mark.parametrize("name", _cases("pw"))
def test_pointwise_entry_by_entry(name):
    res = judged_pointwise(name)
    assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("name", _cases("cpo"))
def test_curve_loglik_and_cpo_entry_by_entry(name):
    res = judged_cpo(name)
    assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("name", _cases("paths"))
def test_sample_paths_entry_by_entry(name):
    res = judged_paths(name)
    assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("case,which,message", J.REFUSED, ids=[q[0].name for q in J.REFUSED])
def test_refusals_by_message(case, which, message):
    from bayesfmmm_amd import _lib, api
    lib = api._lib_entry()
    d = J.make_data(case)
    inp, keep = _input(case, d)
    n_obs = int(np.sum(case.lens))
    with pytest.raises(_lib.BfmmmError, match=message):
        if which == "pw":
            ll, pdf, fit = np.zeros(case.T), np.zeros(n_obs), np.zeros(n_obs)
            api._check(lib.bfmmm_post_pointwise(C.byref(inp), 0, _dp(ll), _dp(pdf), _dp(fit)))
        else:
            cpo = np.zeros(case.n)
            api._check(lib.bfmmm_post_cpo(C.byref(inp), 0, _dp(cpo)))


def test_summary_every_geometry_class_judged():
    worst = {}
    for c in J.CASES:
        for p, fn in (("pw", judged_pointwise), ("cpo", judged_cpo), ("paths", judged_paths)):
            if p in c.passes:
                for k, v in fn(c.name)["worst"].items():
                    worst[k] = max(worst.get(k, 0.0), v)
    for (kernel, lb), v in sorted(worst.items()):
        print(f"largest error / bound, {kernel:18s} {lb:10s}: {v:.3g}")
    for kernel, p in (("k_post_pointwise", "pw"), ("k_post_cpo", "cpo"), ("k_post_cpo_reduce", "cpo")):
        missing = sorted(lb for lb in J.REQUIRED_CLASSES[p] if (kernel, lb) not in worst)
        assert not missing, f"{kernel}: classes never judged: {missing}"
    assert ("k_post_paths", "all") in worst and ("k_post_paths", "noise") in worst
    bad = {k: v for k, v in worst.items() if not v < 1.0}
    assert not bad, f"error / bound not below 1: {bad}"
