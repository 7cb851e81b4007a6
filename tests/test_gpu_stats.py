"""The record builder (csrc/kernels_stats.hip: k_stats_functional<1..5>, k_stats_multivariate, k_stats_totals; the host loop of
bfmmm_create_from_basis) on the device, entry by entry against tests/stats_ref.py.

One sampler per case (tot_mcmc_iters = 1, one chain, no run).  Per case "rec", "ni", dims() and get_basis() are read and held to
every exact check and every bound of stats_ref.check; a second get_basis() is bit-identical to the first, and "rec" is
bit-identical after the get_basis() calls (get_basis relaunches the kernel into scratch and must not touch the records); a
supplied basis comes back bit for bit.  The refusals of set-up are pinned with their messages, each followed by a valid create.
The last test prints the largest error / bound per (degree, P) and asserts that every degree, a curve of more than one chunk, a
point on a knot, both boundaries, lane 0's q = 7, the multivariate kernel at P = 64, the totals kernel at n = 257 and both wide bands
of a supplied basis were judged."""
import numpy as np
import pytest

import factor_ref as F
import stats_ref as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not F.LONGDOUBLE_OK, reason="np.longdouble is not wider than float64 here")]

_records = {}


def make_sampler(c, d=None, deg=None):
    import bayesfmmm_amd as bf
    d = d or S.case_data(c)
    kw = dict(K=2, n_eigen=1, tot_mcmc_iters=1)
    if c.kind == "mv":
        return bf.Sampler(bf.default_config(model=bf.MODEL_MULTIVARIATE, **kw), d["Y"])
    if c.kind == "basis":
        return bf.Sampler(bf.default_config(model=bf.MODEL_FUNCTIONAL, basis_degree=1, **kw), d["y"], basis=d["B"], band=c.band, penalty=d["Pmat"],
                          penalty_band=d["pen_band"])
    return bf.Sampler(bf.default_config(model=bf.MODEL_FUNCTIONAL, basis_degree=deg or c.deg, **kw), d["y"], d["t"], d["ik"], d["bk"])


def run_case(name):
    if name not in _records:
        try:
            _records[name] = _run_case(name)
        except BaseException as e:      # noqa: BLE001 -- pytest.fail raises outside Exception
            _records[name] = e
    if isinstance(_records[name], BaseException):
        raise _records[name]
    return _records[name]


def _run_case(name):
    c = S.BY_NAME[name]
    d = S.case_data(c)
    smp = make_sampler(c)
    n = c.n if c.kind == "mv" else len(d["y"])
    cap = n * c.LREC + 8
    dims = smp.dims()
    extra = []
    rec = smp.debug("rec", cap)
    out = dict(B=None, ni=smp.debug("ni", n + 8).astype(np.int64), dims=dims)
    if rec.shape[0] != n * dims["LREC"]:
        extra.append(f"{name}: \"rec\" has {rec.shape[0]} entries, n LREC = {n * dims['LREC']}")
    if c.kind != "mv":
        B1 = smp.get_basis()
        B2 = smp.get_basis()
        if not all(np.array_equal(a, b) for a, b in zip(B1, B2)):
            extra.append(f"{name}: a second get_basis() differs from the first")
        if not np.array_equal(smp.debug("rec", cap), rec):
            extra.append(f"{name}: \"rec\" changed over get_basis()")
        if c.kind == "basis":
            if not all(np.array_equal(a, b) for a, b in zip(B1, d["B"])):
                extra.append(f"{name}: get_basis() does not return the supplied rows bit for bit")
        else:
            out["B"] = B1
    smp.close()
    out["rec"] = rec.reshape(n, -1)
    res = S.check(c, out)
    res["fails"] += extra
    return res


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_record_builder_against_longdouble(name):
    res = run_case(name)
    print(name, "error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in res["worst"].items()))
    assert not res["fails"], f"{len(res['fails'])} failures\n" + "\n".join(res["fails"][:12])


def _refused(what, message, c, d, **kw):
    from bayesfmmm_amd import _lib
    with pytest.raises(_lib.BfmmmError) as e:
        make_sampler(c, d, **kw).close()
    assert message in str(e.value), f"{what}: refused with '{e.value}'"
    good = S.BY_NAME["lin_P2"]      # a valid create on the same process still works
    res = S.check(good, _fresh(good))
    assert not res["fails"], f"after the refusal of {what}: " + "\n".join(res["fails"][:4])


def _fresh(c):
    d = S.case_data(c)
    smp = make_sampler(c)
    n = len(d["y"])
    out = dict(B=smp.get_basis(), rec=smp.debug("rec", n * c.LREC + 8).reshape(n, -1), ni=smp.debug("ni", n + 8).astype(np.int64), dims=smp.dims())
    smp.close()
    return out


OUTSIDE = "at least one time point lies outside 'boundary_knots'"


@pytest.mark.parametrize("what", ["below b0", "above b1", "nan"])
def test_time_point_outside_is_refused(what):
    c = S.BY_NAME["cubic_P13"]
    d = dict(S.case_data(c))
    b0, b1 = d["bk"]
    t = [x.copy() for x in d["t"]]
    t[3][1] = {"below b0": np.nextafter(b0, -np.inf), "above b1": np.nextafter(b1, np.inf), "nan": np.nan}[what]
    d["t"] = t
    _refused(what, OUTSIDE, c, d)


def test_degree_6_is_refused():
    c = S.BY_NAME["quint_P9_far"]
    _refused("degree 6", "basis_degree larger than 5 is not supported by this build", c, S.case_data(c), deg=6)


def test_P_65_is_refused():
    c = S.BY_NAME["lin_P64"]
    d = dict(S.case_data(c))
    d["ik"] = np.linspace(0.0, 1.0, 65)[1:-1]      # 63 internal knots at degree 1
    _refused("P = 65", "P larger than 64 is not supported by this build", c, d)


def test_largest_errors_and_coverage():
    recs = {c.name: run_case(c.name) for c in S.CASES}
    judged, rows = set(), {}
    for name, res in recs.items():
        c = S.BY_NAME[name]
        judged |= res["judged"]
        key = (c.kind, c.deg, c.P)
        row = rows.setdefault(key, dict(basis=0.0, band=0.0, s=0.0, yy=0.0, YY=0.0))
        for k, v in res["worst"].items():
            row[k] = max(row[k], v)
    for (kind, deg, P), row in sorted(rows.items()):
        print(f"largest device error / bound, {kind:6s} degree {deg} P {P:2d}: " + ", ".join(f"{k} {v:.3g}" for k, v in row.items()))
    need = {f"deg{g}" for g in range(1, 6)} | {"multi_chunk", "knot_hit", "b0", "b1", "q7", "mv_P64", "totals_n257", f"basis_BW{S.BWMID}", f"basis_BW{S.BWWIDE}"}
    assert need <= judged, f"never judged: {sorted(need - judged)}"
    assert all(v <= 1.0 for row in rows.values() for v in row.values())
    assert not any(res["fails"] for res in recs.values())
