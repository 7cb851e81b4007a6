"""bfmmm_get_timing: every public name is accepted, "curve_fit" is the sum of its four kernel families as the library adds them,
each post-processing call counts the launches of the route it took, and bfmmm_debug_get("curve_ll_ms") reports the device time
of the per-curve log-density.  No duration is compared with anything but zero."""
import numpy as np
import pytest

from tiny_sampler import basis_rows, make_tiny

pytestmark = pytest.mark.gpu

NAMES = ("total", "curve_z", "pair_gram", "factor", "sweep", "curve_chi", "loglik", "pg_reduce", "curve_fit_project",
         "curve_fit_rows", "curve_fit_values", "curve_fit_reduce", "curve_fit", "curve_sim", "curve_sim_reduce", "similarity",
         "curve_cov_project", "curve_cov")
FIT_PARTS = ("curve_fit_project", "curve_fit_rows", "curve_fit_values", "curve_fit_reduce")


@pytest.fixture(scope="module")
def smp():
    s = make_tiny(run=True)
    yield s
    s.close()


def _fit_sum_holds(smp):
    ms, launches = 0.0, 0
    for nm in FIT_PARTS:
        a, b = smp.timing(nm)
        ms += a
        launches += b
    assert smp.timing("curve_fit") == (ms, launches)
    assert ms > 0.0


def test_every_name_is_accepted(smp):
    from bayesfmmm_amd import _lib
    for nm in NAMES:
        ms, launches = smp.timing(nm)
        assert ms >= 0.0 and launches >= 0, nm
    for nm in ("nope", "curve_ll", "curve_ll_ms", ""):
        with pytest.raises(_lib.BfmmmError, match="unknown name") as ei:
            smp.timing(nm)
        assert str(ei.value) == "bfmmm_get_timing: unknown name"


def test_curve_fit_is_the_sum_of_its_families_on_both_routes(smp):
    E = basis_rows(smp, 3)
    smp.curve_bands(E)
    _fit_sum_holds(smp)
    assert smp.timing("curve_fit_project")[1] == 1 and smp.timing("curve_fit_project")[0] > 0.0
    assert smp.timing("curve_fit_rows")[1] >= 1 and smp.timing("curve_fit_rows")[0] > 0.0
    assert smp.timing("curve_fit_values") == (0.0, 0) and smp.timing("curve_fit_reduce") == (0.0, 0)
    smp.lib.bfmmm_set_curve_fit_route(1)
    try:
        smp.curve_bands(E)
        _fit_sum_holds(smp)
        assert smp.timing("curve_fit_project")[1] == 1
        assert smp.timing("curve_fit_rows") == (0.0, 0)
        assert smp.timing("curve_fit_values")[1] >= 1 and smp.timing("curve_fit_values")[0] > 0.0
        assert smp.timing("curve_fit_reduce")[1] >= 1 and smp.timing("curve_fit_reduce")[0] > 0.0
    finally:
        smp.lib.bfmmm_set_curve_fit_route(0)


def test_curve_cov_project_reports_one_launch_per_table(smp):
    E = basis_rows(smp, 5)
    smp.curve_cov(E[:3], E[3:])
    assert smp.timing("curve_cov_project")[1] == 2 and smp.timing("curve_cov_project")[0] > 0.0
    assert smp.timing("curve_cov")[1] == 1 and smp.timing("curve_cov")[0] > 0.0
    smp.curve_cov(E[:3])
    assert smp.timing("curve_cov_project")[1] == 1 and smp.timing("curve_cov_project")[0] > 0.0


def test_the_other_calls_report_their_time(smp):
    smp.curve_loglik()
    v = smp.debug("curve_ll_ms", 8)
    assert v.shape == (1,) and v[0] > 0.0
    smp.similarity()
    assert smp.timing("similarity")[1] == 1 and smp.timing("similarity")[0] > 0.0
    smp.curve_bands_simultaneous(basis_rows(smp, 3))
    assert smp.timing("curve_sim")[1] == 1 and smp.timing("curve_sim")[0] > 0.0
    assert smp.timing("curve_sim_reduce") == (0.0, 0)
    assert np.isfinite(smp.timing("total")[0])
