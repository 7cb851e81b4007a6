"""Rows above 8192 draws through the host code of the cluster summaries (capi_cluster.hip): Sampler.cluster_cov_bands,
Sampler.cluster_contrast_bands and Sampler.cluster_eigen on the 2 chains x 4100 slots of
tests/test_gpu_align.py::test_rows_longer_than_8192_draws, N = 8200 draws per row, where the quantiles sort in a workspace
(k_bands_quantiles_big), the band's deviations do too, and with several chunks the second sweep runs and crit is read off in pieces.
The reductions are held to the returned traces by the helpers of tests/test_gpu_cluster_cov.py and tests/test_gpu_cluster_eig.py
with their bounds, the band of the contrasts to tests/cluster_cov_ref.py's rule on the returned trace; chunked calls equal the
one-chunk call byte for byte and launch as often as their chunks say."""
import re

import numpy as np
import pytest

import cluster_cov_ref as CCR
import test_gpu_cluster_contrast as CT
import test_gpu_cluster_cov as CC
import test_gpu_cluster_eig as CE

pytestmark = pytest.mark.gpu

N_CURVES, P, K, T, NCH = 12, 3, 2, 4100, 2
N = NCH * T                      # 8200 draws per row


@pytest.fixture(scope="module")
def long_rows():
    import bayesfmmm_amd as bf
    rng = np.random.default_rng(6)
    cfg = bf.default_config(model=bf.MODEL_MULTIVARIATE, K=K, n_eigen=1, tot_mcmc_iters=T)
    smp = bf.Sampler(cfg, rng.standard_normal((N_CURVES, P)), n_chains=NCH)
    for q in range(NCH):
        smp.select_chain(q)
        smp.init_state(1, 21, chain=q)
    smp.select_chain(0)
    smp.run(bf.SWEEP_WARM, T, seed=21)
    perm = smp.align(pivot=(0, T - 1))["perm"]
    yield dict(smp=smp, perm=perm, E=np.eye(P))
    smp.close()


def test_cluster_cov_bands(long_rows):
    smp, perm, E = long_rows["smp"], long_rows["perm"], long_rows["E"]
    kw = dict(probs=(0.05, 0.5, 0.95), simultaneous=0.1, trace=True)
    one = smp.cluster_cov_bands(E, perm, **kw)                        # 3 pairs x 3 x 3 = 27 rows in one chunk
    assert one["trace"].shape == (3, P, P, N)
    assert smp.timing("cluster_cov")[1] == 1 and smp.timing("cluster_cov_maxdev")[1] == 1
    CC._check_reductions(one, 0.1, "8200 draws")
    shared, per_row = CC._budget_figures(smp, E, perm, **kw)
    # 4 rows a chunk: crit's 3 rows in one piece; 2 rows a chunk: in two
    for rows, nchunks in ((4, 7), (2, 14)):
        got = smp.cluster_cov_bands(E, perm, max_workspace_bytes=shared + rows * per_row + 7, **kw)
        CC._same(got, one, CC.ALL)
        assert smp.timing("cluster_cov")[1] == 2 * nchunks and smp.timing("cluster_cov_maxdev")[1] == nchunks


def test_cluster_contrast_bands(long_rows):
    """the band of the contrasts on long rows: dev's rows sort in the workspace, and with several chunks the second sweep runs"""
    smp, perm, E = long_rows["smp"], long_rows["perm"], long_rows["E"]
    lists = [[(1, 0), (-1, 1)], [(1, 0)], [(1, 1)]]
    kw = dict(perm=perm, probs=(0.05, 0.5, 0.95), simultaneous=0.1, trace=True)
    one = smp.cluster_contrast_bands(E, lists, **kw)                  # 3 contrasts x 3 = 9 rows in one chunk
    assert one["trace"].shape == (3, P, N) and one["norm_trace"].shape == (3, NCH, T)
    assert smp.timing("contrast_values")[1] == 1 and smp.timing("contrast_norm")[1] == 1
    s = CCR.sim_bands(one["trace"], 0.1, one["mean"], one["sd"])
    for k in ("crit", "lower", "upper"):
        assert one[k].tobytes() == np.ascontiguousarray(s[k]).tobytes(), k
    with pytest.raises(Exception) as ei:
        smp.cluster_contrast_bands(E, lists, max_workspace_bytes=1, **kw)
    m = re.search(r"\((\d+) shared by all rows \+ (\d+) per row\)", str(ei.value))
    assert m and "bfmmm_chain_cluster_contrast_bands: 'max_workspace_bytes' below the" in str(ei.value), str(ei.value)
    shared, per_row = int(m.group(1)), int(m.group(2))
    # 4 rows a chunk: crit's 3 rows in one piece; 2 rows a chunk: in two
    for rows, nchunks in ((4, 3), (2, 5)):
        got = smp.cluster_contrast_bands(E, lists, max_workspace_bytes=shared + rows * per_row + 7, **kw)
        CT._same(got, one, CT.KEYS + CT.BAND + ("trace", "norm_trace"))
        assert smp.timing("contrast_values")[1] == 2 * nchunks and smp.timing("contrast_norm")[1] == nchunks


def test_cluster_eigen(long_rows):
    smp, perm, E = long_rows["smp"], long_rows["perm"], long_rows["E"]
    one = smp.cluster_eigen(E, perm, n_functions=1, trace=True)      # 2 x 1 x 3 = 6 eigenfunction rows in one chunk
    assert one["values_trace"].shape == (K, 1, N) and one["functions_trace"].shape == (K, 1, P, N)
    assert smp.timing("cluster_eig_values")[1] == 1
    CE._check_reductions(one, smp, T, "8200 draws")
    # the reference functions of the first call as an array: the budget then applies to this call alone
    kw = dict(n_functions=1, ref=one["ref"], trace=True)
    shared, per_row = CE._budget_figures(smp, E, perm, **kw)
    for rows, nchunks in ((2, 3), (1, 6)):
        got = smp.cluster_eigen(E, perm, max_workspace_bytes=shared + rows * per_row + 7, **kw)
        CE._same(got, one)
        assert smp.timing("cluster_eig_values")[1] == nchunks and smp.timing("cluster_eig")[1] == 1
