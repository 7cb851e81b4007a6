"""api.read_batches: the reference's on-disk chain batches as arrays in Sampler.get_chain's layouts -- the chain the
reference ships entry for entry against the individual readers, and two files written here whose covariate containers are
longer than the draw count, concatenated, with and without the unassigned first draw of every file."""
import os

import numpy as np
import pytest

TRACE = os.path.join(os.path.dirname(__file__), "golden", "Functional_trace") + "/"


@pytest.fixture(scope="module")
def api():
    __import__("__graft_entry__").build()
    from bayesfmmm_amd import api
    return api


def test_shipped_chain_equals_the_individual_readers(api):
    d = api.read_batches(TRACE, 1, X=True, cov_adj=True)
    T = 150
    assert d["n_draws"] == T
    want = {"nu": (2, 7, T), "Z": (40, 2, T), "chi": (40, 3, T), "Phi": (2, 7, 3, T), "sigma_sq": (T,), "pi": (2, T), "alpha_3": (T,),
            "A": (2, 2, T), "delta": (2, 3, T), "tau": (T, 2), "gamma": (2, 7, 3, T), "eta": (7, 1, 2, T), "tau_eta": (2, 1, T),
            "xi": (7, 1, 3, 2, T), "gamma_xi": (7, 1, 3, 2, T), "delta_xi": (2, 3, 1, T), "A_xi": (2, 2, 1, T)}
    assert {k: v.shape for k, v in d.items() if k != "n_draws"} == want
    for key, name in (("nu", "Nu"), ("Z", "Z"), ("chi", "Chi"), ("A", "A"), ("delta", "Delta"), ("pi", "Pi"), ("tau", "Tau")):
        np.testing.assert_array_equal(d[key], api.ReadCube(f"{TRACE}{name}0.txt"), err_msg=key)
    np.testing.assert_array_equal(d["sigma_sq"], api.ReadVec(TRACE + "Sigma0.txt"))
    np.testing.assert_array_equal(d["alpha_3"], api.ReadVec(TRACE + "alpha_30.txt"))
    np.testing.assert_array_equal(d["tau_eta"], api.ReadCube(TRACE + "Tau_Eta0.txt")[..., :T])
    for key, name in (("Phi", "Phi"), ("gamma", "Gamma"), ("eta", "Eta"), ("delta_xi", "Delta_Xi"), ("A_xi", "A_Xi")):
        f = api.ReadFieldCube(f"{TRACE}{name}0.txt")
        for l in range(T):
            np.testing.assert_array_equal(d[key][..., l], f[l, 0], err_msg=key)
    for key, name in (("xi", "Xi"), ("gamma_xi", "Gamma_Xi")):
        f = api.ReadFieldCube(f"{TRACE}{name}0.txt")
        for l in range(T):
            for k in range(2):
                np.testing.assert_array_equal(d[key][..., k, l], f[l, k], err_msg=key)
    # the levels: without X no covariate block, with X alone the mean blocks
    assert not {"eta", "tau_eta", "xi"} & set(api.read_batches(TRACE, 1))
    assert {"eta", "tau_eta"} <= set(api.read_batches(TRACE, 1, X=True)) and "xi" not in api.read_batches(TRACE, 1, X=True)


def _write_two_files(api, d, per, rs, seed=1):
    """two files of `per` draws whose covariate containers hold rs > per entries (empty cubes, ones in Tau_Eta: save_batch)"""
    rng = np.random.default_rng(seed)
    n, K, P, M, D = 5, 2, 4, 2, 2
    truth = {}
    for q in range(2):
        a = {"Nu": rng.standard_normal((K, P, per)), "Chi": rng.standard_normal((n, M, per)), "Z": rng.dirichlet(np.ones(K), (n, per)).transpose(0, 2, 1),
             "A": rng.uniform(1, 2, (K, 2, per)), "Delta": rng.uniform(1, 2, (K, M, per)), "Pi": rng.dirichlet(np.ones(K), per).T,
             "Sigma": rng.uniform(0.1, 1, per), "alpha_3": np.concatenate([[0.0], rng.uniform(1, 9, per - 1)]), "Tau": rng.uniform(1, 2, (per, K))}
        for nm, v in a.items():
            api.write_arma_ascii(d / f"{nm}{q}.txt", v)
        te = np.ones((K, D, rs))
        te[..., :per] = rng.uniform(1, 2, (K, D, per))
        api.write_arma_ascii(d / f"Tau_Eta{q}.txt", te)
        a["Tau_Eta"] = te[..., :per]
        for nm, shp, cols, rows in (("Phi", (K, P, M), 1, per), ("Gamma", (K, P, M), 1, per), ("Eta", (P, D, K), 1, rs), ("Delta_Xi", (K, M, D), 1, rs),
                                    ("A_Xi", (K, 2, D), 1, rs), ("Xi", (P, D, M), K, rs), ("Gamma_Xi", (P, D, M), K, rs)):
            f = np.empty((rows, cols), dtype=object)
            for l in range(rows):
                for k in range(cols):
                    f[l, k] = rng.standard_normal(shp) if l < per else np.zeros((0, 0, 0))
            api.write_arma_field(d / f"{nm}{q}.txt", f)
            a[nm] = f
        truth[q] = a
    return truth, (n, K, P, M, D)


def test_two_written_files_come_back_concatenated(api, tmp_path):
    per, rs = 4, 7
    truth, (n, K, P, M, D) = _write_two_files(api, tmp_path, per, rs)
    d = api.read_batches(str(tmp_path) + "/", 2, X=True, cov_adj=True)
    T = 2 * per
    assert d["n_draws"] == T and d["xi"].shape == (P, D, M, K, T) and d["eta"].shape == (P, D, K, T) and d["tau"].shape == (T, K)
    key_of = {"Nu": "nu", "Chi": "chi", "Z": "Z", "A": "A", "Delta": "delta", "Pi": "pi", "Sigma": "sigma_sq", "alpha_3": "alpha_3",
              "Tau_Eta": "tau_eta"}
    for q in range(2):
        a = truth[q]
        for nm, key in key_of.items():
            np.testing.assert_array_equal(d[key][..., q * per:(q + 1) * per], a[nm], err_msg=nm)
        np.testing.assert_array_equal(d["tau"][q * per:(q + 1) * per], a["Tau"])
        for l in range(per):
            for nm, key in (("Phi", "Phi"), ("Gamma", "gamma"), ("Eta", "eta"), ("Delta_Xi", "delta_xi"), ("A_Xi", "A_xi")):
                np.testing.assert_array_equal(d[key][..., q * per + l], a[nm][l, 0], err_msg=nm)
            for k in range(K):
                np.testing.assert_array_equal(d["xi"][..., k, q * per + l], a["Xi"][l, k])
                np.testing.assert_array_equal(d["gamma_xi"][..., k, q * per + l], a["Gamma_Xi"][l, k])
    assert d["alpha_3"][0] == 0.0 and d["alpha_3"][per] == 0.0
    # drop_unassigned removes exactly draws 0 and per, from every array
    e = api.read_batches(str(tmp_path) + "/", 2, X=True, cov_adj=True, drop_unassigned=True)
    keep = [t for t in range(T) if t not in (0, per)]
    assert e["n_draws"] == T - 2 and set(e) == set(d)
    for key, v in d.items():
        if key == "n_draws":
            continue
        np.testing.assert_array_equal(e[key], v[keep] if key == "tau" else v[..., keep], err_msg=key)
    assert np.all(e["alpha_3"] > 0)


def test_refusals(api, tmp_path):
    _write_two_files(api, tmp_path, 3, 3)
    with pytest.raises(ValueError, match="'n_files' must be greater than 0"):
        api.read_batches(str(tmp_path) + "/", 0)
    os.remove(tmp_path / "Pi1.txt")
    with pytest.raises(FileNotFoundError, match="Pi1.txt"):
        api.read_batches(str(tmp_path) + "/", 2)
    os.remove(tmp_path / "Pi0.txt")      # an optional file that is missing everywhere is skipped
    assert "pi" not in api.read_batches(str(tmp_path) + "/", 2)
    os.remove(tmp_path / "Phi1.txt")
    with pytest.raises(FileNotFoundError, match="Phi1.txt"):
        api.read_batches(str(tmp_path) + "/", 2)
