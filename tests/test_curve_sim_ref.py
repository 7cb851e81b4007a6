"""The rule of the simultaneous band (tests/curve_sim_ref.py) does what it claims, on random (G, N) tables: at
least min(max(floor(N (1 - alpha) + 0.5), 1), N) draws have C <= crit, and at least that many lie inside [lower, upper] at
EVERY grid point once the band is widened by 4 2^-52 max|v| of the row (mean -/+ crit sd is rounded twice per side; without the
widening 2 of 560 such tables missed by an ulp); a constant row (sd exactly 0) does not change crit and its band is its mean;
one draw gives NaN.  No GPU."""
import numpy as np
import pytest

import curve_sim_ref as S

NS = (2, 3, 20, 21, 92, 257, 4001)
GS = (1, 2, 7, 65)
ALPHAS = (0.001, 0.05, 0.5, 0.999)
KINDS = ("plain", "scaled", "constant", "ties", "ties+constant")
CONSTANTS = (0.0, 1.5, -2.0)          # N of them sum exactly, so numpy's sd of the row is exactly 0


def _table(kind, G, N, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((G, N))
    if kind == "scaled":
        v = v * np.exp(rng.uniform(-6, 6, (G, 1))) + rng.uniform(-100, 100, (G, 1))
    if kind.startswith("ties"):
        v = np.round(v, 1)
    return v


def _need(N, alpha):
    return min(max(int(np.floor(N * (1.0 - alpha) + 0.5)), 1), N)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", NS)
def test_band_contains_the_draws_it_claims(N, kind):
    for G in GS:
        for ai, alpha in enumerate(ALPHAS):
            v = _table(kind, G, N, seed=1000 * N + 10 * G + ai)
            base = S.sim_bands(v[None], alpha)
            if kind.endswith("constant"):
                c = CONSTANTS[(N + G + ai) % 3]
                pos = (N + ai) % (G + 1)
                v = np.insert(v, pos, np.full(N, c), axis=0)
            out = S.sim_bands(v[None], alpha)
            need = _need(N, alpha)
            tag = (kind, G, N, alpha)
            assert np.all(np.isfinite(out["crit"])) and out["crit"][0] >= 0.0, tag
            assert int(np.sum(out["C"][0] <= out["crit"][0])) >= need, tag
            wid = 4 * 2.0 ** -52 * np.abs(v).max(axis=1)
            inside = np.all((v >= (out["lower"][0] - wid)[:, None]) & (v <= (out["upper"][0] + wid)[:, None]), axis=0)
            assert int(inside.sum()) >= need, tag
            if kind.endswith("constant"):
                assert out["sd"][0, pos] == 0.0, tag
                assert out["crit"].tobytes() == base["crit"].tobytes(), tag
                assert out["lower"][0, pos] == c and out["upper"][0, pos] == c and out["mean"][0, pos] == c, tag
                keep = np.arange(G + 1) != pos
                for k in ("lower", "upper"):
                    assert np.ascontiguousarray(out[k][0, keep]).tobytes() == base[k][0].tobytes(), (k, tag)


def test_every_row_constant_gives_crit_zero():
    v = np.stack([np.full(20, c) for c in CONSTANTS])[None]
    out = S.sim_bands(v, 0.05)
    assert out["crit"][0] == 0.0 and np.all(out["sd"] == 0.0)
    assert np.array_equal(out["lower"], out["mean"]) and np.array_equal(out["upper"], out["mean"])


def test_one_draw_gives_nan():
    out = S.sim_bands(np.random.default_rng(0).standard_normal((3, 5, 1)), 0.05)
    for k in ("sd", "crit", "lower", "upper"):
        assert np.all(np.isnan(out[k])), k
    assert np.all(np.isfinite(out["mean"]))


def test_moments_can_be_given():
    v = np.random.default_rng(1).standard_normal((2, 7, 21))
    own = S.sim_bands(v, 0.1)
    given = S.sim_bands(v, 0.1, mean=own["mean"], sd=own["sd"])
    for k in ("crit", "lower", "upper"):
        assert own[k].tobytes() == given[k].tobytes()
