"""Host arithmetic of the loudness path (th_k_weighting, th_loudness_n_blocks, th_gated_loudness) against BS.1770-4's published
coefficients and the restatement in tests/loudness_ref.py.  CPU only."""
import math

import numpy as np
import pytest

import thesia_amd as ta
from tests import loudness_ref as ref


def test_k_weighting_48k_matches_bs1770_tables():
    b, a = ta.k_weighting(48000)
    want_b = np.convolve(ref.BS1770_STAGE1[0], ref.BS1770_STAGE2[0])
    want_a = np.convolve(ref.BS1770_STAGE1[1], ref.BS1770_STAGE2[1])
    assert a[0] == 1.0
    assert np.abs(b - want_b).max() <= 1e-12, b - want_b
    assert np.abs(a - want_a).max() <= 1e-12, a - want_a


@pytest.mark.parametrize("sr", [8000, 11025, 16000, 22050, 44100, 48000, 88200, 96000, 192000, 16, 2_822_400])
def test_k_weighting_matches_restatement(sr):
    b, a = ta.k_weighting(sr)
    wb, wa = ref.k_weighting(sr)
    for got, want in ((b, wb), (a, wa)):
        ulp = np.spacing(np.abs(want))
        assert np.all(np.abs(got - want) <= 4 * ulp), (sr, got - want)


def test_unsupported_rates_are_refused():
    for sr in (0, 15, 2_822_401):
        with pytest.raises(ta.ThError) as e:
            ta.k_weighting(sr)
        assert e.value.code == -2
        with pytest.raises(ta.ThError):
            ta.loudness_n_blocks(100000, sr)


@pytest.mark.parametrize("sr", [16, 8000, 11025, 44100, 48000, 192000])
def test_n_blocks_at_the_block_edges(sr):
    s = ref.s100(sr)
    L = 4 * s
    assert s == (sr + 5) // 10 and (sr != 11025 or s == 1103)
    for n, want in ((0, 0), (L - 1, 0), (L, 1), (L + s - 1, 1), (L + s, 2), (L + 8 * s - 1, 8)):
        assert ta.loudness_n_blocks(n, sr) == want == ref.n_blocks(n, sr), (sr, n)


def _same(x, y):
    return (math.isnan(x) and math.isnan(y)) or x == y


def test_gated_loudness_random_series():
    rng = np.random.default_rng(11)
    for n in (1, 2, 5, 40, 297, 3000):
        for spread in (3.0, 30.0, 90.0):
            lufs = rng.uniform(-40 - spread, -10, n)
            e = 10.0 ** ((lufs + 0.691) / 10.0)
            got, want = ta.gated_loudness(e), ref.gated_loudness(e)
            assert _same(got, want), (n, spread, got, want)


def test_gated_loudness_edge_cases():
    B, Eps = ref.BOUNDARIES, ref.ENERGIES
    cases = {
        "no blocks": [],
        "all below -70": [B[0] * 0.999, 1e-12, 0.0, -1.0],
        "on boundaries": list(B[[0, 1, 500, 999, 1000]]),
        "above +30": [1e4, 1e6, 10.0 ** ((31 + 0.691) / 10)],
        "NaN energies": [float("nan"), B[700], float("nan"), B[300]],
        "NaN only": [float("nan")] * 3,
    }
    j = 800
    cases["one bin"] = [Eps[j]] * 4
    for name, e in cases.items():
        got, want = ta.gated_loudness(e), ref.gated_loudness(e)
        assert _same(got, want), (name, got, want)
    assert ta.gated_loudness([]) == -math.inf
    assert ta.gated_loudness(cases["all below -70"]) == -math.inf
    assert ta.gated_loudness([float("nan")] * 3) == -math.inf
    assert ta.gated_loudness([1e6]) == pytest.approx(10 * math.log10(Eps[999]) - 0.691, abs=1e-12)
    # R exactly on a centre (the '>' rule): a single-bin series has R = 0.1 eps_j; replace eps_j by the value whose R is exactly a
    # centre eps_r, then blocks in bin r stay when R == eps_r and go when R is one ulp above it
    r = ref.hist_index(0.1 * Eps[j])
    for bump in (0, 1):
        top = Eps[r] * 10.0
        if bump:
            top = np.nextafter(top, np.inf)
        e = [top] * 50 + [Eps[r]]
        R = 0.1 * (sum(float(c) * Eps[ref.hist_index(v)] for c, v in ((50, top), (1, Eps[r])))) / 51.0
        assert _same(ta.gated_loudness(e), ref.gated_loudness(e)), (bump, R, Eps[r])
