"""The restatement of the normalise / clip-guard arithmetic (tests/dynamics_ref.py) against the reference's own known answers
(tests/golden/dynamics_known_answers.json), and the library's host helpers th_limiter_params and th_normalize_gain against the
restatement.  CPU only."""
import json
import math
import os

import numpy as np
import pytest

import thesia_amd as ta
from tests import dynamics_ref as ref

F32 = np.float32
KIND = {"off": ref.NORM_OFF, "lufs": ref.NORM_LUFS, "rms_dB": ref.NORM_RMS_DB, "peak_dB": ref.NORM_PEAK_DB}


@pytest.fixture(scope="module")
def known(golden_dir):
    with open(os.path.join(golden_dir, "dynamics_known_answers.json")) as f:
        return json.load(f)


def test_peak_hold_works(known):
    k = known["peak_hold"]
    assert ref.hold_length_of(k["sr"], 3.0 / k["sr"] * 1000.0) == k["hold_samples"]
    ph = ref.PeakHold(k["hold_samples"])
    assert [ph.step(x) for x in k["audio"]] == k["target"]


def test_peak_hold_is_the_sliding_maximum():
    """... of the last hold_length values, whenever the ring buffer (hold_length.next_power_of_two() slots) is longer than the hold."""
    rng = np.random.default_rng(5)
    for hold in (1, 3, 5, 7, 15, 17, 160, 221, 882, 960, 3840):
        x = rng.standard_normal(3 * hold + 50).tolist()
        ph = ref.PeakHold(hold)
        got = [ph.step(v) for v in x]
        assert got == [max(x[max(0, i + 1 - hold):i + 1]) for i in range(len(x))], hold


def test_peak_hold_at_a_power_of_two_length_loses_a_value():
    """When hold_length is itself a power of two (>= 2) the buffer has no spare slot, and swap_regions' `buffer[i_front & mask] =
    -inf` (envelope.rs:503-504) overwrites the value the next read needs: the reference then holds too LOW now and then.  That is
    the reference's behaviour at sr = 50 * 2^k (hold = sr / 50), none of them a standard rate; the library computes the true sliding
    maximum there, so the restatement is no reference for it at those rates."""
    rng = np.random.default_rng(5)
    for hold in (2, 4, 8, 64, 1024):
        x = rng.standard_normal(3 * hold + 50).tolist()
        ph = ref.PeakHold(hold)
        got = [ph.step(v) for v in x]
        want = [max(x[max(0, i + 1 - hold):i + 1]) for i in range(len(x))]
        assert all(g <= w for g, w in zip(got, want)) and got != want, hold
    assert ref.limiter_params(51200)["hold_length"] == 1024 and ref.limiter_params(48000)["hold_length"] == 960


def test_box_stack_works(known):
    k = known["box_stack"]
    bs = ref.BoxStackFilter(k["size"], k["num_layers"])
    bs.reset(k["reset"])
    assert [bs.step(x) for x in k["input"]] == k["target"]


def test_box_sum_is_a_sliding_sum():
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, 1000)
    for length in (1, 2, 17, 100):
        bs = ref.BoxSum(length)
        for i, v in enumerate(x):
            got = bs.step(float(v), length)
            assert abs(got - x[max(0, i + 1 - length):i + 1].sum()) <= 1e-12


def test_exact_fma():
    assert ref.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0) == 2.0 ** -29 + 2.0 ** -60  # (the product alone would round the last term away)
    assert ref.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    assert ref.fma(0.0, 0.3, 0.7) == 0.7 and math.isinf(ref.fma(math.inf, 1.0, 0.0))


def test_normalize_gains(known):
    k = known["normalize"]
    for case in k["cases"]:
        want = 10.0 ** (case["gain_dB"] / 20.0)
        got_ref = ref.normalize_gain(KIND[case["kind"]], case["target"], k["stats"])
        got_lib = ta.normalize_gain(KIND[case["kind"]], case["target"], k["stats"])
        assert got_ref.dtype == F32 and abs(float(got_ref) - want) <= k["epsilon"], case
        assert abs(float(got_lib) - want) <= k["epsilon"], case
    assert ref.normalize_gain(ref.NORM_OFF, -3.0, k["stats"]) == 1 == ta.normalize_gain(ref.NORM_OFF, -3.0, k["stats"])


def test_normalize_gain_matches_restatement_within_one_ulp():
    rng = np.random.default_rng(7)
    for _ in range(300):
        st = {"global_lufs": float(rng.uniform(-60, 0)), "rms_dB": float(F32(rng.uniform(-60, 0))), "max_peak": 0.5,
              "max_peak_dB": float(F32(rng.uniform(-40, 0)))}
        for kind in (ref.NORM_LUFS, ref.NORM_RMS_DB, ref.NORM_PEAK_DB):
            target = float(F32(rng.uniform(-40, 0)))
            got, want = ta.normalize_gain(kind, target, st), ref.normalize_gain(kind, target, st)
            assert abs(float(got) - float(want)) <= float(np.spacing(want)), (kind, target, st, got, want)
    silent = {"global_lufs": -math.inf, "rms_dB": -math.inf, "max_peak": 0.0, "max_peak_dB": -math.inf}
    for kind in (ref.NORM_LUFS, ref.NORM_RMS_DB, ref.NORM_PEAK_DB):
        assert math.isinf(ta.normalize_gain(kind, -14.0, silent)) and math.isinf(ref.normalize_gain(kind, -14.0, silent))
        assert math.isnan(ta.normalize_gain(kind, math.nan, silent))
    with pytest.raises(ta.ThError) as e:
        ta.normalize_gain(4, -14.0, silent)
    assert e.value.code == -1


def test_guard_stat_cases(known):
    k = known["guard_stats"]
    eps = k["epsilon_dB"]
    for case in k["before_clip"]:
        dB, cnt = ref.stats_from_wav_before_clip(np.array(case["wav"], F32))
        gain = F32(1) / F32(case["gain_of_peak"]) if "gain_of_peak" in case else F32(case["gain"])
        assert cnt == case["reduction_cnt"] and abs(float(dB) - float(ref.db_from_amp(gain))) <= eps, case
        if case["text"] is not None:
            assert ref.format_stats((dB, cnt)) == case["text"]
    for case in k["global_gain"]:
        st = ref.stats_from_global_gain(case["gain"])
        assert st[1] == case["reduction_cnt"] and ref.format_stats(st) == case["text"]
    for case in k["gain_sequence"]:
        dB, cnt = ref.stats_from_gain_seq(np.array(case["row"], F32))
        assert cnt == case["reduction_cnt"] and abs(float(dB) - float(ref.db_from_amp(F32(case["gain"])))) <= eps
    stats = [ref.stats_from_global_gain(c["gain"]) for c in k["by_mode"]["stats"]]
    for mode, key, first in ((ref.GUARD_CLIP, "clip", 0), (ref.GUARD_REDUCE_GLOBAL_LEVEL, "other", -1), (ref.GUARD_LIMITER, "other", -1)):
        sel = ref.select_guard_stats(stats, mode)
        shown = [[first + i, ref.format_stats(s)] for i, s in enumerate(sel) if ref.format_stats(s)]
        assert shown == k["by_mode"][key], mode
    assert abs(float(ref.db_from_amp(F32(0.5))) - (-6.0206)) <= 1e-4 and "%.2f dB" % ref.db_from_amp(F32(0.5)) == "-6.02 dB"
    assert ref.db_from_amp(F32(0)) == -np.inf and np.isnan(ref.db_from_amp(F32(-1))) and ref.db_from_amp(F32(1)) == 0


def test_guard_modes_on_a_small_track():
    x = np.array([[0.0, 0.6, -0.75, 0.25], [-1.0, 0.0, 0.5, 0.125]], F32)
    clip = ref.apply_gain(x, 8000, 2.0, ref.GUARD_CLIP)
    assert np.array_equal(clip["audio"], [[0, 1, -1, 0.5], [-1, 0, 1, 0.25]]) and np.array_equal(clip["drawn"], 2 * x)
    assert clip["result"] == ref.RESULT_BEFORE_CLIP and [c for _, c in clip["guard_stats"]] == [2, 1]
    red = ref.apply_gain(x, 8000, 2.0, ref.GUARD_REDUCE_GLOBAL_LEVEL)
    assert red["global_gain"] == F32(0.5) and np.array_equal(red["audio"], x) and red["drawn"] is red["audio"]
    assert ref.format_stats(red["guard_stats"][0]) == "-6.02 dB" and len(red["guard_stats"]) == 2
    lim = ref.apply_gain(x, 8000, 2.0, ref.GUARD_LIMITER)
    assert lim["result"] == ref.RESULT_GAIN_SEQUENCE and len(lim["guard_stats"]) == 1 and np.abs(lim["audio"]).max() <= 1
    assert lim["gain_seq"].max() <= 1 and lim["gain_seq"].min() >= 0.5 - 1e-6 and ref.limiter_gain_query(lim).shape == (4,)
    quiet = ref.apply_gain(x, 8000, 0.5, ref.GUARD_LIMITER)
    assert np.array_equal(quiet["audio"], F32(0.5) * x) and np.array_equal(ref.limiter_gain_query(quiet), [1.0])
    for g in (1.0, math.inf, math.nan):
        same = ref.apply_gain(x, 8000, g, ref.GUARD_CLIP)
        assert same["audio"] is same["drawn"] and np.array_equal(same["audio"], x) and same["gain"] == 1
        assert same["result"] == ref.RESULT_GLOBAL_GAIN and same["guard_stats"] == [(0, 0), (0, 0)] and ref.limiter_gain_query(same) is None


def test_limiter_is_transparent_below_threshold_and_bounded_above():
    rng = np.random.default_rng(8)
    y = rng.uniform(-0.9, 0.9, (2, 8000)).astype(F32)
    y[0, 700] = 6.0
    g = ref.PerfectLimiter(8000).gain_sequence(y)
    assert g.max() <= 1.0 and np.abs(ref.limit_apply(y, g)).max() <= 1.0
    # the look-ahead starts `attack` steps early; the release ends: the f32 gain is 1 again
    assert g[700] <= 1 / 6 and g[:700 - 40].min() == 1.0 and g[700 - 40] < 1.0 and g.astype(F32)[-1] == 1.0


@pytest.mark.parametrize("sr", [100, 150, 8000, 11025, 16000, 22050, 44100, 48000, 88200, 96000, 192000, 384000])
def test_limiter_params_match_restatement(sr, known):
    got, want = ta.limiter_params(sr), ref.limiter_params(sr)
    assert got == want, (got, want)
    assert sum(got["box_len"]) == got["attack"] + 2
    if str(sr) in known["limiter_box_lengths"]:
        assert got["box_len"] == known["limiter_box_lengths"][str(sr)]
    for key, val in known["limiter_rounding"].get(str(sr), {}).items():
        assert got[key] == val  # round half away from zero: 220.5 -> 221


def test_limiter_params_refuse_a_zero_attack():
    for sr in (0, 50, 99):
        with pytest.raises(ta.ThError) as e:
            ta.limiter_params(sr)
        assert e.value.code == -2
