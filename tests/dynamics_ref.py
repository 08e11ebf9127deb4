"""Literal, sequential restatement of the reference's normalise / clip-guard arithmetic for the tests: Normalize::normalize_default
(dynamics/normalize.rs:23-45), AudioTrack::apply_gain (track.rs:158-170), Audio::clip / reduce_global_level / limit (audio.rs:133-179),
PerfectLimiter (dynamics/limiter.rs) over PeakHold, BoxSum, BoxFilter, BoxStackFilter (dynamics/envelope.rs) and ExponentialRelease,
and GuardClippingStats (dynamics/stats.rs:111-205).  f64 arithmetic is Python's float (IEEE double, one rounding per operation);
mul_add is an EXACT fused multiply-add (one rounding of the exact rational result); f32 arithmetic is numpy's float32.
Test infrastructure only: the product never imports it."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
NORM_OFF, NORM_LUFS, NORM_RMS_DB, NORM_PEAK_DB = 0, 1, 2, 3
GUARD_CLIP, GUARD_REDUCE_GLOBAL_LEVEL, GUARD_LIMITER = 0, 1, 2
RESULT_GLOBAL_GAIN, RESULT_BEFORE_CLIP, RESULT_GAIN_SEQUENCE = 0, 1, 2
F64_EPSILON = 2.0 ** -52
NEG_INF = -math.inf


def fma(a, b, c):
    """f64::mul_add: a * b + c rounded once (Fraction -> float is correctly rounded)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def round_half_away(x):
    """f64::round"""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def db_from_amp(x):
    """dB_from_amp_default of an f32 (decibel.rs:66-102 with ref 1, amin 0): 20 log10 x; the logarithm in f64, rounded to f32 once"""
    x = float(x)
    if math.isnan(x) or math.copysign(1.0, x) < 0:
        return F32(np.nan)
    return F32(-np.inf) if x == 0 else F32(20.0 * math.log10(x))


# ---------------------------------------------------------------------------------------------- normalize.rs
def normalize_gain(kind, target, stats):
    """stats: dict of th_audio_stats of the ORIGINAL.  10f32.powf((target - stat) / 20) in f32"""
    if kind == NORM_OFF:
        return F32(1)
    stat = {NORM_LUFS: F32(stats["global_lufs"]), NORM_RMS_DB: F32(stats["rms_dB"]), NORM_PEAK_DB: F32(stats["max_peak_dB"])}[kind]
    with np.errstate(all="ignore"):
        return np.power(F32(10), (F32(target) - stat) / F32(20), dtype=F32)


# ---------------------------------------------------------------------------------------------- envelope.rs
class BoxSum:
    def __init__(self, max_length):
        self.buffer, self.capacity, self.index, self.sum, self.wrap_jump = [], 0, 0, 0.0, 0.0
        self.resize(max_length)

    def resize(self, max_length):
        buf_length = max_length + 1
        if buf_length > self.capacity:  # reserve_exact(buf_length - capacity): capacity >= len + additional
            self.capacity = max(self.capacity, len(self.buffer) + (buf_length - self.capacity))
        else:
            del self.buffer[buf_length:]
            self.capacity = len(self.buffer)  # shrink_to_fit
        self.reset(0.0)

    def reset(self, value):
        self.index, self.sum = 0, 0.0
        buf_length = self.capacity
        self.buffer = []
        s = 0.0
        for _ in range(buf_length):
            self.buffer.append(s)
            s = s + value
        self.wrap_jump = s

    def read(self, width):
        if self.index >= width:
            return self.sum - self.buffer[self.index - width]
        return self.sum + self.wrap_jump - self.buffer[self.index + len(self.buffer) - width]

    def write(self, value):
        self.index += 1
        if self.index == len(self.buffer):
            self.index = 0
            self.wrap_jump = self.sum
            self.sum = 0.0
        self.sum += value
        self.buffer[self.index] = self.sum

    def step(self, value, width):
        self.write(value)
        return self.read(width)


class BoxFilter:
    def __init__(self, max_length):
        self.box_sum, self.length, self.max_length, self.multiplier = BoxSum(max_length), max_length, max_length, 1.0 / max_length

    def resize(self, max_length):
        self.box_sum.resize(max_length)
        self.max_length = max_length
        self.set(max_length)

    def set(self, length):
        self.length = length
        self.multiplier = 1.0 / length
        if length > self.max_length:
            self.resize(length)

    def reset(self, fill):
        self.box_sum.reset(fill)

    def step(self, value):
        return self.box_sum.step(value, self.length) * self.multiplier


HARDCODED_RATIOS = [1., 0.582241861690, 0.417758138310, 0.404078562416, 0.334851475794, 0.261069961789, 0.307944914938, 0.273699452340,
                    0.229132636010, 0.189222996712, 0.248329349789, 0.229253789144, 0.201191468123, 0.173033035122, 0.148192357821,
                    0.205275202874, 0.198413552119, 0.178256637764, 0.157821404506, 0.138663023387, 0.121570179349]


class BoxStackFilter:
    """with_num_layers(max_size, num_layers), num_layers <= 6 (the hard-coded ratios)"""

    def __init__(self, max_size, num_layers):
        i_start = num_layers * (num_layers - 1) // 2
        ratios = HARDCODED_RATIOS[i_start:i_start + num_layers]
        total = 0.0
        for r in ratios:  # ndarray's sum of fewer than 8 elements: sequential
            total = total + r
        self.layers = [{"filter": BoxFilter(1), "length": 1, "ratio": r / total, "length_err": 0.0} for r in ratios]
        for layer in self.layers:
            layer["filter"].resize(1)
        self.size = None
        self.set(max_size)
        self.reset(0.0)

    def set(self, size):
        if self.size == size:
            return
        order = size - 1
        total_order = 0
        for layer in self.layers:
            frac = layer["ratio"] * float(order)
            layer_order = int(frac)
            layer["length"] = layer_order + 1
            layer["length_err"] = float(layer_order) - frac
            total_order += layer_order
        for _ in range(total_order, order):
            i_min, mn = 0, math.inf
            for i, layer in enumerate(self.layers):
                if layer["length_err"] < mn:
                    i_min, mn = i, layer["length_err"]
            self.layers[i_min]["length"] += 1
            self.layers[i_min]["length_err"] += 1.0
        for layer in self.layers:
            layer["filter"].set(layer["length"])

    def reset(self, fill):
        for layer in self.layers:
            layer["filter"].reset(fill)

    def step(self, value):
        for layer in self.layers:
            value = layer["filter"].step(value)
        return value

    def lengths(self):
        return [layer["length"] for layer in self.layers]


def hold_length_of(sr, hold_ms):
    return int(round_half_away(float(sr) * hold_ms / 1000.0))


class PeakHold:
    """PeakHold::new(sr, hold_ms) with hold_length = round(sr * hold_ms / 1000), given here directly"""

    def __init__(self, hold_length):
        buf_length = 1
        while buf_length < hold_length:
            buf_length <<= 1  # next_power_of_two
        self.buffer = [NEG_INF] * buf_length
        self.buf_mask = buf_length - 1
        self.i_back = 0
        self.i_front = hold_length
        self.reset(NEG_INF)

    def hold_length(self):
        return self.i_front - self.i_back

    def reset(self, fill):
        hold_length = self.hold_length()
        self.buffer = [fill] * len(self.buffer)
        self.i_back = 0
        self.i_mid_start = hold_length // 2
        self.i_working = self.i_mid_end = self.i_front = hold_length
        self.front_max = self.working_max = self.middle_max = NEG_INF

    def step(self, value):
        self.push(value)
        self.pop()
        return self.read()

    def push(self, value):
        self.buffer[self.i_front & self.buf_mask] = value
        self.i_front += 1
        self.front_max = max(self.front_max, value)

    def pop(self):
        if self.i_back == self.i_mid_start:
            self.swap_regions()
        self.i_back += 1
        if self.i_working != self.i_mid_start:
            self.i_working -= 1
            i = self.i_working & self.buf_mask
            self.working_max = max(self.working_max, self.buffer[i])
            self.buffer[i] = self.working_max

    def read(self):
        return max(max(self.buffer[self.i_back & self.buf_mask], self.middle_max), self.front_max)

    def swap_regions(self):
        self.working_max = NEG_INF
        self.middle_max = self.front_max
        self.front_max = NEG_INF
        prev_front_len = self.i_front - self.i_mid_end
        prev_mid_len = self.i_mid_end - self.i_mid_start
        if prev_front_len <= prev_mid_len + 1:
            self.i_mid_start = self.i_mid_end
            self.i_mid_end = self.i_front
            self.i_working = self.i_mid_end
        else:
            mid_len = (self.i_front - self.i_mid_start) // 2
            self.i_mid_start = self.i_mid_end
            self.i_mid_end += mid_len
            back_len = self.i_mid_start - self.i_back
            working_len = min(back_len, self.i_mid_end - self.i_mid_start)
            self.i_working = self.i_mid_start + working_len
            m = NEG_INF
            for i in range(self.i_mid_end, self.i_front):
                m = max(m, self.buffer[i & self.buf_mask])
            self.front_max = max(self.front_max, m)
            for i in range(self.i_mid_end - 1, self.i_working - 1, -1):
                k = i & self.buf_mask
                self.working_max = max(self.working_max, self.buffer[k])
                self.buffer[k] = self.working_max
        if self.i_back == self.i_mid_start:
            self.working_max = NEG_INF
            self.middle_max = self.front_max
            self.front_max = NEG_INF
            self.i_working = self.i_mid_end
            self.i_mid_start = self.i_mid_end
            if self.i_back == self.i_mid_start:
                self.i_back -= 1
        self.buffer[self.i_front & self.buf_mask] = NEG_INF


# ---------------------------------------------------------------------------------------------- limiter.rs
class ExponentialRelease:
    def __init__(self, release_samples):
        self.release_samples = release_samples
        self.release_slew = 1.0 / (release_samples + 1.0)
        self.output = 1.0

    def step(self, x):
        y = self.output
        r = y if x == y else fma(x - y, self.release_slew, y)  # (x == y: fma(0, slew, y) is y exactly)
        self.output = min(x, r)
        return self.output


class PerfectLimiter:
    """PerfectLimiter::with_default(sr) = new(sr, 1., 5., 15., 40.)"""

    def __init__(self, sr, threshold=1.0, attack_ms=5.0, hold_ms=15.0, release_ms=40.0):
        self.threshold = threshold
        self.attack = int(round_half_away(attack_ms * float(sr) / 1000.0))
        self.smoother = BoxStackFilter(self.attack, 3)
        self.smoother.reset(1.0)
        self.peakhold = PeakHold(hold_length_of(sr, attack_ms + hold_ms))
        self.release = ExponentialRelease(release_ms * float(sr) / 1000.0)

    def calc_gain(self, v_abs):
        raw_gain = self.threshold / (v_abs + F64_EPSILON) if v_abs > self.threshold else 1.0
        peak_holded = -self.peakhold.step(-raw_gain)
        return min(self.smoother.step(self.release.step(peak_holded)), 1.0)

    def gain_sequence(self, wavs):
        """wavs [C, n] f32 -> the f64 gains of process_inplace (before their cast to f32)"""
        v_abs = np.abs(wavs).max(axis=0).astype(np.float64).tolist() + [0.0] * self.attack
        return np.array([self.calc_gain(v) for v in v_abs][self.attack:], np.float64)


def limiter_params(sr):
    lim = PerfectLimiter(sr)
    return {"attack": lim.attack, "hold_length": lim.peakhold.hold_length(), "release_samples": lim.release.release_samples,
            "box_len": lim.smoother.lengths()}


def limit_apply(y, g):
    """y [C, n] f32 (= gain x), g [n] f64 -> f32(clamp(f64(y) g, -1, 1))"""
    return np.clip(y.astype(np.float64) * g[None, :], -1.0, 1.0).astype(F32)


# ---------------------------------------------------------------------------------------------- stats.rs
def stats_from_wav_before_clip(ch):
    peak = np.abs(ch).max() if ch.size else F32(0)
    if peak > 1:
        return db_from_amp(F32(1) / F32(peak)), int((np.abs(ch) > 1).sum())
    return F32(0), 0


def stats_from_global_gain(gain):
    return db_from_amp(F32(gain)), 0


def stats_from_gain_seq(row):
    return db_from_amp(F32(row.min())), int((row != 1).sum())


def format_stats(st):
    """Display for GuardClippingStats (stats.rs:118-132)"""
    dB, cnt = st
    if dB == 0:
        return ""
    return "%.2f dB" % dB if cnt == 0 else "max %.2f dB, total %d samples" % (dB, cnt)


# ---------------------------------------------------------------------------------------------- track.rs / audio.rs
def apply_gain(orig, sr, gain, mode):
    """AudioTrack::apply_gain on orig [C, n] f32.  -> dict: audio, drawn (channel_for_drawing), result, global_gain, gain64 (the
    limiter's f64 gains when it ran, else None), gain_seq (f32 row or None), guard_stats (as Audio::guard_clip_stats holds them)"""
    orig = np.ascontiguousarray(orig, F32)
    n_ch = orig.shape[0]
    gain = F32(gain)
    out = {"gain": gain, "result": RESULT_GLOBAL_GAIN, "global_gain": F32(1), "gain64": None, "gain_seq": None, "before_clip": None}
    if not np.isfinite(gain) or gain == 1:  # audio.clone_from(original): Audio::new's GlobalGain(1) and default stats
        out.update(gain=F32(1), audio=orig, drawn=orig, guard_stats=[(F32(0), 0)] * n_ch)
        return out
    y = gain * orig  # f32
    if mode == GUARD_CLIP:
        out.update(audio=np.clip(y, F32(-1), F32(1)), drawn=y, before_clip=y, result=RESULT_BEFORE_CLIP,
                   guard_stats=[stats_from_wav_before_clip(y[c]) for c in range(n_ch)])
    elif mode == GUARD_REDUCE_GLOBAL_LEVEL:
        peak = float(np.abs(y).max())
        if peak > 1.0:
            g = 1.0 / peak
            y = np.clip((y.astype(np.float64) * g).astype(F32), F32(-1), F32(1))
            out["global_gain"] = F32(g)
        out.update(audio=y, drawn=y, guard_stats=[stats_from_global_gain(out["global_gain"])] * n_ch)
    else:
        out["result"] = RESULT_GAIN_SEQUENCE
        if np.abs(y).max() > 1:
            g = PerfectLimiter(sr).gain_sequence(y)
            out.update(gain64=g, gain_seq=g.astype(F32), audio=limit_apply(y, g))
        else:
            out.update(gain_seq=np.ones(y.shape[1], F32), audio=y)
        out.update(drawn=out["audio"], guard_stats=[stats_from_gain_seq(out["gain_seq"])])
    return out


def select_guard_stats(guard_stats, mode):
    """format_guard_clip_stats (audio.rs:94-111): every channel's entry under Clip, else the first"""
    return list(guard_stats) if mode == GUARD_CLIP else list(guard_stats[:1])


def limiter_gain_query(res):
    """guard_clipping_gain (audio.rs:80-92)"""
    if res["result"] != RESULT_GAIN_SEQUENCE:
        return None
    return res["gain_seq"] if (res["gain_seq"] < 1).any() else np.ones(1, F32)
