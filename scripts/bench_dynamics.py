"""Time th_tm_set_common_guard_clipping for each mode on the bench workload (128 tracks x 30 s x 48 kHz mono, normalised by +12 dB so
that every guard acts), beside th_dev_copy of the same bytes and the loudness passes (th_audio_stats_dev) on the same audio.  A setter
re-derives every track's audio and then recomputes pyramids, stats, specs and images, so its wall time is reported next to the same
setter with nothing to derive (target Off) and to th_tm_set_setting (STFT and images alone).  The kernels' own times come from a trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/bench_dynamics.py --reps 1
lists dyn_apply_kernel and the lim_* kernels by stage.
Usage: python scripts/bench_dynamics.py [--tracks 128] [--seconds 30] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thesia_amd as ta  # noqa: E402
from thesia_amd.api import GUARD_CLIP, GUARD_LIMITER, GUARD_REDUCE_GLOBAL_LEVEL, NORM_OFF, NORM_RMS_DB  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), round(min(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = int(a.seconds * a.sr)
    x = np.random.default_rng(0).uniform(-0.5, 0.5, n).astype(np.float32)
    nbytes = n * 4 * a.tracks
    out = {"tracks": a.tracks, "samples": n * a.tracks, "bytes": nbytes}
    with ta.Context(0) as ctx:
        tm = ta.TrackManager(ctx)
        tm.add_tracks([(i, a.sr, x) for i in range(a.tracks)])
        tm.apply_track_list_changes()
        target = float(np.float32(tm.audio_stats(0)["rms_dB"] + 12.0))
        tm.set_common_normalize(NORM_RMS_DB, target)  # (under the default guard, ReduceGlobalLevel)
        out["gain_dB"] = round(20 * float(np.log10(tm.track_dynamics(0)["normalize_gain"])), 3)
        modes = (("clip", GUARD_CLIP), ("reduce_global_level", GUARD_REDUCE_GLOBAL_LEVEL), ("limiter", GUARD_LIMITER))
        for name, mode in modes:  # warm-up: every kernel of every mode once
            tm.set_common_guard_clipping(mode)
        for name, mode in modes:
            out["set_guard_%s_ms" % name] = timed(lambda: tm.set_common_guard_clipping(mode), a.reps)
        out["limiter_reduction"] = [float(tm.guard_clip_stats(0)[0][0]), int(tm.guard_clip_stats(0)[0][1])]
        # the same setter with nothing to derive (every track is and stays its original): specs untouched, images re-made
        tm.set_common_normalize(NORM_OFF, 0.0)
        out["set_guard_off_target_ms"] = timed(lambda: tm.set_common_guard_clipping(GUARD_LIMITER), a.reps)
        # the STFT, pyramids, stats and images of the setter without the guard: set_setting to the setting in force
        out["set_setting_ms"] = timed(lambda: tm.set_setting(40.0, 4, 1, ta.MEL), a.reps)
        tm.close()
        # yardsticks on the same card in the same run: the loudness passes and a device copy of the same bytes
        bufs = [ctx.to_device(x) for _ in range(a.tracks)]
        tracks = [([b.ptr], n, a.sr, 0) for b in bufs]
        ctx.audio_stats_dev(tracks)
        out["audio_stats_ms"] = timed(lambda: ctx.audio_stats_dev(tracks), a.reps)
        src, dst = ctx.alloc(nbytes), ctx.alloc(nbytes)

        def copy():
            ctx.dev_copy(dst.ptr, src.ptr, nbytes)
            ctx.synchronize()
        copy()
        out["copy_ms"] = timed(copy, a.reps)
        for b in bufs + [src, dst]:
            b.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
