"""Time th_tm_get_loudness_meters on the bench workload (128 tracks x 30 s x 48 kHz mono: 184 M samples, 737 MB) in one process:
the getter's wall time (median of --reps after warm-up), beside it th_audio_stats_dev and th_dev_copy of the same bytes.  The
per-kernel times come from a run of this script under `rocprofv3 --kernel-trace --stats -- python scripts/bench_loudness_meter.py`
(true_peak_kernel against loudness_zero_state_kernel, pass A, on the same audio in the same run).
--devices 0,0 runs the getter's loop through a MultiTrackManager over those slots (th_tmg_get_loudness_meters: the batch split by owner).
Usage: python scripts/bench_loudness_meter.py [--tracks 128] [--seconds 30] [--reps 20] [--devices 0,0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thesia_amd as ta  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--devices", type=lambda s: [int(d) for d in s.split(",")], default=None)
    a = ap.parse_args()
    n = int(a.seconds * a.sr)
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    nbytes = n * 4 * a.tracks
    ids = list(range(a.tracks))
    with ta.Context(0) as ctx:
        tm = ta.MultiTrackManager(a.devices) if a.devices else ta.TrackManager(ctx)
        tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
        tm.add_tracks([(i, a.sr, x) for i in ids])
        for _ in range(3):
            tm.loudness_meters(ids, series=False)
        ts, ts_series = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            tm.loudness_meters(ids, series=False)
            ts.append((time.perf_counter() - t0) * 1e3)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m = tm.loudness_meters(ids)
            ts_series.append((time.perf_counter() - t0) * 1e3)
        # the same bytes through th_audio_stats_dev (passes A - D) and th_dev_copy (read + write)
        bufs = [ctx.to_device(x) for _ in range(a.tracks)]
        tracks = [([b.ptr], n, a.sr, 0) for b in bufs]
        for _ in range(3):
            ctx.audio_stats_dev(tracks)
        ss = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.audio_stats_dev(tracks)
            ss.append((time.perf_counter() - t0) * 1e3)
        src, dst = ctx.alloc(nbytes), ctx.alloc(nbytes)
        ctx.dev_copy(dst.ptr, src.ptr, nbytes)
        ctx.synchronize()
        cs = []
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.dev_copy(dst.ptr, src.ptr, nbytes)
            ctx.synchronize()
            cs.append((time.perf_counter() - t0) * 1e3)
        for b in bufs + [src, dst]:
            b.free()
        tm.close()
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    print(json.dumps({"devices": a.devices, "tracks": a.tracks, "samples": n * a.tracks, "bytes": nbytes, "meters_ms_median": med(ts), "meters_ms_min": round(min(ts), 4),
                      "meters_with_series_ms_median": med(ts_series), "series_doubles": int(sum(d["n_momentary"] + d["n_short_term"] for d in m)),
                      "true_peak_dB": float(m[0]["true_peak_dB"]), "loudness_range": m[0]["loudness_range"],
                      "audio_stats_ms_median": med(ss), "copy_ms": med(cs), "copy_TBps": round(2 * nbytes / float(np.median(cs)) / 1e9, 3),
                      "true_peak_flop": 72 * n * a.tracks}))


if __name__ == "__main__":
    main()
