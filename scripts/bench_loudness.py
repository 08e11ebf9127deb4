"""Time th_audio_stats_dev on the bench workload (128 tracks x 30 s x 48 kHz mono: 184 M samples, 737 MB) and report the read
bandwidth against th_dev_copy's rate on the same card.  Usage: python scripts/bench_loudness.py [--tracks 128] [--seconds 30] [--reps 20]"""
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
    a = ap.parse_args()
    n = int(a.seconds * a.sr)
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    with ta.Context(0) as ctx:
        bufs = [ctx.to_device(x) for _ in range(a.tracks)]
        tracks = [([b.ptr], n, a.sr, 0) for b in bufs]
        for _ in range(3):
            ctx.audio_stats_dev(tracks)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.audio_stats_dev(tracks)
            ts.append((time.perf_counter() - t0) * 1e3)
        # copy yardstick: th_dev_copy of the same bytes (read + write), timed with the context's events
        nbytes = n * 4 * a.tracks
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
    ms, cms = float(np.median(ts)), float(np.median(cs))
    print(json.dumps({"tracks": a.tracks, "samples": n * a.tracks, "bytes": nbytes, "audio_stats_ms_median": round(ms, 4),
                      "audio_stats_ms_min": round(min(ts), 4), "read_TBps_one_pass": round(nbytes / ms / 1e9, 3),
                      "copy_ms": round(cms, 4), "copy_TBps": round(2 * nbytes / cms / 1e9, 3)}))


if __name__ == "__main__":
    main()
