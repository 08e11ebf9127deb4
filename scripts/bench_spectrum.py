"""Time th_tm_get_spectra on the bench workload in a TrackManager (128 mono tracks x 30 s x 48 kHz, win_ms 2048 / 48, t_overlap 4,
linear: T = 2813, H = 1025, row pitch 1056) against th_dev_copy of the bytes the kernel reads (tracks x T x pitch x 4), the two
alternating in one process.  Host clock: both calls end in a synchronise.  The kernels' own times come from a separate run under
rocprofv3 --kernel-trace --stats (spectrum_partial_kernel + spectrum_finish_kernel against copy_f4_kernel).
--devices 0,0 runs the same loop through a MultiTrackManager over those slots (th_tmg_get_spectra: the batch split by owner).
Usage: python scripts/bench_spectrum.py [--tracks 128] [--seconds 30] [--reps 20] [--kind 0] [--devices 0,0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thesia_amd as ta  # noqa: E402


def timed(fn, reps, warmup=0):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=128)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kind", type=int, default=ta.SPECTRUM_MEAN_AMP)
    ap.add_argument("--devices", type=lambda s: [int(d) for d in s.split(",")], default=None)
    a = ap.parse_args()
    n = int(a.seconds * a.sr)
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    with ta.Context(0) as ctx:
        tm = ta.MultiTrackManager(a.devices) if a.devices else ta.TrackManager(ctx)
        tm.set_setting(2048 / 48, 4, 1, ta.LINEAR)
        tm.add_tracks([(i, a.sr, x) for i in range(a.tracks)])
        T, H = tm.spec(0, 0).shape
        nbytes = a.tracks * T * ta.pitch_f32(H) * 4
        whole = [(i, 0, a.kind) for i in range(a.tracks)]
        second = [(i, 0, a.kind, 10.0, 11.0) for i in range(a.tracks)]
        src, dst = ctx.alloc(nbytes), ctx.alloc(nbytes)

        def copy():
            ctx.dev_copy(dst.ptr, src.ptr, nbytes)
            ctx.synchronize()

        for _ in range(3):
            tm.spectra(whole)
            copy()
        ts, cs = [], []
        for _ in range(a.reps):  # alternating: both see the same clocks
            ts += timed(lambda: tm.spectra(whole), 1)
            cs += timed(copy, 1)
        one = timed(lambda: tm.spectrum(0, 0, a.kind), a.reps, 3)
        sec = timed(lambda: tm.spectra(second), a.reps, 3)
        src.free()
        dst.free()
        tm.close()
    ms, cms = float(np.median(ts)), float(np.median(cs))
    print(json.dumps({"devices": a.devices, "tracks": a.tracks, "n_frames": T, "height": H, "kind": a.kind, "bytes_read": nbytes,
                      "get_spectra_ms_median": round(ms, 4), "get_spectra_ms_min": round(min(ts), 4),
                      "read_TBps": round(nbytes / ms / 1e9, 3), "copy_ms_median": round(cms, 4), "copy_ms_min": round(min(cs), 4),
                      "copy_TBps_read_plus_write": round(2 * nbytes / cms / 1e9, 3),
                      "one_channel_call_ms_median": round(float(np.median(one)), 4),
                      "one_second_range_all_tracks_ms_median": round(float(np.median(sec)), 4)}))


if __name__ == "__main__":
    main()
