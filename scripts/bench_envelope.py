"""Time th_tm_get_envelopes on one 30 min x 48 kHz mono track and write profiles/envelope_bench.txt:
  a  one 1800-column overview of the whole track
  b  128 such requests (ranges that start 10 ms apart) in ONE call and as 128 single calls
  c  the tile route for a's pixels, as the parent commit would do it: every 1024-bin tile of the finest pyramid level whose bins are no
     longer than a column (th_tm_get_waveform_tile), re-binned on the host to the 1800 columns (min of minima, max of maxima, mean
     of means: not exact); once, and 128 times
  d  one 1800 x 200 waveform lane of the whole track (th_tm_render_waveform_figures)
Per workload, by the host's clock (median of --reps after warm-up).  The yardstick, which is not the code under test: th_dev_copy (the
library's 16-byte-per-lane copy kernel) over as many bytes as the reduction reads (the whole channel).
Kernel times are not visible from outside the library: they come from a run of their own,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_envelope.py --profile
(--profile runs a's call and its copy --reps times each, nothing else), and `--kernel-stats DIR` reads DIR/**/*kernel_stats.csv into
the report: envelope_reduce_kernel and envelope_columns_kernel beside copy_f4_kernel of the same run.
Usage: python scripts/bench_envelope.py [--reps 20] [--minutes 30] [--requests 128] [--profile] [--kernel-stats DIR] [--out FILE]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import thesia_amd as ta  # noqa: E402
from thesia_amd import _ffi, api  # noqa: E402

INF = float("inf")
W = 1800


def noise(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float32) / 48000.0
    return (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * rng.uniform(-1, 1, n)).astype(np.float32)


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def envelope_call(tm, reqs):
    """the C call alone: the request array, the infos and the output are made once"""
    n = len(reqs)
    arr = (_ffi.EnvelopeRequest * n)(*[api._envelope_request(r) for r in reqs])
    info, need = (_ffi.EnvelopeInfo * n)(), C.c_size_t()
    out = np.empty(sum(4 * r[5] for r in reqs), np.float32)
    p = out.ctypes.data_as(_ffi.c_f32p)
    return (lambda: _ffi.check(_ffi.lib.th_tm_get_envelopes(tm.handle, arr, n, p, out.size, info, C.byref(need)))), out


def tile_route(tm, n, level, edges):
    """the covering tiles of `level`, re-binned to the columns of `edges` on the host"""
    bins = -(-n // (1 << level))
    tiles = [np.frombuffer(tm.get_waveform_tile(0, 0, level, t), np.float32, offset=24).reshape(-1, 3) for t in range(-(-bins // 1024))]
    b = np.concatenate(tiles)[:bins]
    first = np.minimum(edges[:-1] >> level, bins - 1).astype(np.int64)   # the bin that holds a column's first sample
    return np.stack([np.minimum.reduceat(b[:, 0], first), np.maximum.reduceat(b[:, 1], first), np.add.reduceat(b[:, 2], first)], 1), len(tiles)


def kernel_stats(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    rows = {}
    if files:
        for r in csv.DictReader(open(files[-1])):
            for k in ("envelope_reduce_kernel", "envelope_columns_kernel", "copy_f4_kernel"):
                if k in r.get("Name", ""):
                    rows[k] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                               "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        if "envelope_reduce_kernel" in rows and "copy_f4_kernel" in rows:
            rows["reduce_over_copy"] = round(rows["envelope_reduce_kernel"]["avg_us"] / rows["copy_f4_kernel"]["avg_us"], 2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--requests", type=int, default=128)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope_bench.txt"))
    a = ap.parse_args()
    n = int(a.minutes * 60 * 48000)
    res = {}
    with ta.Context(0) as ctx:
        tm = ta.TrackManager(ctx)
        tm.add_tracks([(0, 48000, noise(n, 1)[None])])
        tm.apply_track_list_changes()
        one, out1 = envelope_call(tm, [(0, 0, 1, 0.0, INF, W)])
        src, dst = ctx.alloc(n * 4), ctx.alloc(n * 4)

        def copy():
            ctx.dev_copy(dst.ptr, src.ptr, n * 4)
            ctx.synchronize()

        if a.profile:
            for _ in range(a.reps + 2):
                one()
                copy()
            print(json.dumps({"profiled_calls": a.reps + 2}))
            tm.close()
            return
        res["a"] = {"samples": n, "columns": W, "call": timed(one, a.reps), "bytes_read": n * 4, "copy": timed(copy, a.reps)}
        reqs = [(0, 0, 1, 0.01 * i, INF, W) for i in range(a.requests)]
        batch, outb = envelope_call(tm, reqs)
        singles = [envelope_call(tm, [r])[0] for r in reqs]

        def all_singles():
            for f in singles:
                f()

        res["b"] = {"requests": a.requests, "one_call": timed(batch, max(a.reps // 4, 3)), "single_calls": timed(all_singles, max(a.reps // 4, 3)),
                    "bytes_read": sum(int(e[-1] - e[0]) * 4 for e in (ta.envelope_edges(48000, n, r[3], r[4], W) for r in reqs))}
        edges = ta.envelope_edges(48000, n, 0.0, INF, W)
        level = max(int(np.floor(np.log2(n / W))), 0)
        got, n_tiles = tile_route(tm, n, level, edges)
        one()
        exact = out1.reshape(-1, 4)
        res["c"] = {"level": level, "tiles": n_tiles, "tile_bytes": n_tiles * (24 + 12 * 1024), "once": timed(lambda: tile_route(tm, n, level, edges), a.reps),
                    "times_%d" % a.requests: timed(lambda: [tile_route(tm, n, level, edges) for _ in range(a.requests)], 3),
                    "columns_whose_min_or_max_differs_from_exact": int(((got[:, 0] != exact[:, 0]) | (got[:, 1] != exact[:, 1])).sum())}
        lane = (0, 0, 1, 0.0, INF, W, 200, -1.0, 1.0, 256, (255, 255, 255, 255), (0, 0, 0, 255))
        buf = np.empty(W * 200 * 4, np.uint8)
        res["d"] = {"size": [W, 200], "call": timed(lambda: tm.render_waveform_figures([lane], out=buf), a.reps)}
        src.free()
        dst.free()
        tm.close()
    if a.kernel_stats:
        res["kernels_a"] = kernel_stats(a.kernel_stats)
    lines = ["# scripts/bench_envelope.py: th_tm_get_envelopes, one MI355X, one %.0f min x 48 kHz mono track; host clock = median of %d calls;" % (a.minutes, a.reps),
             "# kernels = rocprofv3 --kernel-trace --stats, a run of its own (average per launch); copy = th_dev_copy over the channel's bytes, same run",
             "# a: one %d-column overview; b: %d such requests in one call / as single calls; c: the tile route for a's pixels; d: a %d x 200 lane" % (W, a.requests, W)]
    for k in sorted(res):
        lines.append("%s %s" % (k, json.dumps(res[k])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
