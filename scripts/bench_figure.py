"""Time th_tm_render_figures on three workloads and write profiles/figure_bench.txt:
  a  one 30 min x 48 kHz channel at the default setting, the whole image as one 2000 x 800 RGBA figure (an overview: ~90 : 1)
  b  128 channels x 30 s, one 1024 x 256 RGBA figure of each whole image, as ONE call and as 128 single calls
  c  one 512 x 512 figure with the crop box of a LOD (3, 1) tile of a's image
Per workload, by the host's clock (median of --reps after warm-up, pinned output): the call; the yardsticks, which are not the code
under test: th_dev_copy (the library's 16-byte-per-lane copy kernel) over as many bytes as the source rows the horizontal pass must
read, and the parent's per-request tile route (th_tm_get_spectrogram_tile(s) under set_lod_source(1)) for c's box and for the tiles of
the level a viewer would fetch to cover b's figures (floor(log2(T / 1024)) in x, 0 in y).
Kernel times are not visible from outside the library: they come from a run of their own per workload,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/a -- python scripts/bench_figure.py --profile a      (likewise b, c)
(--profile runs the workload's call and its copy --reps times, nothing else), and `--kernel-stats DIR` reads DIR/{a,b,c}/**/*kernel_stats.csv
into the report: figure_hpass_kernel and figure_vpass_kernel (per launch, and per call: a call launches each once per piece) beside
copy_f4_kernel, and the horizontal kernel's time per call as a multiple of the copy.
Usage: python scripts/bench_figure.py [--reps 20] [--minutes 30] [--channels 128] [--profile a|b|c] [--kernel-stats DIR] [--out FILE]"""
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
from thesia_amd import _ffi  # noqa: E402

RGBA = ta.FIGURE_RGBA


def noise(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float32) / 48000.0
    return (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * rng.uniform(-1, 1, n)).astype(np.float32)


def rows_read(h, box_top, box_h, out_h):
    """source rows the vertical windows of the whole figure span"""
    s, c, _ = ta.figure_axis(box_top, box_h, out_h, h)
    return int((s + c).max() - s.min())


def timed(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def tile_box(W, Hh, lx, ly, tx, ty):
    lod_w, lod_h = -(-W // (1 << lx)), -(-Hh // (1 << ly))
    sx, sy = tx * 512, ty * 512
    cw, ch = min(max(lod_w - sx, 0), 512), min(max(lod_h - sy, 0), 512)
    ox, oy = max(sx - 4, 0), max(sy - 4, 0)
    w, h = min(lod_w, sx + cw + 4) - ox, min(lod_h, sy + ch + 4) - oy
    left, top = ox * W / lod_w, oy * Hh / lod_h
    return (left, top, (ox + w) * W / lod_w - left, (oy + h) * Hh / lod_h - top), w, h


class Pinned:
    def __init__(self, ctx, cap):
        self.ctx, self.cap, self.p = ctx, cap, C.c_void_p()
        _ffi.check(_ffi.lib.th_host_alloc(ctx.handle, cap, C.byref(self.p)))

    def free(self):
        _ffi.check(_ffi.lib.th_host_free(self.ctx.handle, self.p))


def copy_yardstick(ctx, nbytes, reps, profile):
    nbytes = max(nbytes // 16 * 16, 16)
    src, dst = ctx.alloc(nbytes), ctx.alloc(nbytes)

    def fn():
        ctx.dev_copy(dst.ptr, src.ptr, nbytes)
        ctx.synchronize()

    if profile:
        for _ in range(reps):
            fn()
        r = {}
    else:
        r = timed(fn, reps)
    src.free()
    dst.free()
    return dict(r, bytes=nbytes)


def workload_a_c(ctx, a, which, profile):
    n = int(a.minutes * 60 * 48000)
    tm = ta.TrackManager(ctx)
    tm.add_tracks([(0, 48000, noise(n, 1)[None])])
    tm.apply_track_list_changes()
    Hh, W = tm.img(0, 0).shape
    res = {"image": [Hh, W]}
    if which == "a":
        req = (0, 0, RGBA, 2000, 800, (0.0, 0.0, float(W), float(Hh)))
        rows = rows_read(Hh, 0.0, float(Hh), 800)
    else:
        lod_w = -(-W // 8)
        box, w, h = tile_box(W, Hh, 3, 1, (lod_w // 512) // 2, 0)
        req = (0, 0, RGBA, w, h, box)
        rows = rows_read(Hh, box[1], box[3], h)
        res["tile"] = [3, 1, (lod_w // 512) // 2, 0, w, h]
    pin = Pinned(ctx, req[3] * req[4] * 4 + 64)
    call = lambda: tm.render_figures([req], out=pin.p, cap=pin.cap)  # noqa: E731
    cols = W if which == "a" else int(np.ceil(req[5][2])) + 48
    if profile:
        for _ in range(a.reps + 2):
            call()
    else:
        res["call"] = timed(call, a.reps)
    res["source_bytes"] = rows * cols * 2
    res["copy"] = copy_yardstick(ctx, rows * cols * 2, a.reps, profile)
    if which == "c" and not profile:
        tm.set_lod_source(True)
        t = res["tile"]
        res["parent_tile_route"] = timed(lambda: tm.get_spectrogram_tile(0, 0, t[0], t[1], t[2], t[3]), a.reps)
        tile = tm.get_spectrogram_tile(0, 0, t[0], t[1], t[2], t[3])
        fig, _ = tm.render_figures([req])
        res["equals_parent_tile"] = bool(np.array_equal(np.frombuffer(tile[40:], np.uint8), fig[0].ravel()))
        tm.set_lod_source(False)
    pin.free()
    tm.close()
    return res


def workload_b(ctx, a, profile):
    n = 30 * 48000
    tm = ta.TrackManager(ctx)
    x = noise(n, 2)
    tm.add_tracks([(i, 48000, np.roll(x, 997 * i)[None]) for i in range(a.channels)])
    tm.apply_track_list_changes()
    Hh, W = tm.img(0, 0).shape
    reqs = [(i, 0, RGBA, 1024, 256, (0.0, 0.0, float(W), float(Hh))) for i in range(a.channels)]
    pin = Pinned(ctx, a.channels * 1024 * 256 * 4 + 64)
    one = lambda: tm.render_figures(reqs, out=pin.p, cap=pin.cap)  # noqa: E731

    def singles():
        for r in reqs:
            tm.render_figures([r], out=pin.p, cap=pin.cap)

    res = {"image": [Hh, W], "channels": a.channels}
    rows = rows_read(Hh, 0.0, float(Hh), 256)
    if profile:
        for _ in range(a.reps + 2):
            one()
    else:
        res["one_call"] = timed(one, a.reps)
        res["single_calls"] = timed(singles, max(a.reps // 4, 3))
        lx = max(int(np.floor(np.log2(W / 1024))), 0)
        tiles = [(i, 0, lx, 0, tx, 0) for i in range(a.channels) for tx in range(-(-(-(-W // (1 << lx))) // 512))]
        tm.set_lod_source(True)
        res["parent_tiles"] = dict(timed(lambda: tm.get_spectrogram_tiles(tiles, pinned=True), max(a.reps // 4, 3)), level=[lx, 0], n_tiles=len(tiles))
        tm.set_lod_source(False)
    res["source_bytes"] = rows * W * 2 * a.channels
    res["copy"] = copy_yardstick(ctx, rows * W * 2 * a.channels, a.reps, profile)
    pin.free()
    tm.close()
    return res


def kernel_stats(d, n_calls):
    out = {}
    for w in "abc":
        files = sorted(glob.glob(os.path.join(d, w, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
        if not files:
            continue
        rows = {}
        for r in csv.DictReader(open(files[-1])):
            name = r.get("Name", "")
            for k in ("figure_hpass_kernel", "figure_vpass_kernel", "copy_f4_kernel"):
                if k in name:
                    rows[k] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                               "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        # a call launches each kernel once per piece: the kernels' time per CALL against one copy of the call's source bytes
        if "figure_hpass_kernel" in rows and "copy_f4_kernel" in rows:
            for k in ("figure_hpass_kernel", "figure_vpass_kernel"):
                rows[k]["launches_per_call"] = round(rows[k]["calls"] / n_calls, 2)
                rows[k]["per_call_us"] = round(rows[k]["avg_us"] * rows[k]["calls"] / n_calls, 2)
            rows["hpass_over_copy"] = round(rows["figure_hpass_kernel"]["per_call_us"] / rows["copy_f4_kernel"]["avg_us"], 2)
        out[w] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--profile", choices=["a", "b", "c"])
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "figure_bench.txt"))
    a = ap.parse_args()
    res = {}
    with ta.Context(0) as ctx:
        for w in ([a.profile] if a.profile else ["a", "b", "c"]):
            res[w] = workload_b(ctx, a, bool(a.profile)) if w == "b" else workload_a_c(ctx, a, w, bool(a.profile))
    if a.profile:
        print(json.dumps(res))
        return
    if a.kernel_stats:
        res["kernels"] = kernel_stats(a.kernel_stats, a.reps + 2)  # (--profile: two warm-up calls, then --reps)
    lines = ["# scripts/bench_figure.py: th_tm_render_figures, one MI355X; host clock = median of %d calls into pinned memory;" % a.reps,
             "# kernels = rocprofv3 --kernel-trace --stats, one run per workload (average per launch); copy = th_dev_copy over the source bytes",
             "# a: %.0f min x 48 kHz, whole image -> 2000 x 800; b: %d channels x 30 s -> 1024 x 256 each; c: the box of a LOD (3, 1) tile of a -> 512 x 512"
             % (a.minutes, a.channels)]
    for w in "abc":
        lines.append("%s %s" % (w, json.dumps(res[w])))
    if "kernels" in res:
        for w, k in res["kernels"].items():
            lines.append("kernels_%s %s" % (w, json.dumps(k)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
