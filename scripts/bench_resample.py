"""Measure the export at a target sample rate (th_tm_export_pcm_at) on 64 stereo tracks x 30 s, for 44.1 -> 48, 48 -> 44.1, 48 -> 96
and 96 -> 48 kHz, in one run:
  kernel        scripts/ubench/resample_ab (a child process per pair; built here when missing): the tiled resample kernel, compiled from
                the product's source, beside the naive one-thread-per-output form of the same contract on the same data, both timed by
                hipEvents, bit-identical outputs checked; multiply-adds per second against the 157 TFLOP/s f32 vector peak and the
                algorithmic bytes against the 8 TB/s roofline
  end_to_end    the whole call into pinned host memory (th_host_alloc), median of --reps after warm-up, for F32 and S16 TPDF, beside
                th_tm_export_pcm of the same audio in the same format (no resampling: the yardstick)
  cpu_route     what a host did before this entry existed, on ONE 30 s stereo track: th_tm_copy_audio per channel, then
                scipy.signal.resample_poly with the same windowed sinc (the prototype on the 1 / L grid, 2 K L + 1 taps), one thread per
                channel; cpu_route_64_tracks_16_threads_ms scales the per-channel time to 128 channels on 16 threads
The product kernel's own time comes from a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bench_resample.py --profile
(--profile: the F32 call --reps times per pair, nothing else; read resample_kernel in the kernel stats).
Usage: python scripts/bench_resample.py [--tracks 64] [--seconds 30] [--reps 5] [--pairs 44100:48000,...] [--profile] [--no-kernel]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import thesia_amd as ta  # noqa: E402
from thesia_amd import _ffi, api  # noqa: E402

AB_SRC = os.path.join(ROOT, "scripts", "ubench", "resample_ab.hip")
AB_EXE = os.path.join(ROOT, "scripts", "ubench", "resample_ab")
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")


def build_ab():
    deps = [AB_SRC] + [os.path.join(CSRC, f) for f in ("kernels_resample.hip", "resample_block.h", "resample_core.h", "kernels.h", "reader_plan.h")]
    if os.path.exists(AB_EXE) and all(os.path.getmtime(d) <= os.path.getmtime(AB_EXE) for d in deps):
        return
    lib_dir = os.path.join(ROOT, "thesia_amd")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", AB_SRC,
                           "-L" + lib_dir, "-lthesia_amd", "-Wl,-rpath," + lib_dir, "-o", AB_EXE])


def cpu_route(tm, tid, sr_in, sr_out):
    from scipy.signal import resample_poly
    from tests import resample_ref as R
    p = R.plan(sr_in, sr_out)
    L, M, K = p["L"], p["M"], p["K"]
    h = R.proto(p, np.arange(-K * L, K * L + 1) / L) / L  # the same kernel on the 1 / L grid (resample_poly multiplies its filter by L)
    t0 = time.perf_counter()
    chans = [tm.audio(tid, c) for c in range(2)]
    t1 = time.perf_counter()
    with ThreadPoolExecutor(2) as pool:
        ys = list(pool.map(lambda x: resample_poly(x.astype(np.float64), L, M, window=h).astype(np.float32), chans))
    t2 = time.perf_counter()
    return chans, ys, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", default="44100:48000,48000:44100,48000:96000,96000:48000")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    pairs = [tuple(int(v) for v in p.split(":")) for p in a.pairs.split(",")]
    res = {"tracks": a.tracks, "channels": 2, "seconds": a.seconds, "pairs": {}}
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    if not a.profile and not a.no_kernel:
        build_ab()
        for sr_in, sr_out in pairs:
            out = subprocess.run([AB_EXE, str(sr_in), str(sr_out), str(a.seconds), str(a.tracks), str(a.reps)], capture_output=True, text=True)
            if out.returncode != 0:  # (a fault in the child ends the measurement: nothing more is started on the card)
                print(json.dumps({"error": "resample_ab failed", "pair": [sr_in, sr_out], "rc": out.returncode, "stderr": out.stderr[-400:]}))
                sys.exit(1)
            res["pairs"]["%d:%d" % (sr_in, sr_out)] = {"kernel": json.loads(out.stdout.strip().splitlines()[-1])}
    rng = np.random.default_rng(0)
    with ta.Context(0) as ctx:
        for sr_in in sorted({p[0] for p in pairs}):
            n = int(a.seconds * sr_in)
            x = rng.uniform(-0.9, 0.9, (2, n)).astype(np.float32)
            ids = list(range(a.tracks))
            tm = ta.TrackManager(ctx)
            tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
            tm.add_tracks([(i, sr_in, x) for i in ids])
            for _, sr_out in [p for p in pairs if p[0] == sr_in]:
                r = res["pairs"].setdefault("%d:%d" % (sr_in, sr_out), {})
                n_out = ta.resample_n_out(n, sr_in, sr_out)
                cap = max(n, n_out) * 2 * a.tracks * 4 + 16 * a.tracks
                pin = C.c_void_p()
                _ffi.check(_ffi.lib.th_host_alloc(ctx.handle, cap, C.byref(pin)))
                pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(cap,))
                e2e = {}
                for name, fmt, dith in (("f32", api.PCM_F32, api.DITHER_NONE),) + (() if a.profile else (("s16_tpdf", api.PCM_S16, api.DITHER_TPDF),)):
                    calls = {"export_pcm_at_ms": lambda: tm.export_pcm_at([(i, sr_out, fmt, dith, 1) for i in ids], out=pinned)}
                    if not a.profile:
                        calls["export_pcm_ms"] = lambda: tm.export_pcm([(i, fmt, dith, 1) for i in ids], out=pinned)
                    e = {}
                    for label, fn in calls.items():
                        fn()
                        ts = []
                        for _ in range(a.reps):
                            t0 = time.perf_counter()
                            out, infos = fn()
                            ts.append((time.perf_counter() - t0) * 1e3)
                        e[label] = med(ts)
                        e[label.replace("_ms", "_min_ms")] = round(min(ts), 3)
                        e[label.replace("_ms", "_out_bytes")] = int(out.size)
                    e2e[name] = e
                r["end_to_end"] = e2e
                if not a.profile:
                    chans, ys, copy_ms, poly_ms = cpu_route(tm, 0, sr_in, sr_out)
                    out, infos = tm.export_pcm_at([(0, sr_out, api.PCM_F32)])
                    got = out.view(np.float32).reshape(-1, 2).T
                    m = min(got.shape[1], ys[0].size)
                    r["cpu_route"] = {"copy_audio_ms": round(copy_ms, 2), "resample_poly_2_channels_2_threads_ms": round(poly_ms, 1),
                                      "cpu_route_64_tracks_16_threads_ms": round(copy_ms * a.tracks + poly_ms * (2 * a.tracks) / 16.0, 1),
                                      "max_abs_difference_from_the_gpu_export": float(max(np.abs(got[c, :m] - ys[c][:m]).max() for c in range(2)))}
                _ffi.check(_ffi.lib.th_host_free(ctx.handle, pin))
            tm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
