"""Measure the band-limited export (th_tm_export_pcm_band) on 64 stereo tracks x 30 s at 48 kHz, in one run:
  kernel        scripts/ubench/band_ab (a child process per row length; built here when missing): the band kernel, compiled from the
                product's source, at 2K = 512, 4096 and 65536, beside the resample kernel driven with the same row at L = M = 1 on the
                same data, both timed by hipEvents, bit-identical outputs checked; multiply-adds per second against the 157 TFLOP/s f32
                vector peak
  end_to_end    the whole call into pinned host memory (th_host_alloc) at 2K = 4096, median of --reps after warm-up, for F32 and S16
                TPDF, beside th_tm_export_pcm of the same audio in the same format (no filter: the yardstick)
  cpu_route     what a host did before this entry existed, on ONE 30 s stereo track: th_tm_copy_audio per channel, then an FFT
                convolution with the same f32 row in numpy (f64), one thread per channel; cpu_route_64_tracks_16_threads_ms scales the
                per-channel time to 128 channels on 16 threads
Writes the result as JSON to --out (profiles/band_bench.txt) and prints it.  Kernel: windows of back-to-back launches of 25 ms or
more, median of 7 (3 for the longest row, whose single launch is 0.3 - 1.1 s); end to end: 3 warm-up calls, median of --reps.
Usage: python scripts/bench_band.py [--tracks 64] [--seconds 30] [--reps 10] [--half-taps 256,2048,32768] [--no-kernel] [--out FILE]"""
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

AB_SRC = os.path.join(ROOT, "scripts", "ubench", "band_ab.hip")
AB_EXE = os.path.join(ROOT, "scripts", "ubench", "band_ab")
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
SR = 48000


def build_ab():
    deps = [AB_SRC] + [os.path.join(CSRC, f) for f in ("kernels_band.hip", "band_block.h", "kernels_resample.hip", "resample_block.h",
                                                       "resample_core.h", "kernels.h", "reader_plan.h")]
    if os.path.exists(AB_EXE) and all(os.path.getmtime(d) <= os.path.getmtime(AB_EXE) for d in deps):
        return
    lib_dir = os.path.join(ROOT, "thesia_amd")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", AB_SRC,
                           "-L" + lib_dir, "-lthesia_amd", "-Wl,-rpath," + lib_dir, "-o", AB_EXE])


def cpu_route(tm, tid, row):
    K = row.size // 2
    t0 = time.perf_counter()
    chans = [tm.audio(tid, c) for c in range(2)]
    t1 = time.perf_counter()

    def one(x):
        n = x.size + row.size - 1
        nfft = 1 << (n - 1).bit_length()
        # y[j] = sum over k of c[k] x[j - K + 1 + k] is sample j + K of the convolution of x with the reversed row
        z = np.fft.irfft(np.fft.rfft(x.astype(np.float64), nfft) * np.fft.rfft(row[::-1].astype(np.float64), nfft), nfft)
        return z[K: K + x.size].astype(np.float32)

    with ThreadPoolExecutor(2) as pool:
        ys = list(pool.map(one, chans))
    t2 = time.perf_counter()
    return ys, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_bench.txt"))
    ap.add_argument("--half-taps", default="256,2048,32768")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    res = {"tracks": a.tracks, "channels": 2, "seconds": a.seconds, "sr": SR, "kernel": {}}
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    if not a.no_kernel:
        build_ab()
        for K in [int(v) for v in a.half_taps.split(",")]:
            out = subprocess.run([AB_EXE, str(K), str(a.seconds), str(a.tracks), str(7 if K < 16384 else 3)], capture_output=True, text=True)
            if out.returncode != 0:  # (a fault in the child ends the measurement: nothing more is started on the card)
                print(json.dumps({"error": "band_ab failed", "half_taps": K, "rc": out.returncode, "stdout": out.stdout[-600:], "stderr": out.stderr[-400:]}))
                sys.exit(1)
            res["kernel"]["2K=%d" % (2 * K)] = json.loads(out.stdout.strip().splitlines()[-1])
    rng = np.random.default_rng(0)
    K = 2048
    bd = (ta.BAND_PASS, 200.0, 8000.0, 0.0)  # (trans_hz 0: the default 2K = 4096)
    plan = ta.band_plan(SR, *bd)
    assert plan["half_taps"] == K
    row = ta.band_coefs(SR, plan)[1]
    with ta.Context(0) as ctx:
        n = int(a.seconds * SR)
        x = rng.uniform(-0.9, 0.9, (2, n)).astype(np.float32)
        ids = list(range(a.tracks))
        tm = ta.TrackManager(ctx)
        tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
        tm.add_tracks([(i, SR, x) for i in ids])
        cap = n * 2 * a.tracks * 4 + 16 * a.tracks
        pin = C.c_void_p()
        _ffi.check(_ffi.lib.th_host_alloc(ctx.handle, cap, C.byref(pin)))
        pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(cap,))
        e2e = {}
        for name, fmt, dith in (("f32", api.PCM_F32, api.DITHER_NONE), ("s16_tpdf", api.PCM_S16, api.DITHER_TPDF)):
            calls = {"export_pcm_band_ms": lambda: tm.export_pcm_band([(i,) + bd + (fmt, dith, 1) for i in ids], out=pinned),
                     "export_pcm_ms": lambda: tm.export_pcm([(i, fmt, dith, 1) for i in ids], out=pinned)}
            e = {}
            for label, fn in calls.items():
                for _ in range(3):
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
        res["end_to_end_2K=4096"] = e2e
        ys, copy_ms, fft_ms = cpu_route(tm, 0, row)
        out, infos = tm.export_pcm_band([(0,) + bd + (api.PCM_F32,)])
        got = out.view(np.float32).reshape(-1, 2).T
        res["cpu_route_2K=4096"] = {"copy_audio_ms": round(copy_ms, 2), "fft_convolution_2_channels_2_threads_ms": round(fft_ms, 1),
                                    "cpu_route_64_tracks_16_threads_ms": round(copy_ms * a.tracks + fft_ms * (2 * a.tracks) / 16.0, 1),
                                    "max_abs_difference_from_the_gpu_export": float(max(np.abs(got[c] - ys[c]).max() for c in range(2)))}
        _ffi.check(_ffi.lib.th_host_free(ctx.handle, pin))
        tm.close()
    text = json.dumps(res, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
