"""Time th_tm_export_pcm on the bench line's audio (128 tracks x 30 s x 48 kHz, taken as 64 stereo tracks) in one process, for
S16 TPDF, S24 TPDF and F32:
  call_pinned_ms    the whole call into pinned host memory (th_host_alloc), median of --reps after warm-up
  call_pageable_ms  the same into an ordinary numpy array
  parent_route_ms   what a host did before this entry existed: th_tm_copy_audio per channel, then the numpy restatement's quantise
                    and interleave (tests/export_ref.py); measured on --parent-tracks tracks and scaled to all of them
  d2d_copy_ms       a device-to-device hipMemcpyAsync that reads and writes as many bytes as the kernel does together (a copy of
                    (read + written) / 2 bytes), and copy_kernel_ms, the same through th_dev_copy (the library's 16-byte-per-lane
                    copy kernel): the yardsticks, not the code under test
The kernel time alone is not visible from outside the library: it comes from a run of this script under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_export.py --profile` (export_kernel against the copy's kernel in the same
run); --profile runs each format --reps times and the copy, nothing else.  kernel_bytes are the algorithmic ones: 4 read per sample
plus 2, 3 or 4 written; the roofline is the 8 TB/s HBM peak.
Usage: python scripts/bench_export.py [--tracks 64] [--seconds 30] [--reps 10] [--parent-tracks 2] [--profile]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import thesia_amd as ta  # noqa: E402
from thesia_amd import _ffi, api  # noqa: E402

CASES = [("s16_tpdf", api.PCM_S16, api.DITHER_TPDF, 2), ("s24_tpdf", api.PCM_S24, api.DITHER_TPDF, 3), ("f32", api.PCM_F32, api.DITHER_NONE, 4)]
HBM_PEAK = 8.0e12


def hip_runtime():
    """the HIP runtime this process already holds (thesia_amd._ffi loaded it), for hipMemcpyAsync"""
    for name in ("libamdhip64.so.7", "libamdhip64.so"):
        try:
            h = C.CDLL(name)
            h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            h.hipDeviceSynchronize.argtypes = []
            return h
        except (OSError, AttributeError):
            continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-tracks", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    n = int(a.seconds * a.sr)
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.9, 0.9, (2, n)).astype(np.float32)
    ids = list(range(a.tracks))
    samples = 2 * n * a.tracks
    res = {"tracks": a.tracks, "channels": 2, "samples": samples, "piece_bytes": api.EXPORT_PIECE_BYTES}
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    with ta.Context(0) as ctx:
        tm = ta.TrackManager(ctx)
        tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
        tm.add_tracks([(i, a.sr, x) for i in ids])
        cap = samples * 4 + 16 * a.tracks
        pin = C.c_void_p()
        _ffi.check(_ffi.lib.th_host_alloc(ctx.handle, cap, C.byref(pin)))
        pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(cap,))
        pageable = np.empty(cap, np.uint8)
        pageable[:] = 0  # (touched: the pages exist before the first timed copy)
        for name, fmt, dith, bps in CASES:
            reqs = [(i, fmt, dith, 1) for i in ids]
            kernel_bytes = samples * (4 + bps)
            r = {"kernel_bytes": kernel_bytes, "roofline_ms_at_8TBps": round(kernel_bytes / HBM_PEAK * 1e3, 4)}
            for label, buf in (("call_pinned_ms", pinned),) + (() if a.profile else (("call_pageable_ms", pageable),)):
                for _ in range(2):
                    tm.export_pcm(reqs, out=buf)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out, infos = tm.export_pcm(reqs, out=buf)
                    ts.append((time.perf_counter() - t0) * 1e3)
                r[label] = med(ts)
                r[label.replace("_ms", "_min_ms")] = round(min(ts), 3)
            r["out_bytes"] = int(out.size)
            r["n_clamped"] = int(sum(o["n_clamped"] for o in infos))
            # the yardstick: a device-to-device copy with the same read-plus-written byte count
            half = kernel_bytes // 2 // 16 * 16
            src, dst = ctx.alloc(half), ctx.alloc(half)
            hip = hip_runtime()

            def d2d():
                assert hip.hipMemcpyAsync(dst.ptr, src.ptr, half, 3, None) == 0  # hipMemcpyDeviceToDevice, the null stream
                assert hip.hipDeviceSynchronize() == 0

            def copy_kernel():
                ctx.dev_copy(dst.ptr, src.ptr, half)
                ctx.synchronize()

            for label, fn in (("d2d_copy", d2d if hip else None), ("copy_kernel", copy_kernel)):
                if fn is None:
                    r[label + "_ms"] = None
                    continue
                fn()
                cs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    cs.append((time.perf_counter() - t0) * 1e3)
                r[label + "_ms"] = med(cs)
                r[label + "_TBps"] = round(2 * half / float(np.median(cs)) / 1e9, 3)
            src.free()
            dst.free()
            if not a.profile:
                from tests import export_ref as R
                k = max(1, min(a.parent_tracks, a.tracks))
                t0 = time.perf_counter()
                for i in ids[:k]:
                    chans = np.stack([tm.audio(i, c) for c in range(2)])
                    want, _, _ = R.pcm_bytes(fmt, dith, 1, chans, 0, n)
                r["parent_route_ms"] = round((time.perf_counter() - t0) * 1e3 * a.tracks / k, 1)
                r["parent_route_tracks_measured"] = k
                o = infos[k - 1]
                assert np.array_equal(out[o["offset"]: o["offset"] + o["n_bytes"]], want)  # the two routes give the same bytes
            res[name] = r
        _ffi.check(_ffi.lib.th_host_free(ctx.handle, pin))
        tm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
