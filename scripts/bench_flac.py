"""Time th_tm_export_flac and th_tm_export_flac_ex (flags 0, 1 = LPC, 2 = stereo, 3 = both) on 64 stereo tracks x 30 s x 48 kHz in
one process, on music-like and on noise input, 16 bit TPDF, and write profiles/flac_lpc_bench.txt (profiles/flac_bench.txt is the
record of the entry without flags):
  flac_pinned_ms    the whole call into pinned host memory (th_host_alloc), median of --reps (at least 7) after warm-up
  pcm_pinned_ms     th_tm_export_pcm of the same requests into the same memory: the only way to get this audio out before this entry
  host_16_threads_ms  th_flac_encode_i32 of the same integers on 16 host threads (a track per task; measured on --host-tracks tracks
                    and scaled to all of them)
  flac_bytes / pcm_bytes  what crosses the bus either way
  ex                per flags value of th_tm_export_flac_ex: the call's median and minimum, the files' bytes and their share of the
                    PCM's, and th_flac_encode_i32_ex on 16 host threads; flags 0 must give the bytes of th_tm_export_flac
  fixture           this encoder's frame bytes of the audio of tests/golden/flac_libflac_head.flac beside libFLAC's own
  kernels           each kernel's time by hipEvents, summed over the call's pieces, median of --reps: a child process,
                    scripts/ubench/flac_time (the product's kernels and planner compiled into a program of their own; built here
                    with hipcc when it is missing), on input of the same kind, once per flags value
--profile runs the calls --reps times and nothing else (for a run under a profiler).
Usage: python scripts/bench_flac.py [--tracks 64] [--seconds 30] [--reps 9] [--host-tracks 16] [--profile]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import thesia_amd as ta  # noqa: E402
from thesia_amd import _ffi, api  # noqa: E402


def music(n, sr, seed):
    """decaying chords over a noise floor at -70 dB: what a fixed predictor gains on"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = np.zeros(n)
    for f in (110.0, 220.0, 277.2, 329.6, 440.0, 659.3):
        x += rng.uniform(0.05, 0.2) * np.sin(2 * np.pi * f * (1 + 0.001 * seed) * t + rng.uniform(0, 6.28)) * np.exp(-((t * 2.0) % 1.0) * 3.0)
    return np.stack([x + 3e-4 * rng.standard_normal(n), 0.8 * x + 3e-4 * rng.standard_normal(n)]).astype(np.float32)


def kernel_times(kind, seconds, tracks, reps, flags=0):
    import shutil
    import subprocess
    exe = os.path.join(ROOT, "scripts", "ubench", "flac_time")
    csrc = os.path.join(ROOT, "thesia_amd", "csrc")
    deps = [exe + ".hip", os.path.join(ROOT, "include", "thesia_amd.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc)
                                                                             if f.startswith("flac_") or f in ("kernels_flac.hip", "export_core.h", "stft_core.h", "kernels.h")]
    # (a binary older than its sources, one of the tree before the flags for instance, would take no fifth argument and time flags 0)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", exe + ".hip",
                               os.path.join(ROOT, "thesia_amd", "csrc", "flac_plan.cpp"), "-o", exe])
    out = subprocess.run([exe, kind, str(seconds), str(tracks), str(reps), str(flags)], check=True, capture_output=True, text=True).stdout
    res = json.loads(out.strip().splitlines()[-1])
    assert res.get("flags") == flags, "scripts/ubench/flac_time did not run flags %d: %r" % (flags, res.get("flags"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flac_lpc_bench.txt"))
    a = ap.parse_args()
    assert a.reps >= 7
    n = int(a.seconds * a.sr)
    ids = list(range(a.tracks))
    fmt, dith = api.PCM_S16, api.DITHER_TPDF
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    lines, kernels = [], []
    with ta.Context(0) as ctx:
        cap = sum((ta.flac_bound(n, 2, fmt) + 15) // 16 * 16 for _ in ids)
        pin = C.c_void_p()
        _ffi.check(_ffi.lib.th_host_alloc(ctx.handle, cap, C.byref(pin)))
        pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(cap,))
        for kind in ("music", "noise"):
            rng = np.random.default_rng(1)
            tracks = [music(n, a.sr, i) if kind == "music" else rng.uniform(-0.9, 0.9, (2, n)).astype(np.float32) for i in ids[:4]]
            tm = ta.TrackManager(ctx)
            tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
            tm.add_tracks([(i, a.sr, tracks[i % len(tracks)]) for i in ids])
            reqs = [(i, fmt, dith, 1) for i in ids]
            r = {"input": kind, "tracks": a.tracks, "channels": 2, "samples": 2 * n * a.tracks, "format": "s16_tpdf"}
            for label, call in (("flac", tm.export_flac), ("pcm", tm.export_pcm)):
                for _ in range(2):
                    call(reqs, out=pinned)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out, infos = call(reqs, out=pinned)
                    ts.append((time.perf_counter() - t0) * 1e3)
                r[label + "_pinned_ms"] = med(ts)
                r[label + "_pinned_min_ms"] = round(min(ts), 3)
                r[label + "_bytes"] = int(sum(o["n_bytes"] for o in infos))
                if label == "flac":
                    first = out[infos[0]["offset"]: infos[0]["offset"] + infos[0]["n_bytes"]].tobytes()
            r["flac_over_pcm_bytes"] = round(r["flac_bytes"] / r["pcm_bytes"], 4)
            r["ex"], firsts = [], {}
            for flags in (0, 1, 2, 3):
                for _ in range(2):
                    tm.export_flac(reqs, out=pinned, flags=flags)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out, infos = tm.export_flac(reqs, out=pinned, flags=flags)
                    ts.append((time.perf_counter() - t0) * 1e3)
                nbytes = int(sum(o["n_bytes"] for o in infos))
                firsts[flags] = out[infos[0]["offset"]: infos[0]["offset"] + infos[0]["n_bytes"]].tobytes()
                r["ex"].append({"flags": flags, "pinned_ms": med(ts), "pinned_min_ms": round(min(ts), 3), "bytes": nbytes,
                                "over_pcm_bytes": round(nbytes / r["pcm_bytes"], 4)})
            assert firsts[0] == first and r["ex"][0]["bytes"] == r["flac_bytes"]  # flags == 0 is the entry without flags
            if not a.profile:
                k = max(1, min(a.host_tracks, a.tracks))
                q = []
                for i in ids[:k]:
                    x = np.stack([tm.audio(i, c) for c in range(2)])
                    q.append(np.stack([ta.export_quantize(fmt, dith, 1, c, 0, x[c])[0] for c in range(2)]))
                assert ta.flac_encode_i32(q[0], fmt, a.sr) == first  # the two routes give the same file
                with ThreadPoolExecutor(max_workers=16) as pool:
                    t0 = time.perf_counter()
                    list(pool.map(lambda qq: ta.flac_encode_i32(qq, fmt, a.sr), q))
                    r["host_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3 * a.tracks / k, 1)
                    for e in r["ex"]:
                        assert ta.flac_encode_i32(q[0], fmt, a.sr, flags=e["flags"]) == firsts[e["flags"]]
                        t0 = time.perf_counter()
                        list(pool.map(lambda qq: ta.flac_encode_i32(qq, fmt, a.sr, flags=e["flags"]), q))
                        e["host_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3 * a.tracks / k, 1)
                r["host_tracks_measured"] = k
            tm.close()
            lines.append(json.dumps(r))
            if not a.profile:
                kernels.append(kind)
        _ffi.check(_ffi.lib.th_host_free(ctx.handle, pin))
    for kind in kernels:  # (behind the context: one process on the card at a time)
        for flags in (0, 1, 2, 3):
            lines.append(json.dumps({"kernels": kernel_times(kind, a.seconds, a.tracks, a.reps, flags)}))
    if not a.profile:
        from tests import flac_ref as F
        gold = os.path.join(ROOT, "tests", "golden", "flac_libflac_head.flac")
        data = open(gold, "rb").read()
        dec = F.decode(data)
        mine = ta.flac_encode_i32(np.array(dec["channels"], np.int32), api.PCM_S16, dec["sr"])
        lpc = ta.flac_encode_i32(np.array(dec["channels"], np.int32), api.PCM_S16, dec["sr"], flags=ta.FLAC_LPC)
        lines.append(json.dumps({"fixture": "flac_libflac_head.flac", "samples": len(dec["channels"][0]), "pcm_bytes": 2 * len(dec["channels"][0]),
                                 "libflac_frame_bytes": len(data) - dec["first_frame"], "this_encoder_frame_bytes": len(mine) - 42,
                                 "this_encoder_lpc_frame_bytes": len(lpc) - 42}))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# python scripts/bench_flac.py --tracks %d --seconds %g --reps %d\n" % (a.tracks, a.seconds, a.reps))
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
