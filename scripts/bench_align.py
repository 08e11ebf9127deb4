"""Measure the alignment reader (th_tm_align_tracks) on a 30 s x 48 kHz reference range searched over +-0.1 s and +-1 s, in one run:
  kernel        scripts/ubench/align_time (a child process; built here when missing): the correlation kernel and its fold, compiled from
                the product's source on the pieces the reader makes, timed by hipEvents; T fma/s against the 39.3 T fma/s vector f64 peak
  end_to_end    the whole call (median and minimum of --reps after a warm-up), summary and curve, with what it found
  cpu_route     what a host did before this entry existed: th_tm_copy_audio of both channels, then an FFT cross-correlation in numpy
                f64 (np.fft.rfft) and the same peak / gain / null arithmetic.  Not code of the product
Usage: python scripts/bench_align.py [--seconds 30] [--reps 5] [--no-kernel] [--no-cpu] [--out profiles/align_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import thesia_amd as ta  # noqa: E402

EXE_SRC = os.path.join(ROOT, "scripts", "ubench", "align_time.hip")
EXE = os.path.join(ROOT, "scripts", "ubench", "align_time")
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")
LAGS = (0.1, 1.0)


def build_exe():
    deps = [EXE_SRC] + [os.path.join(CSRC, f) for f in ("kernels_align.hip", "align_block.h", "align_core.h", "align_plan.h", "align_plan.cpp", "host_math.cpp")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", EXE_SRC, os.path.join(CSRC, "align_plan.cpp"),
                           os.path.join(CSRC, "host_math.cpp"), "-o", EXE])


def cpu_route(tm, sr, n_ref, D):
    """both channels over PCIe, then the correlation by FFT -> (lag, gain, null_dB, seconds in the copies, in the arithmetic)"""
    t0 = time.perf_counter()
    a, b = tm.audio(0, 0), tm.audio(1, 0)
    t1 = time.perf_counter()
    a = a[:n_ref].astype(np.float64)
    b = b.astype(np.float64)
    size = 1 << int(np.ceil(np.log2(a.size + b.size)))
    r = np.fft.irfft(np.conj(np.fft.rfft(a, size)) * np.fft.rfft(b, size), size)      # r[l] = sum a[k] b[k + l], circular
    lags = np.concatenate([r[-D:], r[:D + 1]])
    i = int(np.argmax(lags))
    lag = i - D
    e_ref = float(a @ a)
    w = b[max(lag, 0): max(lag, 0) + a.size]
    e_probe = float(w @ w)
    gain = lags[i] / e_ref
    resid = max(e_probe - lags[i] * gain, 0.0)
    null = 10 * np.log10(resid / e_probe) if resid > 0 else -np.inf
    t2 = time.perf_counter()
    return lag, gain, null, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sr, n = 48000, int(a.seconds * 48000)
    lines = []
    if not a.no_kernel:
        build_exe()
        out = subprocess.run([EXE, str(a.seconds), str(a.reps)] + [str(x) for x in LAGS], capture_output=True, text=True)
        if out.returncode != 0:  # (a fault in the child ends the measurement: nothing more is started on the card)
            print(json.dumps({"error": "align_time failed", "rc": out.returncode, "stderr": out.stderr[-400:]}))
            sys.exit(1)
        lines += [{"kernel": json.loads(ln)} for ln in out.stdout.strip().splitlines()]
    rng = np.random.default_rng(0)
    ref = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    probe = np.zeros(n + 2 * sr, np.float32)
    probe[1234:1234 + n] = 0.5 * ref
    probe += (1e-3 * rng.standard_normal(probe.size)).astype(np.float32)
    with ta.Context(0) as ctx:
        tm = ta.TrackManager(ctx)
        tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
        tm.add_tracks([(0, sr, ref[None, :]), (1, sr, probe[None, :])])
        for D_sec in LAGS:
            row = {"seconds": a.seconds, "max_lag_sec": D_sec}
            for name, kind in (("summary", ta.ALIGN_OUT_SUMMARY), ("curve", ta.ALIGN_OUT_CURVE)):
                req = ta.align_request(0, 0, 1, 0, 0.0, float("inf"), D_sec, kind)
                tm.align_tracks([req])
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    outs, infos = tm.align_tracks([req])
                    ts.append((time.perf_counter() - t0) * 1e3)
                s = ta.align_summary(outs[0])
                row[name] = {"ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "doubles": int(outs[0].size), "lag": s["lag"],
                             "gain": round(s["gain"], 6), "null_dB": round(s["null_dB"], 2), "rho": round(s["rho"], 6)}
            if not a.no_cpu:
                D = int(round(D_sec * sr))
                cpu_route(tm, sr, n, D)
                t0 = time.perf_counter()
                lag, gain, null, t_copy, t_math = cpu_route(tm, sr, n, D)
                row["cpu_route"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "copy_audio_ms": round(t_copy * 1e3, 1),
                                    "fft_and_peak_ms": round(t_math * 1e3, 1), "lag": lag, "gain": round(float(gain), 6), "null_dB": round(float(null), 2)}
            lines.append({"end_to_end": row})
        tm.close()
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
