"""Measure the formant reader (th_tm_get_formants) on 64 stereo tracks x 30 s x 48 kHz with the speech defaults (analysis at 11 kHz,
10 poles, 50 ms Gaussian window, 12.5 ms step), in one run:
  kernels       scripts/ubench/formant_time (a child process; built here when missing): resample_kernel and formant_kernel, compiled
                from the product's sources on the plan the reader makes, each timed by hipEvents
  end_to_end    the whole call for all 128 channels (median and minimum of --reps after a warm-up), formants and LPC
  cpu_route     what a host did before this entry existed, on 16 channels in 16 threads: th_tm_copy_audio per channel, then
                scipy.signal.resample_poly to 11 kHz, pre-emphasis, Gaussian window, autocorrelation, Levinson-Durbin over all frames at
                once and the eigenvalues of the companion matrices, in numpy; scaled to 128 channels.  Not code of the product
Usage: python scripts/bench_formant.py [--tracks 64] [--seconds 30] [--reps 5] [--no-kernel] [--no-cpu]"""
import argparse
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

EXE_SRC = os.path.join(ROOT, "scripts", "ubench", "formant_time.hip")
EXE = os.path.join(ROOT, "scripts", "ubench", "formant_time")
CSRC = os.path.join(ROOT, "thesia_amd", "csrc")


def build_exe():
    deps = [EXE_SRC] + [os.path.join(CSRC, f) for f in ("kernels_formant.hip", "formant_block.h", "formant_core.h", "formant_plan.h", "formant_plan.cpp",
                                                        "kernels_resample.hip", "resample_block.h", "host_math.cpp")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return
    lib_dir = os.path.join(ROOT, "thesia_amd")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", EXE_SRC,
                           os.path.join(CSRC, "formant_plan.cpp"), os.path.join(CSRC, "host_math.cpp"), "-L" + lib_dir, "-lthesia_amd",
                           "-Wl,-rpath," + lib_dir, "-o", EXE])


def cpu_channel(tm, tid, ch, plan, g):
    """one channel the old way -> (frames, seconds spent in the copy, in the decimation, in the LPC and roots)"""
    from scipy.signal import resample_poly
    t0 = time.perf_counter()
    x = tm.audio(tid, ch)
    t1 = time.perf_counter()
    L, M, K = plan["rs"]
    t = np.arange(-K * L, K * L + 1) / L
    rho = min(1.0, L / M)
    h = rho * 0.95 * np.sinc(rho * 0.95 * t) * np.blackman(t.size)   # a windowed sinc of the product's length (its window differs)
    u = resample_poly(x.astype(np.float64), L, M, window=h / L)
    t2 = time.perf_counter()
    p, W, H = plan["n_poles"], plan["win"], plan["hop"]
    d = u.copy()
    d[1:] -= plan["alpha"] * u[:-1]
    d = np.concatenate([np.zeros(W // 2), d, np.zeros(W)])
    F = -(-u.size // H)
    fr = np.lib.stride_tricks.as_strided(d, (F, W), (d.strides[0] * H, d.strides[0])) * g
    r = np.stack([(fr[:, :W - m] * fr[:, m:]).sum(axis=1) for m in range(p + 1)], axis=1)
    r[:, 0] *= 1.0 + 2.0 ** -30
    ok = r[:, 0] > 0
    r = r[ok]
    a = np.zeros((r.shape[0], p + 1))
    a[:, 0] = 1.0
    E = r[:, 0].copy()
    for i in range(1, p + 1):
        acc = r[:, i] + (a[:, 1:i] * r[:, i - 1:0:-1]).sum(axis=1)
        k = -acc / E
        a[:, 1:i] = a[:, 1:i] + k[:, None] * a[:, i - 1:0:-1]
        a[:, i] = k
        E = E * (1.0 - k * k)
    comp = np.zeros((r.shape[0], p, p))
    comp[:, 0, :] = -a[:, 1:]
    comp[:, np.arange(1, p), np.arange(p - 1)] = 1.0
    z = np.linalg.eigvals(comp)
    f = np.angle(z) * plan["sr_analysis"] / (2 * np.pi)
    bw = -np.log(np.abs(z) ** 2) * plan["sr_analysis"] / (2 * np.pi)
    t3 = time.perf_counter()
    return (F, f, bw), t1 - t0, t2 - t1, t3 - t2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    sr, n = 48000, int(a.seconds * 48000)
    res = {"tracks": a.tracks, "channels": 2 * a.tracks, "seconds": a.seconds, "sr": sr}
    if not a.no_kernel:
        build_exe()
        out = subprocess.run([EXE, str(a.seconds), str(2 * a.tracks), str(a.reps)], capture_output=True, text=True)
        if out.returncode != 0:  # (a fault in the child ends the measurement: nothing more is started on the card)
            print(json.dumps({"error": "formant_time failed", "rc": out.returncode, "stderr": out.stderr[-400:]}))
            sys.exit(1)
        res["kernels"] = json.loads(out.stdout.strip().splitlines()[-1])
    rng = np.random.default_rng(0)
    t = np.arange(n) / sr
    x = np.stack([0.3 * np.sin(2 * np.pi * 700 * t) + 0.2 * np.sin(2 * np.pi * 1220 * t) + 0.05 * rng.standard_normal(n) for _ in range(2)]).astype(np.float32)
    plan = ta.formant_plan(sr, n, ta.formant_request())
    res["frames_per_channel"] = plan["n_frames_total"]
    with ta.Context(0) as ctx:
        tm = ta.TrackManager(ctx)
        tm.set_setting(40.0, 2, 1, ta.LINEAR)  # (the specs are not what is measured: a cheap framing)
        tm.add_tracks([(i, sr, x) for i in range(a.tracks)])
        e2e = {}
        for name, kind in (("formants", ta.FORMANT_OUT_FORMANTS), ("lpc", ta.FORMANT_OUT_LPC)):
            reqs = [ta.formant_request(i, c, kind=kind) for i in range(a.tracks) for c in range(2)]
            out = np.empty(len(reqs) * plan["n_frames_total"] * 12, np.float64)
            tm.get_formants(reqs, out=out)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                outs, infos = tm.get_formants(reqs, out=out)
                ts.append((time.perf_counter() - t0) * 1e3)
            e2e[name] = {"ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "doubles": int(sum(o.size for o in outs)),
                         "n_invalid": int(sum(i["n_invalid"] for i in infos)), "n_unconverged": int(sum(i["n_unconverged"] for i in infos))}
        res["end_to_end"] = e2e
        if not a.no_cpu:
            g = ta.formant_window(plan["window"], plan["win"])
            n_thr = 16
            work = [(i // 2 % a.tracks, i % 2) for i in range(n_thr)]
            t0 = time.perf_counter()
            with ThreadPoolExecutor(n_thr) as pool:
                rs = list(pool.map(lambda w: cpu_channel(tm, w[0], w[1], plan, g), work))
            wall = time.perf_counter() - t0
            res["cpu_route"] = {"channels_measured": n_thr, "threads": n_thr, "wall_ms": round(wall * 1e3, 1),
                                "copy_audio_ms_per_channel": round(1e3 * np.mean([r[1] for r in rs]), 2),
                                "decimation_ms_per_channel": round(1e3 * np.mean([r[2] for r in rs]), 1),
                                "lpc_and_roots_ms_per_channel": round(1e3 * np.mean([r[3] for r in rs]), 1),
                                "scaled_to_all_channels_on_16_threads_ms": round(wall * 1e3 * 2 * a.tracks / n_thr, 1)}
        tm.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
