"""Formant candidates, the host side (no GPU): the plan table and every argument rule, the absolute frame grid, th_formants_f64 and
th_formant_frame_f64 bit for bit against the restatement (tests/formant_ref.py), and three checks that do not share its formulation:
the LPC coefficients against a dense solve of the Toeplitz system, every root against the residual bound of its own polynomial, and
a known answer (the impulse response of an all-pole filter)."""
import math

import numpy as np
import pytest

import thesia_amd as ta
from tests import formant_ref as R

INF, NAN = float("inf"), float("nan")
EPS = 2.0 ** -53


def _sec(sample, sr):
    """a time whose product with sr rounds up to exactly `sample`"""
    t = sample / sr
    while math.ceil(t * float(sr)) > sample:
        t = float(np.nextafter(t, 0.0))
    assert math.ceil(t * float(sr)) == sample
    return t


def signals(n, sr, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    noise = 0.1 * rng.standard_normal(n)
    pulses = np.zeros(n)
    pulses[::max(sr // 120, 1)] = 1.0
    vowel = pulses.copy()
    for fr, bw in ((700, 80), (1200, 90), (2600, 120)):   # a pulse train through three resonators
        rho, th = math.exp(-math.pi * bw / sr), 2 * math.pi * fr / sr
        y = np.zeros(n)
        for i in range(n):
            y[i] = vowel[i] + 2 * rho * math.cos(th) * (y[i - 1] if i > 0 else 0.0) - rho * rho * (y[i - 2] if i > 1 else 0.0)
        vowel = y
    return {"noise": noise.astype(np.float32), "sine_noise": (0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.01 * noise).astype(np.float32),
            "vowel": (vowel / np.abs(vowel).max()).astype(np.float32), "sine": (0.5 * np.sin(2 * np.pi * 997.0 * t)).astype(np.float32)}


def assert_bits(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, np.nonzero(a.ravel().view(np.uint64) != b.ravel().view(np.uint64))[0][:5])


# ---------------------------------------------------------------------------------------------------------------- plans
def test_defaults_and_plan_table():
    r = ta.formant_request()
    assert (r.sr_analysis, r.n_poles, r.win_sec, r.step_sec, r.preemph_hz, r.window, r.kind) == (11000, 10, 0.05, 0.0125, 50.0, 0, 0)
    assert r.start_sec == 0.0 and r.end_sec == INF
    p = ta.formant_plan(48000, 480000, r)
    assert (p["sr_analysis"], p["resampled"], p["win"], p["hop"], p["n_analysis"]) == (11000, 1, 550, 138, 110000)
    assert p["n_analysis"] == ta.resample_n_out(480000, 48000, 11000) and p["rs"] == (11, 48, 559)
    assert p["n_frames_total"] == -(-110000 // 138) and (p["frame_first"], p["frame_end"]) == (0, p["n_frames_total"])
    assert p["alpha"] == math.exp(-2.0 * math.pi * 50.0 / 11000.0)
    p = ta.formant_plan(44100, 44100, r)
    assert (p["sr_analysis"], p["resampled"], p["win"], p["hop"], p["n_analysis"], p["rs"][:2]) == (11000, 1, 550, 138, 11000, (110, 441))
    p = ta.formant_plan(8000, 8001, ta.formant_request(sr_analysis=8000))
    assert (p["sr_analysis"], p["resampled"], p["win"], p["hop"], p["n_analysis"], p["n_frames_total"]) == (8000, 0, 400, 100, 8001, 81)
    p = ta.formant_plan(8000, 8000, ta.formant_request(sr_analysis=0))
    assert (p["sr_analysis"], p["resampled"], p["n_frames_total"]) == (8000, 0, 80)
    assert ta.formant_plan(8000, 0, ta.formant_request(sr_analysis=0))["n_frames_total"] == 0
    assert ta.formant_plan(8000, 100, ta.formant_request(sr_analysis=0, preemph_hz=INF))["alpha"] == 0.0
    assert ta.formant_plan(8000, 100, ta.formant_request(sr_analysis=0, step_sec=0.0))["hop"] == 1


BAD = [dict(n_poles=0), dict(n_poles=3), dict(n_poles=34), dict(n_poles=11), dict(win_sec=NAN), dict(win_sec=INF), dict(win_sec=0.0),
       dict(win_sec=-0.05), dict(win_sec=11.0 / 11000), dict(win_sec=4097.0 / 11000), dict(step_sec=NAN), dict(step_sec=-1.0),
       dict(step_sec=INF), dict(step_sec=65537.0 / 11000), dict(preemph_hz=NAN), dict(preemph_hz=-1.0), dict(window=2), dict(kind=2),
       dict(which=3), dict(start_sec=NAN), dict(end_sec=NAN), dict(start_sec=-1.0), dict(start_sec=INF), dict(start_sec=2.0, end_sec=1.0)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join("%s=%s" % c for c in kw.items()))
def test_argument_rules(kw):
    with pytest.raises(ta.ThError) as e:
        ta.formant_plan(48000, 480000, ta.formant_request(**kw))
    assert e.value.code == -1, (e.value.code, str(e.value))


def test_limits_accepted_and_zero_rate():
    ta.formant_plan(48000, 480000, ta.formant_request(win_sec=12.0 / 11000))     # W = p + 2
    ta.formant_plan(48000, 480000, ta.formant_request(win_sec=4096.0 / 11000, step_sec=65536.0 / 11000, n_poles=32))
    with pytest.raises(ta.ThError) as e:
        ta.formant_plan(0, 100, ta.formant_request())
    assert e.value.code == -1


@pytest.mark.parametrize("sr,sr_a", [(192000, 2000), (96000, 95999)])
def test_refused_rate_pair_is_unsupported(sr, sr_a):
    with pytest.raises(ta.ThError):
        ta.resample_plan(sr, sr_a)
    with pytest.raises(ta.ThError) as e:
        ta.formant_plan(sr, 1000, ta.formant_request(sr_analysis=sr_a, win_sec=0.01))
    assert e.value.code == ta._ffi.ERR_UNSUPPORTED
    with pytest.raises(ta.ThError) as e:   # an argument fault of the same request comes first
        ta.formant_plan(sr, 1000, ta.formant_request(sr_analysis=sr_a, win_sec=0.01, n_poles=3))
    assert e.value.code == ta._ffi.ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------- frame grid
@pytest.mark.parametrize("sr,sr_a", [(8000, 0), (44100, 11000)])
def test_frame_grid_and_range_is_a_slice(sr, sr_a):
    x = signals(sr // 4, sr, 3)["vowel"]
    base = dict(sr_analysis=sr_a, n_poles=6, win_sec=0.01, step_sec=0.004)
    plan = ta.formant_plan(sr, x.size, ta.formant_request(**base))
    H, n_a, rate = plan["hop"], plan["n_analysis"], plan["sr_analysis"]
    assert plan["n_frames_total"] == -(-n_a // H)
    whole, _ = ta.formants_f64(x, sr, base)
    assert whole.shape == (plan["n_frames_total"], 8)
    for s0 in (0, 1, H - 1, H, H + 1, 5 * H + 1):
        for s1 in (s0, s0 + 1, 7 * H, 7 * H + 1, None):
            if s1 is not None and s1 < s0:
                continue
            req = dict(base, start_sec=_sec(s0, rate), end_sec=INF if s1 is None else _sec(s1, rate))
            assert ta.audio_sample_range(rate, n_a, req["start_sec"], req["end_sec"]) == (s0, n_a if s1 is None else s1)
            p = ta.formant_plan(sr, x.size, ta.formant_request(**req))
            f0, f1 = -(-s0 // H), plan["n_frames_total"] if s1 is None else -(-s1 // H)
            assert (p["frame_first"], p["frame_end"]) == (f0, f1), (s0, s1)
            part, _ = ta.formants_f64(x, sr, req, f0, f1 - f0)
            assert_bits(part, whole[f0:f1], (s0, s1))
    with pytest.raises(ta.ThError):
        ta.formants_f64(x, sr, base, plan["n_frames_total"], 1)


# ---------------------------------------------------------------------------------------------------------------- the restatement
RESTATED = [  # sr, sr_a, p, win samples, hop samples, window, preemph_hz, signal
    (8000, 0, 2, 4, 1, 0, 50.0, "noise"), (8000, 0, 10, 129, 7, 0, 50.0, "vowel"), (8000, 0, 16, 64, 64, 1, INF, "sine_noise"),
    (8000, 0, 32, 65, 130, 0, 50.0, "sine"), (8000, 0, 4, 63, 63, 1, 50.0, "vowel"), (44100, 11000, 10, 550, 138, 0, 50.0, "vowel"),
    (48000, 11000, 8, 200, 300, 1, INF, "noise")]


@pytest.mark.parametrize("sr,sr_a,p,W,H,window,pre,name", RESTATED)
def test_host_equals_the_restatement_bit_for_bit(sr, sr_a, p, W, H, window, pre, name):
    rate = sr_a or sr
    n = 700 if sr == 8000 else sr // 8
    x = signals(n, sr, 5)[name]
    for kind in (ta.FORMANT_OUT_FORMANTS, ta.FORMANT_OUT_LPC):
        req = dict(sr_analysis=sr_a, n_poles=p, win_sec=W / rate, step_sec=H / rate, preemph_hz=pre, window=window, kind=kind)
        plan = ta.formant_plan(sr, n, req)
        assert (plan["win"], plan["hop"]) == (W, H)
        frames = sorted({0, 1, plan["n_frames_total"] // 2, plan["n_frames_total"] - 1})
        u = R.analysis_signal(x, sr, plan)
        g, z0 = ta.formant_window(window, W), ta.formant_start_points(p)
        for f in frames:
            fit = R.frame(u, plan, g, z0, f)
            got = ta.formant_frame_f64(x, sr, req, f)
            assert (got["status"], got["sweeps"]) == (fit["status"], fit["sweeps"]), f
            for k in ("r", "a", "roots"):
                assert_bits(got[k].view(np.float64), fit[k].view(np.float64), (k, f))
            assert_bits([got["r0_loaded"], got["E"]], [fit["r0_loaded"], fit["E"]], f)
            if kind == ta.FORMANT_OUT_LPC:
                fit = R.frame(u, plan, g, z0, f, roots=False)
            want = np.array(R.pack(fit, plan))
            row = ta.formants_f64(x, sr, req, f, 1)[0][0]
            assert np.array_equal(np.isnan(row), np.isnan(want)), f
            if kind == ta.FORMANT_OUT_LPC:
                assert_bits(row, want, f)
            else:  # step 6 goes through libm on both sides: the same bits where they agree, else the last place
                assert_bits(row[:2], want[:2], f)
                fin = ~np.isnan(want)
                assert (np.abs(row[fin] - want[fin]) <= np.spacing(np.abs(want[fin]))).all(), f


# ---------------------------------------------------------------------------------------------------------------- independent checks
FITS = [(p, W) for p in (2, 4, 10, 16, 32) for W in (p + 2, 63, 64, 65, 129, 550, 1023) if W >= p + 2]


@pytest.fixture(scope="module")
def fits():
    """the raw fit of a few frames of four signals at every (p, W): 50 Hz pre-emphasis, Gaussian window; computed once"""
    sr, n = 8000, 4000
    out = []
    for name, x in signals(n, sr, 9).items():
        for p, W in FITS:
            req = dict(sr_analysis=0, n_poles=p, win_sec=W / sr, step_sec=0.05)
            for f in (2, 5, 8):
                out.append((name, p, W, f, ta.formant_frame_f64(x, sr, req, f)))
    return out


def test_every_frame_converges(fits):
    worst = max(fit["sweeps"] for *_, fit in fits)
    print("frames %d, most sweeps %d" % (len(fits), worst))
    assert all(fit["status"] == 0 for *_, fit in fits), [(c[:4], c[4]["status"]) for c in fits if c[4]["status"] != 0][:5]
    assert 1 <= worst <= 64
    x = signals(4000, 8000, 9)["vowel"]
    _, counts = ta.formants_f64(x, 8000, dict(sr_analysis=0))
    assert counts == (0, 0)


def test_lpc_coefficients_against_a_dense_solve(fits):
    """a solves T a = -r[1 .. p], T the symmetric Toeplitz matrix of (r0', r[1], .. r[p - 1]).  A backward-stable dense solve has a
    relative forward error of at most about p eps cond(T); Levinson-Durbin on a positive definite T is weakly stable, its residual is
    of the order p^2 eps |r0'| |a| (Cybenko 1980), so its forward error is at most about p^2 eps cond(T).  The bound asserted is the
    sum of both with a factor 2, from the condition number numpy computes for this very T."""
    ratio = 0.0
    for name, p, W, f, fit in fits:
        r, a = fit["r"], fit["a"]
        col = np.concatenate([[fit["r0_loaded"]], r[1:p]])
        T = col[np.abs(np.subtract.outer(np.arange(p), np.arange(p)))]
        want = np.linalg.solve(T, -r[1:])
        bound = 2.0 * (p * p + p) * 2 * EPS * np.linalg.cond(T)
        err = np.linalg.norm(a[1:] - want) / np.linalg.norm(want)
        ratio = max(ratio, err / bound)
        assert err <= bound, (name, p, W, f, err, bound)
        # ... and E is the prediction error of that a: r0' + sum a_k r[k]
        assert abs(fit["E"] - (fit["r0_loaded"] + a[1:] @ r[1:])) <= bound * fit["r0_loaded"] * (1 + np.abs(a[1:]).sum()), (name, p, W, f)
    print("worst error / bound %.3g" % ratio)


def test_every_root_satisfies_its_residual_bound(fits):
    """|P(z)| <= 2 p 2^-53 sum |a_k| |z|^(p - k) + 2^-40 |P'(z)|: Horner's backward error plus the stop rule (the last correction is
    below 2^-40, and |P(z)| is about |w| |P'(z)|).  P and P' are evaluated in extended precision."""
    worst = 0.0
    for name, p, W, f, fit in fits:
        a = fit["a"].astype(np.longdouble)
        for z in fit["roots"]:
            zl = np.clongdouble(z)
            P, D = np.clongdouble(1.0), np.clongdouble(0.0)
            for k in range(1, p + 1):
                D = D * zl + P
                P = P * zl + a[k]
            scale = sum(abs(float(a[k])) * abs(z) ** (p - k) for k in range(p + 1))
            bound = 2 * p * EPS * scale + 2.0 ** -40 * abs(complex(D))
            worst = max(worst, abs(complex(P)) / (EPS * scale))
            assert abs(complex(P)) <= bound, (name, p, W, f, z, abs(complex(P)), bound)
    print("worst |P(z)| = %.2f x 2^-53 x sum |a_k| |z|^(p - k)" % worst)


def test_known_answer_all_pole_impulse_response():
    sr, res = 10000, [(700.0, 80.0), (1200.0, 90.0), (2600.0, 120.0), (3500.0, 150.0)]
    A = np.array([1.0])
    for fr, bw in res:
        rho, th = math.exp(-math.pi * bw / sr), 2 * math.pi * fr / sr
        A = np.convolve(A, [1.0, -2 * rho * math.cos(th), rho * rho])
    W, lead = 4096, 2048
    h = np.zeros(W)
    for i in range(W):
        h[i] = (1.0 if i == 0 else 0.0) - sum(A[k] * h[i - k] for k in range(1, 9) if i >= k)
    x = np.concatenate([np.zeros(lead), h, np.zeros(8)]).astype(np.float32)   # frame 1 (centre 2048) starts on the impulse
    req = dict(sr_analysis=0, n_poles=8, win_sec=W / sr, step_sec=lead / sr, preemph_hz=INF, window=ta.FORMANT_WIN_RECT)
    plan = ta.formant_plan(sr, x.size, req)
    assert (plan["win"], plan["hop"], plan["alpha"]) == (W, lead, 0.0)
    out, counts = ta.formants_f64(x, sr, req, 1, 1)
    assert counts == (0, 0) and out[0, 0] == 4
    df = np.abs(out[0, 2:6] - [c[0] for c in res]).max()
    db = np.abs(out[0, 6:10] - [c[1] for c in res]).max()
    print("formants within %.2e Hz, bandwidths within %.2e Hz" % (df, db))
    assert df <= 1e-3 and db <= 1e-3


# ---------------------------------------------------------------------------------------------------------------- edge cases
def test_silence_is_invalid():
    out, counts = ta.formants_f64(np.zeros(1000, np.float32), 8000, dict(sr_analysis=0))
    assert out.shape == (10, 12) and np.isnan(out).all() and counts == (10, 0)
    fit = ta.formant_frame_f64(np.zeros(1000, np.float32), 8000, dict(sr_analysis=0), 3)
    assert fit["status"] == 1 and not fit["roots"].any() and not fit["a"][1:].any() and fit["sweeps"] == 0


@pytest.mark.parametrize("pre", [50.0, INF])
@pytest.mark.parametrize("at", [0, 333, 999])
def test_one_nan_sample_invalidates_exactly_the_frames_that_touch_it(at, pre):
    sr, W, H = 8000, 65, 20
    x = signals(1000, sr, 4)["noise"]
    x[at] = NAN
    req = dict(sr_analysis=0, n_poles=4, win_sec=W / sr, step_sec=H / sr, preemph_hz=pre)
    out, counts = ta.formants_f64(x, sr, req)
    touched = []
    for f in range(out.shape[0]):
        b = f * H - W // 2     # d[at] and d[at + 1] carry the NaN (alpha x NaN is NaN even when alpha is 0)
        touched.append(any(b <= n < b + W and n < x.size for n in (at, at + 1)))
    assert np.array_equal(np.isnan(out).all(axis=1), touched) and not np.isnan(out[~np.array(touched), :2]).any()
    assert counts == (sum(touched), 0) and 0 < sum(touched) < out.shape[0]
