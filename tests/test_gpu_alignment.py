"""Every stream-ordered ("_dev") entry on device pointers that are only ELEMENT-aligned (include/thesia_amd.h, Conventions).

The kernels branch on the alignment of the base pointers they are given (float4 / float2 / dword fast paths against
per-element paths), and every buffer the rest of the suite hands over starts on a 256-byte boundary.  A host that uploads
the reference's Array2<f32> of channels x samples (core/audio.rs:25) as it is gives every channel after the first a base
that is 4-byte aligned and nothing more; spec rows and images may be sub-rectangles of wider arrays.  Here every input
and output of a call is a VIEW into one device arena:

  - the arena holds a sentinel bit pattern (SENT1 of tests/test_gpu_streams.py: a NaN for f32, 0xBEEF for u16, 0xA5 for
    bytes); a view starts MARGIN (4 KiB: a layout choice, so that a head or tail that is off by a few vector widths lands
    in sentinel that is read back, not in another view or in unmapped memory) + k elements behind a 256-byte boundary and
    has MARGIN of sentinel behind it;
  - k runs over the phases of the access widths the kernels use: 0 .. 3 elements for f32 (16-byte phases), 0, 1, 2, 3, 4, 6
    for u16 (odd pixel; 4-, 8-, 16-byte phases), 0, 1 for f64, 0 .. 3 pixels for RGBA / colour-map pointers.  A case varies
    one pointer, the others at 0; one case per entry has every pointer at a different non-zero offset.

Asserted for every case:
  1. the outputs against the oracle / restatement, with the function and tolerance the existing test of the same entry uses
     (imported, not copied);
  2. bit-identical outputs to the same call on the same data with every offset 0 — except th_channel_stats_dev's
     sum_squares and th_audio_stats_dev's rms_dB, whose unaligned side sums in another order by design (1. only);
  3. every byte of the arena outside the extents the header gives the library still holds what it held before the call.

The table ENTRIES names every (entry, DEVICE pointer) pair; test_table_names_every_device_pointer (no GPU needed) parses
the header and fails when a "_dev" function or a struct field commented DEVICE is missing from it.  A pointer below its
stated alignment is refused with TH_ERR_INVALID_ARG before anything is launched (test_misaligned_pointer_is_refused).
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

# ---------------------------------------------------------------- the table: entry -> {DEVICE pointer: (offsets k, alignment in bytes)}
F32 = ((0, 1, 2, 3), 4)
U16 = ((0, 1, 2, 3, 4, 6), 2)
F64 = ((0, 1), 8)
PX = ((0, 1, 2, 3), 4)        # RGBA8 pixels / colour-map entries
BYTES = ((0, 1, 3, 7), 1)
ENTRIES = {
    "th_calc_spec_batch_dev": {"wav": F32, "spec": F32, "d_minmax": F32},
    "th_calc_spec_batch_ranged_dev": {"wav": F32, "spec": F32, "d_minmax": F32, "d_range": F32},
    "th_minmax_reduce_dev": {"d_minmax": F32, "d_out": F32},
    "th_global_db_range_dev": {"d_min_negmax": F32, "d_range": F32},
    "th_minmax_reduce_range_dev": {"d_minmax": F32, "d_min_negmax": F32, "d_range": F32},
    "th_spec_to_img_dev": {"d_spec": F32, "d_img": U16},
    "th_spec_to_img_batch_dev": {"spec": F32, "img": U16},
    "th_spec_to_img_batch_dev_ranged": {"spec": F32, "img": U16, "d_range": F32},
    "th_spec_to_img_raster_batch_dev": {"img.spec": F32, "img.img": U16, "tiles": PX, "d_range": F32, "d_colormap": PX},
    "th_raster_tiles_dev": {"img": U16, "rgba": PX, "d_colormap": PX},
    "th_encode_spectrogram_tile_dev": {"d_img": U16},
    "th_encode_waveform_tile_dev": {"d_wav": F32},
    "th_waveform_tiles_dev": {"wav": F32, "bins": F32},
    "th_waveform_pyramid_dev": {"wav": F32, "out": F32},
    "th_channel_stats_dev": {"wav": F32},
    "th_audio_stats_dev": {"channels": F32, "block_energy": F64},
    "th_dev_upload": {"dst_dev": BYTES},
    "th_dev_download": {"src_dev": BYTES},
}
# "_dev" names of the header with no device memory access of their own to vary
EXEMPT = {
    "th_dev_alloc": "returns an allocation (hipMalloc: 256-byte aligned)",
    "th_dev_free": "frees an allocation, reads nothing",
    "th_dev_copy": "states 16 bytes for both pointers and the size: offsets and refusal in tests/test_gpu_streams.py "
                   "(test_dev_copy_on_caller_stream, test_dev_copy_refuses_misaligned_arguments)",
}
COVERED = {}   # entry -> test function names that run it (filled by @covers at import)


def covers(*entries):
    def deco(fn):
        for e in entries:
            assert e in ENTRIES, e
            COVERED.setdefault(e, []).append(fn.__name__)
        return fn
    return deco


def cases(entry):
    """[(id, {pointer: k})]: all offsets 0; every pointer over its non-zero offsets, the others at 0; every pointer at a
    different non-zero offset."""
    ptrs = ENTRIES[entry]
    out = [("base", {})]
    for p, (offs, _) in ptrs.items():
        out += [(f"{p}+{k}", {p: k}) for k in offs if k]
    if len(ptrs) > 1:
        out.append(("all", {p: offs[1 + i % (len(offs) - 1)] for i, (p, (offs, _)) in enumerate(ptrs.items())}))
    return [pytest.param(ks, id=i) for i, ks in out]


# ---------------------------------------------------------------- completeness (CPU)
def _header():
    return open(os.path.join(ROOT, "include", "thesia_amd.h")).read()


def header_device_pointers():
    """{function with a _dev name: set of DEVICE pointer names} from include/thesia_amd.h: parameters named d_* / *_dev, and
    the fields commented DEVICE of every struct a parameter points to (a nested struct's fields as outer.inner)."""
    txt = _header()
    # a comment becomes a mark where it says DEVICE and nothing otherwise (comments hold ';' and ')' of their own)
    marked = re.sub(r"/\*.*?\*/", lambda m: "@DEVICE@" if "DEVICE" in m.group(0) else "", txt, flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(th_\w+);", marked, flags=re.S):
        fields = []
        for decl, mark in re.findall(r"([^;{}@]+);[ \t]*(@DEVICE@)?", body):   # (the comment behind a field, on its line)
            m = re.match(r"(.*?)(\w+)$", decl.split(",")[0].strip(), flags=re.S)
            if m:
                fields.append((m.group(1).strip(), m.group(2), bool(mark)))
        structs[name] = fields

    def dev_fields(sname, prefix=""):
        out = set()
        for ftype, fname, is_dev in structs[sname]:
            if ftype in structs:
                out |= dev_fields(ftype, prefix + fname + ".")
            elif is_dev:
                out.add(prefix + fname)
        return out

    plain = marked.replace("@DEVICE@", "")
    found = {}
    for name, params in re.findall(r"TH_API\s+[\w\s\*]+?\b(th_\w+)\s*\(([^)]*)\)", plain):
        if not re.search(r"_dev(_|$)", name):
            continue
        ptrs = set()
        for prm in params.split(","):
            m = re.match(r"\s*(.*?)(\w+)\s*$", prm, flags=re.S)
            if not m:
                continue
            ptype, pname = m.group(1), m.group(2)
            st = re.search(r"\b(th_\w+)\b", ptype)
            if st and st.group(1) in structs:
                ptrs |= dev_fields(st.group(1))
            elif "*" in ptype and (pname.startswith("d_") or pname.endswith("_dev")):
                ptrs.add(pname)
        found[name] = ptrs
    return found


def test_table_names_every_device_pointer():
    """Every function of include/thesia_amd.h with a _dev name, and every DEVICE pointer it takes, is in ENTRIES (or the
    function in EXEMPT, with the reason), and every entry of the table is run by a test of this file."""
    found = header_device_pointers()
    assert len(found) >= 20 and found["th_calc_spec_batch_dev"] == {"wav", "spec", "d_minmax"}, found   # the parser sees the header
    assert found["th_spec_to_img_raster_batch_dev"] == {"img.spec", "img.img", "tiles", "d_range", "d_colormap"}
    assert found["th_audio_stats_dev"] == {"channels", "block_energy"}
    for fn, ptrs in sorted(found.items()):
        if fn in EXEMPT:
            continue
        assert fn in ENTRIES, f"{fn} takes DEVICE pointers {sorted(ptrs)} and is not in the table"
        assert ptrs == set(ENTRIES[fn]), (fn, sorted(ptrs), sorted(ENTRIES[fn]))
    assert set(ENTRIES) | set(EXEMPT) == set(found), set(ENTRIES) ^ set(found)
    assert set(COVERED) == set(ENTRIES), set(ENTRIES) - set(COVERED)
    # the header states the contract the table follows
    conv = _header().split("#ifndef THESIA_AMD_H")[0]
    assert "Alignment." in conv and "TH_ERR_INVALID_ARG" in conv


# ---------------------------------------------------------------- the arena
MARGIN = 4096   # bytes of sentinel in front of and behind every view
DEV = "cuda:0"


def _sentinel(dtype):
    from tests.test_gpu_streams import SENT1
    import torch
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([SENT1[torch.float32]], np.uint32).view(np.uint8)
    if dtype == np.float64:   # (the f32 pattern in both halves)
        return np.array([SENT1[torch.float32]] * 2, np.uint32).view(np.uint8)
    if dtype == np.uint16:
        return np.array([SENT1[torch.int16]], np.int16).view(np.uint8)
    assert dtype == np.uint8
    return np.array([SENT1[torch.uint8]], np.uint8)


class Arena:
    """One device allocation per case; add() carves views out of it, commit() fills and uploads it, check() reads it back and
    asserts that nothing outside the views' writable elements changed.
    ks: {pointer name of the table: offset k in elements}; shift: {pointer name: extra BYTES} (misaligned pointers)."""

    def __init__(self, ks=None, shift=None):
        self.ks, self.shift = dict(ks or {}), dict(shift or {})
        self.views, self.size, self.dev = {}, 0, None

    def add(self, role, key, dtype, n, data=None, writable=None, phase=0, unit=1):
        """A view of n elements of dtype for the table's pointer `role` at MARGIN + (k + phase) * unit elements.
        data: its content before the call (an input), else sentinel; writable: None (an input: nothing), True (all of it)
        or a bool mask over the n elements."""
        dtype = np.dtype(dtype)
        k = (self.ks.get(role, 0) + phase) * unit
        off = self.size + MARGIN + k * dtype.itemsize + self.shift.get(role, 0)
        end = off + n * dtype.itemsize
        if data is not None:
            data = np.ascontiguousarray(data, dtype).reshape(-1)
            assert data.size == n, (key, data.size, n)
        if writable is True:
            writable = np.ones(n, bool)
        self.views[key] = (dtype, self.size, off, n, data, writable)
        self.size = -(-(end + MARGIN) // 256) * 256
        return key

    def commit(self):
        import torch
        host = np.empty(self.size, np.uint8)
        may = np.zeros(self.size, bool)
        starts = sorted(v[1] for v in self.views.values()) + [self.size]
        for dtype, start, off, n, data, writable in self.views.values():
            stop = starts[starts.index(start) + 1]
            pat = _sentinel(dtype)
            host[start:stop] = np.tile(pat, (stop - start) // pat.size)
            if data is not None:
                host[off:off + data.nbytes] = data.view(np.uint8)
            if writable is not None:
                may[off:off + n * dtype.itemsize] = np.repeat(writable, dtype.itemsize)
        self.before, self.may = host, may
        self.dev = torch.from_numpy(host.copy()).to(DEV)
        self.base = self.dev.data_ptr()
        assert self.base % 256 == 0
        torch.cuda.synchronize()
        return self

    def ptr(self, key):
        return self.base + self.views[key][2]

    def check(self):
        """Read the arena back; every byte outside the writable elements is what it was (sentinel, or an input's data)."""
        import torch
        torch.cuda.synchronize()
        self.after = self.dev.cpu().numpy()
        bad = np.flatnonzero((self.after != self.before) & ~self.may)
        if bad.size:
            b = int(bad[0])
            key, (dtype, start, off, n, _, _) = max(((k, v) for k, v in self.views.items() if v[1] <= b), key=lambda kv: kv[1][1])
            raise AssertionError(f"stray write: {bad.size} bytes changed outside the extents of the call, the first in the "
                                 f"surrounding of view {key!r} at byte {b - off} relative to the view's start "
                                 f"(the view holds {n * dtype.itemsize} bytes; offsets {self.ks})")
        return self

    def get(self, key):
        dtype, _, off, n, _, _ = self.views[key]
        return self.after[off:off + n * dtype.itemsize].view(dtype).copy()


def rows_mask(n_rows, pitch, row_elems, owned=False):
    """(view length, writable mask) of n_rows rows of row_elems elements at `pitch`: [0, row_elems) of each row; the whole
    row including its padding only where the library owns it (exactly th_pitch_f32 / th_pitch_u16)."""
    if n_rows == 0:
        return 0, np.zeros(0, bool)
    if owned:
        return n_rows * pitch, np.ones(n_rows * pitch, bool)
    n = (n_rows - 1) * pitch + row_elems
    return n, (np.arange(n) % pitch) < row_elems


def rows_of(flat, n_rows, pitch, row_elems):
    """the n_rows x row_elems payload of a pitched view"""
    out = np.empty((n_rows, row_elems), flat.dtype)
    for r in range(n_rows):
        out[r] = flat[r * pitch:r * pitch + row_elems]
    return out


def same(a, b):
    if isinstance(a, (bytes, float, int)):
        return a == b or (isinstance(a, float) and a != a and b != b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


_BASE = {}    # key of a case -> the outputs of its all-zero-offset run
_LAST = {}    # "arena": the arena of the call in flight (test_misaligned_pointer_is_refused looks at it after the refusal)
_PLANS = {}   # route -> plan (closed with the context)


def drive(key, run, check, ks, loose=()):
    """Run one case: 1. against the oracle, 2. bit-identical to the all-zero-offset run of the same data (but `loose`)."""
    got = run(ks)
    check(got)
    if ks:
        if key not in _BASE:
            _BASE[key] = run({})
            check(_BASE[key])
        base = _BASE[key]
        assert set(got) == set(base)
        for name in got:
            if name not in loose:
                assert same(got[name], base[name]), f"{key}: output {name!r} at offsets {ks} differs from the one at offset 0"


@pytest.fixture(scope="module")
def ctx():
    import torch
    import thesia_amd as ta
    torch.cuda.init()
    c = ta.Context(0)
    yield c
    for plan in _PLANS.values():
        plan.close()
    _PLANS.clear()
    c.close()


def _lib():
    import thesia_amd as ta
    return ta.api.lib, ta.api.check


# ---------------------------------------------------------------- calc_spec on every route
def _routes():
    from tests.test_gpu_parity import F32_FLOOR
    from tests.test_gpu_streams import ROUTES
    r = dict(ROUTES)
    # the app's own 40 ms window: hop 480 ("phased" register reuse) and hop 441 ("dynamic": odd offsets) of the wave kernel
    r["phased-2048"] = (48000, 1920, 480, 2048, 0, 0, 0, "stft_wave_kernel", F32_FLOOR, (1000, 2048, 40017))
    r["dynamic-2048"] = (44100, 1764, 441, 2048, 0, 0, 0, "stft_wave_kernel", F32_FLOOR, (1000, 2048, 40017))
    assert sorted(r) == sorted(ROUTE_NAMES), set(r) ^ set(ROUTE_NAMES)   # every route of tests/test_gpu_streams.py, and the two modes
    return r


ROUTE_NAMES = ["generic-4", "generic-6144", "chirp-z-134", "wave-2048", "multi-512", "mel-banded-2048", "mel-moment-4096", "mel-rows-4096",
               "mel-rows-2048", "block-mel-8192", "subwave-32768", "phased-2048", "dynamic-2048"]
LONG_ROUTES = ("block-mel-8192", "subwave-32768")   # two phases instead of four: their frames are the slow ones
_ROUTE_DATA = {}


def _route_data(name):
    """(channel signals, [(dB, amp or None)]): shorter than n_fft, exactly n_fft, and the two rows of ONE planar 2 x N array with
    N % 4 != 0 (the reference's Array2 layout: the second row's phase differs from the first's)."""
    from oracle import oracle as orc
    from tests.synth import synth_track
    if name not in _ROUTE_DATA:
        sr, win, hop, n_fft, scale, n_mel, _, _, _, lens = _routes()[name]
        assert lens[2] % 4 != 0
        wavs = [synth_track(1300 + 7 * i + n_fft, sr, n) for i, n in enumerate(lens + (lens[2],))]
        fb = (orc.calc_mel_fb(sr, n_fft, n_mel) if n_mel else orc.calc_mel_fb_default(sr, n_fft)) if scale else None
        want = []
        for x in wavs:
            w, amp = orc.calc_spec(x, win, hop, n_fft, mel_fb=fb, return_amp=True)
            want.append((w, None if scale else amp))
        _ROUTE_DATA[name] = (wavs, want)
    return _ROUTE_DATA[name]


def _plan(ctx, name):
    import thesia_amd as ta
    if name in _PLANS:
        return _PLANS[name]
    sr, win, hop, n_fft, scale, n_mel, which, kernel, _, _ = _routes()[name]
    plan = ta.Plan(ctx, sr, win, hop, n_fft, ta.MEL if scale else ta.LINEAR, n_mel)
    if which:
        plan.set_kernel(which)
    assert plan.kernel_name.startswith(kernel) if kernel.endswith("_") else plan.kernel_name == kernel, (name, plan.kernel_name)
    if name == "mel-moment-4096":
        assert plan.mel_moments_info()["groups"] > 0
    _PLANS[name] = plan
    return plan


def _spec_pitch(H, layout):
    """dense rows | a pitch the library does not own (never written outside [0, H)) | exactly th_pitch_f32 (padding owned)"""
    import thesia_amd as ta
    own = ta.pitch_f32(H)
    if layout == "dense":
        return H, 0, own == H
    if layout == "foreign":
        p = H + 3 if H + 3 != own else H + 5
        return p, p, False
    return own, own, True


def run_calc_spec(ctx, route, ranged, ks, layout="dense", chans=(0, 1, 2, 3), shift=None):
    import thesia_amd as ta
    wavs, _ = _route_data(route)
    plan = _plan(ctx, route)
    H = plan.height
    pitch, desc_pitch, owned = _spec_pitch(H, layout)
    ar = Arena(ks, shift)
    n_long = wavs[2].size
    ar.add("wav", "w0", np.float32, wavs[0].size, wavs[0])
    ar.add("wav", "w1", np.float32, wavs[1].size, wavs[1])
    ar.add("wav", "planar", np.float32, 2 * n_long, np.stack([wavs[2], wavs[3]]))
    Ts = [plan.n_frames(x.size) for x in wavs]
    for i in chans:
        n, mask = rows_mask(Ts[i], pitch, H, owned)
        ar.add("spec", f"s{i}", np.float32, n, writable=mask)
    ar.add("d_minmax", "mm", np.float32, 2 * len(chans), writable=True)
    if ranged:
        ar.add("d_range", "rng", np.float32, 2, writable=True)
    ar.commit()
    wptr = [ar.ptr("w0"), ar.ptr("w1"), ar.ptr("planar"), ar.ptr("planar") + 4 * n_long]
    descs = (ta.ChanDesc * len(chans))(*[ta.ChanDesc(wptr[i], ar.ptr(f"s{i}"), wavs[i].size, Ts[i], desc_pitch) for i in chans])
    _LAST["arena"] = ar
    if ranged:
        plan.calc_spec_batch_ranged_dev(descs, ar.ptr("mm"), 100.0, ar.ptr("rng"))
    else:
        plan.calc_spec_batch_dev(descs, ar.ptr("mm"))
    ctx.synchronize()
    ar.check()
    out = {f"spec{i}": rows_of(ar.get(f"s{i}"), Ts[i], pitch, H) for i in chans}
    out["mm"] = ar.get("mm").reshape(-1, 2)
    if ranged:
        out["rng"] = ar.get("rng")
    return out


def check_calc_spec(route, got, chans=(0, 1, 2, 3)):
    from oracle import oracle as orc
    from tests.test_gpu_parity import assert_spec_close
    _, want = _route_data(route)
    floor = _routes()[route][8]
    mm = got["mm"]
    for j, i in enumerate(chans):
        g, (w, amp) = got[f"spec{i}"], want[i]
        assert_spec_close(g, w, amp, floor=floor)
        assert mm[j, 0] == g.min() and mm[j, 1] == g.max(), (route, i, mm[j], g.min(), g.max())
    if "rng" in got:
        lo, hi = orc.global_db_range(mm[:, 0], mm[:, 1], 100.0)
        assert (got["rng"][0], got["rng"][1]) == (np.float32(lo), np.float32(hi)), (route, got["rng"], lo, hi)


def _calc_spec_cases():
    """(route, id, ks, layout).  wav / d_minmax over their offsets with the spec layouts in turn; spec over its offsets in
    each of the three layouts; the long transforms at two phases instead of four."""
    out = []
    lay = ("dense", "foreign", "owned")
    for route in ROUTE_NAMES:
        offs = (1,) if route in LONG_ROUTES else (1, 2, 3)
        for k in offs:
            out.append((route, f"wav+{k}", {"wav": k}, lay[k % 3]))
            out.append((route, f"d_minmax+{k}", {"d_minmax": k}, lay[(k + 1) % 3]))
        for k in ((3,) if route in LONG_ROUTES else (1, 2, 3)):
            for layout in (lay[1:] if route in LONG_ROUTES else lay):
                out.append((route, f"spec+{k}-{layout}", {"spec": k}, layout))
        out.append((route, "all-owned", {"wav": 3, "spec": 1, "d_minmax": 2}, "owned"))
        out.append((route, "all-foreign", {"wav": 2, "spec": 3, "d_minmax": 1}, "foreign"))
    return [pytest.param(r, ks, layout, id=f"{r}-{i}") for r, i, ks, layout in out]


@gpu
@covers("th_calc_spec_batch_dev")
@pytest.mark.parametrize("route,ks,layout", _calc_spec_cases())
def test_calc_spec_batch_dev(ctx, route, ks, layout):
    """Boundary frames, edge jobs and interior chunks all read from the shifted base; rows written at a shifted base in a dense,
    a foreign and the library's own pitch.  The rows equal those of the dense, all-aligned run bit for bit."""
    drive(("spec", route), lambda k: run_calc_spec(ctx, route, False, k, layout if k else "dense"), lambda g: check_calc_spec(route, g), ks)


@gpu
@covers("th_calc_spec_batch_ranged_dev")
@pytest.mark.parametrize("ks", cases("th_calc_spec_batch_ranged_dev"))
@pytest.mark.parametrize("chans", [(0, 1, 2, 3), (3,)], ids=["batch", "one-channel"])
def test_calc_spec_batch_ranged_dev(ctx, ks, chans):
    """...and the batch's dB range in the same call; a one-channel batch folds the range into the wave kernel's follow-up
    launch (here the channel is the planar array's second row)."""
    drive(("ranged", chans), lambda k: run_calc_spec(ctx, "wave-2048", True, k, "foreign" if k else "dense", chans),
          lambda g: check_calc_spec("wave-2048", g, chans), ks)


@gpu
@covers("th_calc_spec_batch_ranged_dev")
@pytest.mark.parametrize("route", [r for r in ROUTE_NAMES if r != "wave-2048"])
def test_calc_spec_batch_ranged_dev_every_route(ctx, route):
    drive(("ranged", route), lambda k: run_calc_spec(ctx, route, True, k, "owned" if k else "dense"), lambda g: check_calc_spec(route, g),
          {"wav": 1, "spec": 2, "d_minmax": 3, "d_range": 1})


# ---------------------------------------------------------------- the three range reductions
def _mm(n):
    rng = np.random.default_rng(3 + n)
    mm = rng.uniform(-120, 5, (n, 2)).astype(np.float32)
    mm[rng.integers(0, n), 0] = -np.inf
    return mm


def run_reduce(ctx, entry, n, ks, shift=None):
    mm = _mm(n)
    ar = Arena(ks, shift)
    pair = np.array([mm[:, 0].min(), -mm[:, 1].max()], np.float32)
    if entry == "th_global_db_range_dev":
        ar.add("d_min_negmax", "in", np.float32, 2, pair)
    else:
        ar.add("d_minmax", "in", np.float32, 2 * n, mm)
    outs = {"th_minmax_reduce_dev": ["d_out"], "th_global_db_range_dev": ["d_range"], "th_minmax_reduce_range_dev": ["d_min_negmax", "d_range"]}[entry]
    for o in outs:
        ar.add(o, o, np.float32, 2, writable=True)
    ar.commit()
    _LAST["arena"] = ar
    if entry == "th_minmax_reduce_dev":
        ctx.minmax_reduce_dev(ar.ptr("in"), n, ar.ptr("d_out"))
    elif entry == "th_global_db_range_dev":
        ctx.global_db_range_dev(ar.ptr("in"), 80.0, ar.ptr("d_range"))
    else:
        ctx.minmax_reduce_range_dev(ar.ptr("in"), n, 80.0, ar.ptr("d_range"), ar.ptr("d_min_negmax"))
    ctx.synchronize()
    ar.check()
    return {o: ar.get(o) for o in outs}


def check_reduce(n, got):
    from oracle import oracle as orc
    mm = _mm(n)
    for name, g in got.items():
        if name == "d_range":
            lo, hi = orc.global_db_range(mm[:, 0], mm[:, 1], 80.0)
            assert (g[0], g[1]) == (np.float32(lo), np.float32(hi)), (n, g, lo, hi)
        else:
            assert g[0] == mm[:, 0].min() and g[1] == -mm[:, 1].max(), (n, name, g)


def _reduce_cases():
    return [pytest.param(e, ks.values[0], id=f"{e}-{ks.id}") for e in ("th_minmax_reduce_dev", "th_global_db_range_dev", "th_minmax_reduce_range_dev")
            for ks in cases(e)]


@gpu
@covers("th_minmax_reduce_dev", "th_global_db_range_dev", "th_minmax_reduce_range_dev")
@pytest.mark.parametrize("entry,ks", _reduce_cases())
@pytest.mark.parametrize("n", [1, 5, 257])
def test_range_reductions(ctx, entry, ks, n):
    drive((entry, n), lambda k: run_reduce(ctx, entry, n, k), lambda g: check_reduce(n, g), ks)


# ---------------------------------------------------------------- quantiser
# (T, H, i_start, i_end, colormap length, spec layout, image layout): the shapes of test_spec_to_img_bit_exact — i_start odd
# and even, rows >= H (zero rows) — with NaN / +-inf / rounding-boundary values.  padded: th_pitch_f32 (an even pitch > H: the
# 8-byte loads are the base's to decide); owned: th_pitch_u16; foreign: an even pitch of a wider surface (dword stores decided by
# the base alone) or an odd one.
IMG_SHAPES = [(1, 1, 0, 1, 258, "dense", "dense"), (63, 65, 0, 65, 258, "padded", "owned"), (300, 1025, 0, 1025, 258, "padded", "foreign"),
              (257, 128, 0, 140, 258, "foreign", "owned"), (129, 513, 0, 1026, 4, "dense", "dense"), (70, 70, 3, 50, None, "padded", "foreign"),
              (1000, 37, 0, 37, 258, "padded", "dense")]


def _img_spec(T, H):
    rng = np.random.default_rng(T * 7 + H)
    spec = rng.uniform(-140, 10, (T, H)).astype(np.float32)
    spec.ravel()[rng.integers(0, spec.size, 5)] = -np.inf
    spec.ravel()[rng.integers(0, spec.size, 3)] = np.nan
    spec.ravel()[rng.integers(0, spec.size, 2)] = np.inf
    edge = [-100.0, 0.0, -50.0, -100.0 + 100.0 * 0.5 / 65281]
    spec.ravel()[:min(4, spec.size)] = edge[:min(4, spec.size)]
    return spec


def _img_layouts(T, H, rows, sl, il):
    """-> (spec pitch, spec view floats, host spec rows -> flat) , (img pitch, view length, mask)"""
    import thesia_amd as ta
    sp = {"dense": H, "padded": ta.pitch_f32(H), "foreign": H + 3}[sl]
    ip = {"dense": T, "owned": ta.pitch_u16(T), "foreign": T + 6 if (T + 6) % 64 else T + 8}[il]
    n_img, mask = rows_mask(rows, ip, T, owned=ip == ta.pitch_u16(T))
    return sp, ip, n_img, mask


def _pitched(a, pitch, whole_rows):
    """rows of `a` laid out at `pitch` (7.0 in the padding, as a wider array's own data)"""
    T, H = a.shape
    out = np.full((T, pitch), 7.0, a.dtype)
    out[:, :H] = a
    flat = out.reshape(-1)
    return flat if whole_rows else flat[:(T - 1) * pitch + H]


def run_spec_to_img(ctx, entry, shapes, rng_db, ks, shift=None):
    """th_spec_to_img_dev (one dense image per call), th_spec_to_img_batch_dev (host range), ..._ranged (device range)"""
    from thesia_amd import _ffi
    lib, check = _lib()
    single = entry == "th_spec_to_img_dev"
    rs, ri = ("d_spec", "d_img") if single else ("spec", "img")
    ar = Arena(ks, shift)
    lay = []
    for j, (T, H, i0, i1, cm, sl, il) in enumerate(shapes):
        if single:
            sl = il = "dense"
        sp, ip, n_img, mask = _img_layouts(T, H, i1 - i0, sl, il)
        ar.add(rs, f"spec{j}", np.float32, T * sp if sl == "padded" else (T - 1) * sp + H, _pitched(_img_spec(T, H), sp, sl == "padded"), phase=j)
        ar.add(ri, f"img{j}", np.uint16, n_img, writable=mask, phase=j)
        lay.append((sp, ip))
    if entry.endswith("_ranged"):
        ar.add("d_range", "rng", np.float32, 2, np.array(rng_db, np.float32))
    ar.commit()
    _LAST["arena"] = ar
    cm = shapes[0][4]
    if single:
        T, H, i0, i1 = shapes[0][:4]
        check(lib.th_spec_to_img_dev(ctx.handle, ar.ptr("spec0"), T, H, i0, i1, rng_db[0], rng_db[1], cm or 0, ar.ptr("img0")))
    else:
        descs = [_ffi.ImgDesc(ar.ptr(f"spec{j}"), ar.ptr(f"img{j}"), T, H, i0, i1, sp, ip) for j, ((T, H, i0, i1, *_r), (sp, ip)) in enumerate(zip(shapes, lay))]
        if entry.endswith("_ranged"):
            ctx.spec_to_img_batch_ranged(descs, ar.ptr("rng"), cm or 0)
        else:
            ctx.spec_to_img_batch(descs, rng_db[0], rng_db[1], cm or 0)
    ctx.synchronize()
    ar.check()
    return {f"img{j}": rows_of(ar.get(f"img{j}"), i1 - i0, ip, T) for j, ((T, H, i0, i1, *_r), (sp, ip)) in enumerate(zip(shapes, lay))}


def check_spec_to_img(shapes, rng_db, got):
    from oracle import oracle as orc
    cm = shapes[0][4]
    for j, (T, H, i0, i1, *_r) in enumerate(shapes):
        if rng_db[0] == rng_db[1] == -np.inf:
            assert got[f"img{j}"].shape == (i1 - i0, T) and not got[f"img{j}"].any(), j     # drawing.rs:16-18
        else:
            assert np.array_equal(got[f"img{j}"], orc.convert_spectrogram_to_img(_img_spec(T, H), (i0, i1), rng_db, cm)), (j, T, H)


SILENT = (-np.inf, -np.inf)


@gpu
@covers("th_spec_to_img_dev")
@pytest.mark.parametrize("ks", cases("th_spec_to_img_dev"))
@pytest.mark.parametrize("shape", [1, 4, 5, 6], ids=lambda j: "x".join(str(v) for v in IMG_SHAPES[j][:4]))
def test_spec_to_img_dev(ctx, shape, ks):
    shapes = [IMG_SHAPES[shape]]
    for rng_db in ((-100.0, 0.0),) + ((SILENT,) if shape == 5 else ()):
        drive(("img1", shape, rng_db), lambda k: run_spec_to_img(ctx, "th_spec_to_img_dev", shapes, rng_db, k),
              lambda g: check_spec_to_img(shapes, rng_db, g), ks)


@gpu
@covers("th_spec_to_img_batch_dev", "th_spec_to_img_batch_dev_ranged")
@pytest.mark.parametrize("rng_db", [(-100.0, 0.0), SILENT], ids=["range", "all-neg-inf"])
@pytest.mark.parametrize("entry,ks", [pytest.param(e, ks.values[0], id=f"{e}-{ks.id}") for e in ("th_spec_to_img_batch_dev", "th_spec_to_img_batch_dev_ranged")
                                      for ks in cases(e)])
def test_spec_to_img_batch_dev(ctx, entry, ks, rng_db):
    """Seven images in one batch, image j one more element off than image j - 1 (mixed phases in one launch); the all -inf
    range zero-fills each sub-rectangle and nothing else (a 2-D memset with the host range, the kernel with the device range)."""
    shapes = [s[:4] + (258,) + s[5:] for s in IMG_SHAPES]
    drive((entry, rng_db), lambda k: run_spec_to_img(ctx, entry, shapes, rng_db, k), lambda g: check_spec_to_img(shapes, rng_db, g), ks)


# ---------------------------------------------------------------- quantise + raster in one pass
CM_LEN = 258
# (T, hh = spec height, i_start, i_end, spec layout, image layout): tile widths with and without whole quads, rows >= hh
FUSED_SHAPES = [(700, 347, 0, 347, "padded", "owned"), (1030, 300, 5, 521, "dense", "foreign"), (37, 9, 0, 9, "foreign", "dense")]


def _cmap(n=CM_LEN):
    return bytes(np.random.default_rng(5).integers(0, 256, n * 4, dtype=np.uint8))


def _tile_geoms(W, H):
    import thesia_amd as ta
    return [(tx, ty, ta.spectrogram_tile_geometry(W, H, 0, 0, tx, ty)) for tx in range(-(-W // 512)) for ty in range(-(-H // 512))]


def run_fused(ctx, rng_db, ks, shift=None):
    from thesia_amd import _ffi
    ar = Arena(ks, shift)
    items, lay = [], []
    for j, (T, hh, i0, i1, sl, il) in enumerate(FUSED_SHAPES):
        sp, ip, n_img, mask = _img_layouts(T, hh, i1 - i0, sl, il)
        ar.add("img.spec", f"spec{j}", np.float32, T * sp if sl == "padded" else (T - 1) * sp + hh, _pitched(_img_spec(T, hh), sp, sl == "padded"), phase=j)
        ar.add("img.img", f"img{j}", np.uint16, n_img, writable=mask, phase=j)
        geoms = _tile_geoms(T, i1 - i0)
        skip = 1 if j == 1 else None                          # a NULL tile: skipped
        offs, off = [], 0
        for t, (_, _, g) in enumerate(geoms):
            offs.append(None if t == skip else off)
            off += 0 if t == skip else g.width * g.height      # packed back to back: bases only 4-byte aligned
        ar.add("tiles", f"tiles{j}", np.uint8, off * 4, writable=True, phase=j, unit=4)
        lay.append((sp, ip, geoms, offs))
    ar.add("d_range", "rng", np.float32, 2, np.array(rng_db, np.float32))
    ar.add("d_colormap", "cmap", np.uint8, CM_LEN * 4, np.frombuffer(_cmap(), np.uint8), unit=4)
    ar.commit()
    _LAST["arena"] = ar
    for j, ((T, hh, i0, i1, *_r), (sp, ip, geoms, offs)) in enumerate(zip(FUSED_SHAPES, lay)):
        items.append((_ffi.ImgDesc(ar.ptr(f"spec{j}"), ar.ptr(f"img{j}"), T, hh, i0, i1, sp, ip),
                      [0 if o is None else ar.ptr(f"tiles{j}") + 4 * o for o in offs]))
    descs = ctx.make_img_tiles_descs(items)
    ctx.spec_to_img_raster_batch(descs, ar.ptr("cmap"), CM_LEN, d_range=ar.ptr("rng"))
    ctx.synchronize()
    ar.check()
    out = {}
    for j, ((T, hh, i0, i1, *_r), (sp, ip, geoms, offs)) in enumerate(zip(FUSED_SHAPES, lay)):
        out[f"img{j}"] = rows_of(ar.get(f"img{j}"), i1 - i0, ip, T)
        flat = ar.get(f"tiles{j}")
        for (tx, ty, g), o in zip(geoms, offs):
            if o is not None:
                out[f"tile{j}-{tx}-{ty}"] = flat[4 * o:4 * (o + g.width * g.height)]
    return out


def check_fused(rng_db, got):
    from oracle import oracle as orc
    cmap = _cmap()
    n_tiles = 0
    for j, (T, hh, i0, i1, *_r) in enumerate(FUSED_SHAPES):
        if rng_db == SILENT:
            want = np.zeros((i1 - i0, T), np.uint16)
        else:
            want = orc.convert_spectrogram_to_img(_img_spec(T, hh), (i0, i1), rng_db, CM_LEN)
        assert np.array_equal(got[f"img{j}"], want), j
        for tx, ty, g in _tile_geoms(T, i1 - i0):
            if f"tile{j}-{tx}-{ty}" in got:
                assert got[f"tile{j}-{tx}-{ty}"].tobytes() == orc.encode_spectrogram_tile(want, cmap, 1, 0, 0, tx, ty)[40:], (j, tx, ty)
                n_tiles += 1
    assert n_tiles == sum(len(_tile_geoms(T, i1 - i0)) for T, _, i0, i1, *_r in FUSED_SHAPES) - 1


@gpu
@covers("th_spec_to_img_raster_batch_dev")
@pytest.mark.parametrize("rng_db", [(-100.0, -3.5), SILENT], ids=["range", "all-neg-inf"])
@pytest.mark.parametrize("ks", cases("th_spec_to_img_raster_batch_dev"))
def test_spec_to_img_raster_batch_dev(ctx, ks, rng_db):
    """Three images in one batch at different phases (image j one element / pixel further off), tiles packed back to back behind
    a lead of k pixels, one NULL tile, the range and the colour map on the device at shifted bases."""
    drive(("fused", rng_db), lambda k: run_fused(ctx, rng_db, k), lambda g: check_fused(rng_db, g), ks)


# ---------------------------------------------------------------- raster
RASTER_SHAPES = [(1100, 700, "owned"), (1031, 530, "dense")]   # (every tile width a multiple of 4 | not)


def _u16_img(W, H):
    return np.random.default_rng(W * 31 + H).integers(0, 65536, (H, W), dtype=np.uint16)


def run_raster(ctx, W, H, il, ks, shift=None):
    import thesia_amd as ta
    from thesia_amd import _ffi
    img = _u16_img(W, H)
    pitch = ta.pitch_u16(W) if il == "owned" else W
    ar = Arena(ks, shift)
    ar.add("img", "img", np.uint16, H * pitch, np.pad(img, ((0, 0), (0, pitch - W))))
    geoms = _tile_geoms(W, H)
    assert il != "owned" or all(g.origin_x % 4 == 0 and g.width % 4 == 0 for _, _, g in geoms)   # only the base decides the source path
    offs = np.cumsum([0] + [g.width * g.height for _, _, g in geoms])
    ar.add("rgba", "rgba", np.uint8, int(offs[-1]) * 4, writable=True, unit=4)
    ar.add("d_colormap", "cmap", np.uint8, CM_LEN * 4, np.frombuffer(_cmap(), np.uint8), unit=4)
    ar.commit()
    _LAST["arena"] = ar
    descs = [_ffi.RasterDesc(ar.ptr("img"), ar.ptr("rgba") + 4 * int(o), W, H, g.origin_x, g.origin_y, g.width, g.height, pitch, 0)
             for (_, _, g), o in zip(geoms, offs)]
    ctx.raster_tiles(descs, ar.ptr("cmap"), CM_LEN)
    ctx.synchronize()
    ar.check()
    flat = ar.get("rgba")
    return {f"tile-{tx}-{ty}": flat[4 * int(o):4 * int(o + g.width * g.height)] for (tx, ty, g), o in zip(geoms, offs)}


def check_raster(W, H, got):
    from oracle import oracle as orc
    img, cmap = _u16_img(W, H), _cmap()
    for tx, ty, _ in _tile_geoms(W, H):
        assert got[f"tile-{tx}-{ty}"].tobytes() == orc.encode_spectrogram_tile(img, cmap, 1, 0, 0, tx, ty)[40:], (tx, ty)


@gpu
@covers("th_raster_tiles_dev")
@pytest.mark.parametrize("ks", cases("th_raster_tiles_dev"))
@pytest.mark.parametrize("W,H,il", RASTER_SHAPES)
def test_raster_tiles_dev(ctx, W, H, il, ks):
    drive(("raster", W), lambda k: run_raster(ctx, W, H, il, k), lambda g: check_raster(W, H, g), ks)


# ---------------------------------------------------------------- tiles returned to the host
TILE_IMG = (700, 1100)   # (height, width)
TILE_REQS = [(0, 0, 1, 1), (0, 0, 2, 0), (1, 0, 1, 0), (2, 1, 0, 0)]   # level (0, 0): the raster alone; LOD: two resample passes in front


def run_spectrogram_tile(ctx, foreign, ks, shift=None):
    H, W = TILE_IMG
    img = _u16_img(W, H)
    pitch = W + 6 if foreign else W
    ar = Arena(ks, shift)
    ar.add("d_img", "img", np.uint16, (H - 1) * pitch + W, _pitched(img, pitch, False))
    ar.commit()
    _LAST["arena"] = ar
    out = {str(r): ctx.encode_spectrogram_tile_dev(ar.ptr("img"), H, W, _cmap(), 3, *r, img_pitch=pitch if foreign else 0) for r in TILE_REQS}
    ar.check()
    return out


_TILE_WANT = {}


def check_spectrogram_tile(got):
    from oracle import oracle as orc
    H, W = TILE_IMG
    for r in TILE_REQS:
        if r not in _TILE_WANT:
            _TILE_WANT[r] = orc.encode_spectrogram_tile(_u16_img(W, H), _cmap(), 3, *r)
        assert got[str(r)] == _TILE_WANT[r], r


@gpu
@covers("th_encode_spectrogram_tile_dev")
@pytest.mark.parametrize("ks", cases("th_encode_spectrogram_tile_dev"))
@pytest.mark.parametrize("foreign", [False, True], ids=["dense", "pitch"])
def test_encode_spectrogram_tile_dev(ctx, foreign, ks):
    drive(("tile", foreign), lambda k: run_spectrogram_tile(ctx, foreign, k), check_spectrogram_tile, ks)


# ---------------------------------------------------------------- waveform
N_WAV = 300_001
WAVE_LEVELS = (0, 1, 4, 9)


def _wave():
    from tests.synth import synth_track
    if "x" not in _TILE_WANT:
        _TILE_WANT["x"] = synth_track(5, 48000, N_WAV)
    return _TILE_WANT["x"]


def _wave_jobs():
    import thesia_amd as ta
    jobs = []
    for level in WAVE_LEVELS:
        n_tiles = -(-(-(-N_WAV // (1 << level))) // 1024)
        for tile in sorted({0, n_tiles // 2, n_tiles - 1}):   # (each level's last tile is partial)
            start, bins, _ = ta.waveform_tile_geometry(N_WAV, level, tile)
            jobs.append((level, tile, start, bins))
    return jobs


def run_waveform_tile(ctx, ks, shift=None):
    x = _wave()
    ar = Arena(ks, shift)
    ar.add("d_wav", "wav", np.float32, N_WAV, x)
    ar.commit()
    _LAST["arena"] = ar
    out = {f"{level}-{tile}": ctx.encode_waveform_tile_dev(ar.ptr("wav"), N_WAV, 42, level, tile) for level, tile, _, _ in _wave_jobs()}
    ar.check()
    return out


def check_waveform_tile(got):
    from oracle import oracle as orc
    from tests.test_gpu_streams import _assert_bins
    x = _wave()
    peak = float(np.abs(x).max())
    for level, tile, _, bins in _wave_jobs():
        want, g = orc.encode_waveform_tile(x, 42, level, tile), got[f"{level}-{tile}"]
        assert g[:24] == want[:24] and len(g) == len(want), (level, tile)
        _assert_bins(np.frombuffer(g[24:], np.float32).reshape(-1, 3), np.frombuffer(want[24:], np.float32).reshape(-1, 3), level, peak, (level, tile))


@gpu
@covers("th_encode_waveform_tile_dev")
@pytest.mark.parametrize("ks", cases("th_encode_waveform_tile_dev"))
def test_encode_waveform_tile_dev(ctx, ks):
    drive("wtile", lambda k: run_waveform_tile(ctx, k), check_waveform_tile, ks)


def run_waveform_tiles(ctx, ks, shift=None):
    from thesia_amd import _ffi
    x = _wave()
    ar = Arena(ks, shift)
    ar.add("wav", "wav", np.float32, N_WAV, x)
    jobs = _wave_jobs()
    for j, (_, _, _, bins) in enumerate(jobs):
        ar.add("bins", f"bins{j}", np.float32, 3 * bins, writable=True, phase=j)   # (bin_count x 3 floats, each job at its own phase)
    ar.commit()
    _LAST["arena"] = ar
    ctx.waveform_tiles([_ffi.WaveDesc(ar.ptr("wav"), ar.ptr(f"bins{j}"), N_WAV, start, level, bins) for j, (level, _, start, bins) in enumerate(jobs)])
    ctx.synchronize()
    ar.check()
    return {f"{level}-{tile}": ar.get(f"bins{j}").reshape(-1, 3) for j, (level, tile, _, _) in enumerate(jobs)}


def check_waveform_tiles(got):
    from tests.test_gpu_streams import _assert_bins, _want_bins
    x = _wave()
    peak = float(np.abs(x).max())
    for level, tile, _, _ in _wave_jobs():
        _assert_bins(got[f"{level}-{tile}"], _want_bins(x, level, tile), level, peak, (level, tile))


@gpu
@covers("th_waveform_tiles_dev")
@pytest.mark.parametrize("ks", cases("th_waveform_tiles_dev"))
def test_waveform_tiles_dev(ctx, ks):
    drive("wtiles", lambda k: run_waveform_tiles(ctx, k), check_waveform_tiles, ks)


# lengths: whole lanes of 16 samples in whole blocks of 4096 | a partial last lane | shorter than one lane — so that both sides of
# the kernel's `valid == 16` run at every phase; 14 levels: the base pass (0 .. 12) and one tree pass
PYR_LENS = (3 * 4096, 2 * 4096 + 5 * 16 + 7, 11)
PYR_LEVELS = 14


def _pyr_x(n):
    from tests.synth import synth_track
    return synth_track(8 + n, 44100, n)


def run_pyramid(ctx, ks, shift=None):
    import thesia_amd as ta
    from thesia_amd import _ffi
    ar = Arena(ks, shift)
    jobs = []
    for i, n in enumerate(PYR_LENS):
        ar.add("wav", f"wav{i}", np.float32, n, _pyr_x(n), phase=i)
        for first in (0, 1, 2):
            total = ta.api.pyramid_offset(n, PYR_LEVELS) - ta.api.pyramid_offset(n, first)
            ar.add("out", f"out{i}-{first}", np.float32, total, writable=True, phase=i + first)
            jobs.append((i, n, first))
    ar.commit()
    _LAST["arena"] = ar
    ctx.waveform_pyramid_dev([_ffi.PyramidDesc(ar.ptr(f"wav{i}"), ar.ptr(f"out{i}-{first}"), n, PYR_LEVELS, first) for i, n, first in jobs])
    ctx.synchronize()
    ar.check()
    out = {}
    for i, n, first in jobs:
        flat, base = ar.get(f"out{i}-{first}"), ta.api.pyramid_offset(n, first)
        for level in range(first, PYR_LEVELS):
            a = ta.api.pyramid_offset(n, level) - base
            out[f"{n}-{first}-{level}"] = flat[a:a + 3 * ta.api.pyramid_bins(n, level)].reshape(-1, 3)
    return out


def check_pyramid(got):
    from tests.test_gpu_streams import _assert_bins, _want_bins
    for n in PYR_LENS:
        x = _pyr_x(n)
        peak = float(np.abs(x).max())
        for first in (0, 1, 2):
            for level in range(first, PYR_LEVELS):
                lv = got[f"{n}-{first}-{level}"]
                assert lv.shape[0] == -(-n // (1 << level)), (n, first, level)
                for t in range(-(-lv.shape[0] // 1024)):
                    _assert_bins(lv[1024 * t:1024 * (t + 1)], _want_bins(x, level, t), level, peak, (n, first, level, t))


@gpu
@covers("th_waveform_pyramid_dev")
@pytest.mark.parametrize("ks", cases("th_waveform_pyramid_dev"))
def test_waveform_pyramid_dev(ctx, ks):
    """Nine pyramids in one call (three lengths x first_level 0, 1, 2), channel i and its outputs i (+ first_level) elements further
    off: level 0 is written with 16-byte stores only where `out` lies on that grid, dword stores elsewhere."""
    drive("pyramid", lambda k: run_pyramid(ctx, k), check_pyramid, ks)


# ---------------------------------------------------------------- channel statistics
STATS_LENS = (5, 15, 16, 160, 4095, 4096, 4097, 2 * 4096 - 1, 2 * 4096 + 1, 100_003)


def _stats_x(n):
    rng = np.random.default_rng(17 + n)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    x[rng.integers(0, n)] = -1.5 if n % 2 else 1.25
    return x


def run_channel_stats(ctx, ks, shift=None):
    from thesia_amd import _ffi
    ar = Arena(ks, shift)
    for n in STATS_LENS:
        ar.add("wav", f"wav{n}", np.float32, n, _stats_x(n))
    ar.commit()
    _LAST["arena"] = ar
    ss, pk = ctx.channel_stats_dev([_ffi.StatsDesc(ar.ptr(f"wav{n}"), n) for n in STATS_LENS])
    ar.check()
    return {"sum_squares": ss, "abs_max": pk}


def check_channel_stats(got):
    from oracle import oracle as orc
    from tests.test_gpu_parity import CHANNEL_STATS_SUM_REL
    for n, s, p in zip(STATS_LENS, got["sum_squares"], got["abs_max"]):
        x = _stats_x(n)
        want_s = orc.sum_squares(x)
        assert p == orc.abs_max(x), (n, p)
        assert abs(s - want_s) <= CHANNEL_STATS_SUM_REL * max(want_s, 1e-30), (n, s, want_s)


@gpu
@covers("th_channel_stats_dev")
@pytest.mark.parametrize("ks", cases("th_channel_stats_dev"))
def test_channel_stats_dev(ctx, ks):
    """The unaligned side sums the squares of a thread's 16 samples one after the other, the aligned side pairwise: sum_squares
    is held to the reference bound only; the peak is exact either way."""
    drive("stats", lambda k: run_channel_stats(ctx, k), check_channel_stats, ks, loose=("sum_squares",))


# ---------------------------------------------------------------- loudness
def _audio_tracks():
    """[(C, sr, n, kind, x)]: the very tracks of test_block_energies_match_restatement_ragged_batch — C = 1 .. 8, rates 8 k .. 192 k,
    lengths at the block edges, a DC-heavy 192 kHz track, a NaN sample, an empty track — from the same generator in the same
    order: which VALUES meet _check_track's bar is that test's matter (its bar follows the f64 filter's rounding on the very
    signal, and another draw of the 96 kHz DC track misses it by a tenth at an aligned base); this one varies the ADDRESSES.
    Every track is ONE planar C x n array, so with n % 4 != 0 its channels have mixed phases."""
    from tests import loudness_ref as ref
    from tests.test_gpu_loudness import _signal
    if "audio" not in _TILE_WANT:
        rng = np.random.default_rng(5)
        specs = []
        for sr in (8000, 11025, 16000, 44100, 48000, 96000, 192000):
            s, L = ref.s100(sr), 4 * ref.s100(sr)
            specs += [(1, sr, L - 1, "noise"), (2, sr, L, "dc"), (3, sr, L + s - 1, "clipped"), (4, sr, L + s, "noise")]
        specs += [(5, 48000, 3 * 48000 + 7, "dc"), (6, 44100, 2 * 44100, "clipped"), (7, 16000, 3 * 16000, "noise"),
                  (8, 11025, 2 * 11025 + 3, "dc"), (2, 48000, 2 * 48000, "nan"), (1, 192000, 192000 + 5, "dc"), (1, 22050, 0, "noise")]
        _TILE_WANT["audio"] = [(C, sr, n, kind, _signal(rng, C, n, kind)) for C, sr, n, kind in specs]
    return _TILE_WANT["audio"]


def run_audio_stats(ctx, ks, shift=None):
    from tests import loudness_ref as ref
    ar = Arena(ks, shift)
    specs = _audio_tracks()
    for j, (C, sr, n, kind, x) in enumerate(specs):
        ar.add("channels", f"x{j}", np.float32, C * n, x, phase=j)
        ar.add("block_energy", f"e{j}", np.float64, ref.n_blocks(n, sr), writable=True, phase=j)   # n_blocks doubles
    ar.commit()
    _LAST["arena"] = ar
    st = ctx.audio_stats_dev([([ar.ptr(f"x{j}") + 4 * c * n for c in range(C)], n, sr, ar.ptr(f"e{j}")) for j, (C, sr, n, _, _) in enumerate(specs)])
    ar.check()
    out = {}
    for j, s in enumerate(st):
        out[f"e{j}"] = ar.get(f"e{j}")
        out.update({f"{k}{j}": float(v) for k, v in s.items()})
    return out


_REF_E = {}


def check_audio_stats(got):
    from tests import loudness_ref as ref
    from tests.test_gpu_loudness import _check_track
    real = ref.block_energies

    def memo(x, sr, dtype=np.float64):   # (the restatement is a per-sample Python loop: once per track and precision)
        key = (x.tobytes(), x.shape, sr, np.dtype(dtype).name)
        if key not in _REF_E:
            _REF_E[key] = real(x, sr, dtype)
        return _REF_E[key]

    ref.block_energies = memo
    try:
        for j, (C, sr, n, kind, x) in enumerate(_audio_tracks()):
            st = {k: got[f"{k}{j}"] for k in ("global_lufs", "rms_dB", "max_peak", "max_peak_dB")}
            _check_track(x, sr, st, got[f"e{j}"], (C, sr, n, kind))
    finally:
        ref.block_energies = real


@gpu
@covers("th_audio_stats_dev")
@pytest.mark.parametrize("ks", cases("th_audio_stats_dev"))
def test_audio_stats_dev(ctx, ks):
    """The K-weighting pipeline stages its chunks in another layout when a channel is not 16-byte aligned, and takes the
    statistics in another order: block energies, loudness and peak bit for bit those of the aligned run, rms_dB to the bound
    of _check_track."""
    drive("audio", lambda k: run_audio_stats(ctx, k), check_audio_stats, ks,
          loose=tuple(f"rms_dB{j}" for j in range(len(_audio_tracks()))))


# ---------------------------------------------------------------- host copy helpers
@gpu
@covers("th_dev_upload", "th_dev_download")
@pytest.mark.parametrize("k", BYTES[0])
def test_dev_upload_download_at_byte_offsets(ctx, k):
    lib, check = _lib()
    data = np.random.default_rng(k).integers(0, 256, 100_003, dtype=np.uint8)
    ar = Arena({"dst_dev": k, "src_dev": k})
    ar.add("dst_dev", "dst", np.uint8, data.size, writable=True)
    ar.add("src_dev", "src", np.uint8, data.size, data[::-1].copy())
    ar.commit()
    check(lib.th_dev_upload(ctx.handle, ar.ptr("dst"), data.ctypes.data, data.size))
    back = np.empty_like(data)
    check(lib.th_dev_download(ctx.handle, back.ctypes.data, ar.ptr("src"), back.size))
    ar.check()
    assert np.array_equal(ar.get("dst"), data) and np.array_equal(back, data[::-1])


# ---------------------------------------------------------------- a pointer below its stated alignment is refused

def _refusal_runs(ctx):
    return {
        "th_calc_spec_batch_dev": lambda s: run_calc_spec(ctx, "wave-2048", False, {}, shift=s),
        "th_calc_spec_batch_ranged_dev": lambda s: run_calc_spec(ctx, "wave-2048", True, {}, shift=s),
        "th_minmax_reduce_dev": lambda s: run_reduce(ctx, "th_minmax_reduce_dev", 5, {}, s),
        "th_global_db_range_dev": lambda s: run_reduce(ctx, "th_global_db_range_dev", 5, {}, s),
        "th_minmax_reduce_range_dev": lambda s: run_reduce(ctx, "th_minmax_reduce_range_dev", 5, {}, s),
        "th_spec_to_img_dev": lambda s: run_spec_to_img(ctx, "th_spec_to_img_dev", [IMG_SHAPES[1]], (-100.0, 0.0), {}, s),
        "th_spec_to_img_batch_dev": lambda s: run_spec_to_img(ctx, "th_spec_to_img_batch_dev", IMG_SHAPES[1:3], (-100.0, 0.0), {}, s),
        "th_spec_to_img_batch_dev_ranged": lambda s: run_spec_to_img(ctx, "th_spec_to_img_batch_dev_ranged", IMG_SHAPES[1:3], (-100.0, 0.0), {}, s),
        "th_spec_to_img_raster_batch_dev": lambda s: run_fused(ctx, (-100.0, -3.5), {}, s),
        "th_raster_tiles_dev": lambda s: run_raster(ctx, 1031, 530, "dense", {}, s),
        "th_encode_spectrogram_tile_dev": lambda s: run_spectrogram_tile(ctx, True, {}, s),
        "th_encode_waveform_tile_dev": lambda s: run_waveform_tile(ctx, {}, s),
        "th_waveform_tiles_dev": lambda s: run_waveform_tiles(ctx, {}, s),
        "th_waveform_pyramid_dev": lambda s: run_pyramid(ctx, {}, s),
        "th_channel_stats_dev": lambda s: run_channel_stats(ctx, {}, s),
        "th_audio_stats_dev": lambda s: run_audio_stats(ctx, {}, s),
    }


# what th_last_error() calls the argument where the header's name is a path or a parameter of another spelling
_ARG_NAME = {"img.spec": "spec", "img.img": "img", "tiles": "tile", "d_spec": "spec", "d_img": "img"}
_REFUSALS = [(e, p, b) for e, ptrs in ENTRIES.items() for p, (_, align) in ptrs.items() if align > 1
             for b in sorted({1, 2, align // 2} - {0, align})]


@gpu
@pytest.mark.parametrize("entry,pointer,nbytes", [pytest.param(e, p, b, id=f"{e}-{p}+{b}B") for e, p, b in _REFUSALS])
def test_misaligned_pointer_is_refused(ctx, entry, pointer, nbytes):
    """A device pointer `nbytes` off its stated alignment: TH_ERR_INVALID_ARG naming the argument, before anything is launched —
    the arena is as it was, inputs and outputs."""
    import thesia_amd as ta
    _LAST.clear()
    with pytest.raises(ta.ThError) as e:
        _refusal_runs(ctx)[entry]({pointer: nbytes})
    assert e.value.code == -1, e.value
    assert _ARG_NAME.get(pointer, pointer) in str(e.value) and "aligned" in str(e.value), str(e.value)
    ctx.synchronize()
    ar = _LAST["arena"]
    ar.may[:] = False
    ar.check()
