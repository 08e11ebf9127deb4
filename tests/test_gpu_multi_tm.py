"""th_tmg (MultiTrackManager): several slots of one process give exactly what ONE TrackManager holding every track gives —
updated ids, max_sr, db state, revisions, specs, images, tiles of every kind, batched tiles, render metadata — after every
step of one scenario; placement follows the stated rule; a failing set_setting / add_tracks changes no slot; tile readers
never see a half-applied writer.  On a one-GPU box the slots share the card ([0, 0], [0, 0, 0]); [0, 1] runs where two
devices exist."""
import ctypes as C
import threading

import numpy as np
import pytest

import thesia_amd as ta
from thesia_amd import _ffi
from tests import dynamics_ref as ref
from tests.synth import synth_track

pytestmark = pytest.mark.gpu

LAYOUTS = [[0], [0, 0], [0, 0, 0], [0, 1]]


def _layout(devices):
    if max(devices) >= ta.device_count():
        pytest.skip(f"needs {max(devices) + 1} devices")
    return devices


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cmap(golden_dir):
    return open(f"{golden_dir}/colormap_inferno_rgba258.bin", "rb").read()


def track(seed, sr, seconds, channels=1, peak=0.2):
    n = int(sr * seconds)
    x = np.stack([synth_track(seed + c, sr, n) for c in range(channels)])
    return (x * (peak / np.abs(x).max())).astype(np.float32)


# id -> (sr, planar audio).  Weights (n_samples x n_channels): 3 > 4 > 2 > 1, so the loudest track (3, 48 kHz stereo) and
# the max_sr track (4, 96 kHz) land on different slots for every N >= 2
TRACKS = {1: (8000, track(10, 8000, 3.0)), 2: (44100, track(20, 44100, 2.0)),
          3: (48000, track(30, 48000, 1.5, channels=2, peak=0.95)), 4: (96000, track(40, 96000, 1.0))}


def place(resident, batch, n_slots):
    """The placement rule restated: resident ids stay; new ids longest-first by n_samples x n_channels (ties in input order)
    to the slot with the least resident weight (ties: the lowest slot).  resident: id -> (slot, weight); batch: [(id, w)]."""
    load = [0] * n_slots
    for s, w in resident.values():
        load[s] += w
    out = dict(resident)
    new = [(i, w) for i, w in batch if i not in resident]
    for i, w in sorted(new, key=lambda e: -e[1]):  # (sorted is stable)
        s = min(range(n_slots), key=lambda k: (load[k], k))
        out[i] = (s, w)
        load[s] += w
    for i, w in batch:
        if i in resident:
            out[i] = (resident[i][0], w)
    return out


def raw_batch(mgr, reqs, fill=0, extra=0):
    """th_*_get_spectrogram_tiles into a pageable buffer of `extra` bytes more than needed, every byte `fill` before the call: the
    whole buffer (padding included) and the offsets."""
    multi = isinstance(mgr, ta.MultiTrackManager)
    fn = _ffi.lib.th_tmg_get_spectrogram_tiles if multi else _ffi.lib.th_tm_get_spectrogram_tiles
    n = len(reqs)
    arr = (_ffi.TileRequest * n)(*[_ffi.TileRequest(*r, 0) for r in reqs])
    offs = (C.c_size_t * (n + 1))()
    need = C.c_size_t()
    assert fn(mgr.handle, arr, n, None, 0, offs, C.byref(need)) == _ffi.ERR_BUFFER_TOO_SMALL
    buf = np.full(need.value + extra, fill, np.uint8)
    _ffi.check(fn(mgr.handle, arr, n, buf.ctypes.data_as(C.c_void_p), buf.size, offs, C.byref(need)))
    assert need.value == buf.size - extra == offs[n]
    return buf.tobytes(), list(offs)


def snapshot(mgr, ids):
    """Everything a host can read back from a manager."""
    s = {"db": mgr.db_state(), "rev": mgr.revisions()}
    reqs = []
    for i in ids:
        nch = TRACKS_NOW[i][1].shape[0]
        for ch in range(nch):
            s[("spec", i, ch)] = mgr.spec(i, ch)
            s[("img", i, ch)] = mgr.img(i, ch)
            for lx, ly, tx, ty in [(0, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 0), (2, 0, 0, 0), (3, 4, 0, 0)]:
                s[("tile", i, ch, lx, ly, tx, ty)] = mgr.get_spectrogram_tile(i, ch, lx, ly, tx, ty)
                reqs.append((i, ch, lx, ly, tx, ty))
            for lv in (0, 1, 3, 8, 30):
                s[("wave", i, ch, lv)] = mgr.get_waveform_tile(i, ch, lv, 0)
            s[("meta", i, ch)] = mgr.render_metadata(i, ch, 1.25, False)
    reqs = reqs[::-1]  # (an order that interleaves the slots)
    if reqs:
        s["batch"] = raw_batch(mgr, reqs)
        s["batch_pinned"] = mgr.get_spectrogram_tiles(reqs, pinned=True)
    return s


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


TRACKS_NOW = {}


@pytest.mark.parametrize("devices", LAYOUTS, ids=lambda d: "-".join(map(str, d)))
def test_multi_manager_equals_one_manager(ctx, cmap, devices):
    devices = _layout(devices)
    one, multi = ta.TrackManager(ctx), ta.MultiTrackManager(devices)
    mgrs = (one, multi)
    assert multi.n_devices == len(devices)
    TRACKS_NOW.clear()  # (what is resident: what snapshot() reads back)
    resident = {}

    def step(fn):
        out = [fn(m) for m in mgrs]
        assert out[0] == out[1]
        assert_same(snapshot(one, sorted(TRACKS_NOW)), snapshot(multi, sorted(TRACKS_NOW)))
        return out[0]

    try:
        step(lambda m: m.set_colormap(cmap))
        batch = [(i, sr, x) for i, (sr, x) in TRACKS.items()]
        for m in mgrs:
            m.add_tracks(batch)
        TRACKS_NOW.update(TRACKS)
        resident = place(resident, [(i, x.size) for i, _, x in batch], len(devices))
        assert {i: multi.device_of(i) for i in TRACKS} == {i: s for i, (s, _) in resident.items()}
        assert set(resident[i][0] for i in TRACKS) == set(range(len(devices))), "every slot owns a track"
        if len(devices) > 1:
            assert resident[3][0] != resident[4][0], "loudest and max_sr tracks share a slot"
        upd, sr = step(lambda m: m.apply_track_list_changes())
        assert upd == [1, 2, 3, 4] and sr == 96000
        step(lambda m: m.set_dB_range(80.0))
        # the loudest track goes: the range moves on slots where nothing changed
        db0 = one.db_state()
        for m in mgrs:
            m.remove_track(3)
        del TRACKS_NOW[3], resident[3]
        with pytest.raises(ta.ThError) as e:
            multi.device_of(3)
        assert e.value.code == _ffi.ERR_NOT_FOUND
        upd, _ = step(lambda m: m.apply_track_list_changes())
        assert upd == [1, 2, 4] and one.db_state()[1] < db0[1]
        # a resident id again, with new audio: replaced on its own slot
        TRACKS_NOW[2] = (44100, track(21, 44100, 2.5))
        slot2 = multi.device_of(2)
        for m in mgrs:
            m.add_tracks([(2, 44100, TRACKS_NOW[2][1])])
        assert multi.device_of(2) == slot2
        step(lambda m: m.apply_track_list_changes())
        step(lambda m: m.set_setting(20.0, 4, 2, ta.LINEAR))
        step(lambda m: m.apply_track_list_changes())  # (nothing to do: the same on both)
    finally:
        multi.close()
        one.close()


def _setup_three(ctx, cmap):
    devices = [0, 0, 0]
    one, multi = ta.TrackManager(ctx), ta.MultiTrackManager(devices)
    for m in (one, multi):
        m.set_colormap(cmap)
        m.add_tracks([(i, sr, x) for i, (sr, x) in TRACKS.items()])
        m.apply_track_list_changes()
    assert {multi.device_of(i) for i in TRACKS} == {0, 1, 2}
    TRACKS_NOW.clear()
    TRACKS_NOW.update(TRACKS)
    return one, multi


def test_failed_mutators_change_no_slot(ctx, cmap):
    one, multi = _setup_three(ctx, cmap)
    try:
        before = snapshot(multi, sorted(TRACKS_NOW))
        # n_fft 2^21 (> TH_MAX_N_FFT): every slot would have to re-plan; none may change
        for m in (one, multi):
            with pytest.raises(ta.ThError) as e:
                m.set_setting(40.0, 4, 1024, ta.LINEAR)
            assert e.value.code == _ffi.ERR_UNSUPPORTED
        assert "slot" in str(e.value) and "device 0" in str(e.value)
        assert_same(before, snapshot(multi, sorted(TRACKS_NOW)))
        # a batch whose track 11 cannot be planned (40 ms at 100 MHz: n_fft 2^22) while 10 and 12 go to other slots: those
        # slots stage their tracks, then discard them
        bad = [(10, 48000, track(50, 48000, 1.0)), (11, 100_000_000, track(51, 48000, 0.02)), (12, 48000, track(52, 48000, 0.8))]
        resident = {i: (multi.device_of(i), x.size) for i, (_, x) in TRACKS.items()}
        where = place(resident, [(i, x.size) for i, _, x in bad], 3)
        assert where[11][0] not in (where[10][0], where[12][0])
        for m in (one, multi):
            with pytest.raises(ta.ThError) as e:
                m.add_tracks(bad)
            assert e.value.code == _ffi.ERR_UNSUPPORTED
        assert f"slot {where[11][0]} (device 0)" in str(e.value)
        for i in (10, 11, 12):
            with pytest.raises(ta.ThError):
                multi.device_of(i)
            with pytest.raises(ta.ThError):
                multi.get_waveform_tile(i, 0, 0, 0)
        assert_same(before, snapshot(multi, sorted(TRACKS_NOW)))
        assert_same(snapshot(one, sorted(TRACKS_NOW)), snapshot(multi, sorted(TRACKS_NOW)))
        # later calls still work, and still agree
        good = [b for b in bad if b[0] != 11]
        for m in (one, multi):
            m.add_tracks(good)
        TRACKS_NOW.update({i: (sr, x) for i, sr, x in good})
        assert [multi.device_of(i) for i in (10, 12)] == [where[10][0], where[12][0]]
        assert one.apply_track_list_changes() == multi.apply_track_list_changes()
        assert_same(snapshot(one, sorted(TRACKS_NOW)), snapshot(multi, sorted(TRACKS_NOW)))
        # the same batch (as ids 20, 21, 22) while a normalise target is in force: every staged track's audio is derived from its
        # stats before its specs are made, so the slots of 20 and 22 discard derived audio as well
        for m in (one, multi):
            m.set_common_normalize(ref.NORM_RMS_DB, -6.0)
        before = snapshot(multi, sorted(TRACKS_NOW))
        assert_same(snapshot(one, sorted(TRACKS_NOW)), before)
        bad = [(i + 10, sr, x) for i, sr, x in bad]
        resident = {i: (multi.device_of(i), x.size) for i, (_, x) in TRACKS_NOW.items()}
        where = place(resident, [(i, x.size) for i, _, x in bad], 3)
        assert where[21][0] not in (where[20][0], where[22][0])
        for m in (one, multi):
            with pytest.raises(ta.ThError) as e:
                m.add_tracks(bad)
            assert e.value.code == _ffi.ERR_UNSUPPORTED
        assert f"slot {where[21][0]} (device 0)" in str(e.value)
        for i in (20, 21, 22):
            with pytest.raises(ta.ThError):
                multi.device_of(i)
        assert_same(before, snapshot(multi, sorted(TRACKS_NOW)))
        assert_same(snapshot(one, sorted(TRACKS_NOW)), snapshot(multi, sorted(TRACKS_NOW)))
        good = [b for b in bad if b[0] != 21]
        for m in (one, multi):
            m.add_tracks(good)
        TRACKS_NOW.update({i: (sr, x) for i, sr, x in good})
        assert [multi.device_of(i) for i in (20, 22)] == [where[20][0], where[22][0]]
        assert one.apply_track_list_changes() == multi.apply_track_list_changes()
        assert_same(snapshot(one, sorted(TRACKS_NOW)), snapshot(multi, sorted(TRACKS_NOW)))
        assert all(one.track_dynamics(i)["normalize_gain"] > 1 and one.track_dynamics(i) == multi.track_dynamics(i) for i in (20, 22))
    finally:
        multi.close()
        one.close()


def test_batched_tiles_of_two_slots_write_their_records_only():
    """A pageable buffer, so every slot stages its own records; slot 0's requests first, so slot 1's first record lies behind all of
    slot 0's in the caller's buffer but first in slot 1's staging.  Every record is the single-tile path's; the padding between
    records and the bytes behind the last keep what they held.  No colormap is set: the batch makes each slot upload the default."""
    with ta.MultiTrackManager([0, 0]) as multi:
        multi.add_tracks([(i, sr, x) for i, (sr, x) in TRACKS.items()])
        multi.apply_track_list_changes()
        reqs = [(i, ch, lx, ly, tx, 0) for i, (_, x) in TRACKS.items() for ch in range(x.shape[0])
                for lx, ly, tx in [(0, 0, 0), (0, 0, 1), (1, 1, 0), (3, 4, 0)]]
        reqs.sort(key=lambda r: multi.device_of(r[0]))  # (stable)
        owners = [multi.device_of(r[0]) for r in reqs]
        assert set(owners) == {0, 1} and owners == sorted(owners)
        buf, offs = raw_batch(multi, reqs, fill=0xA5, extra=64)
        padding = 0
        for k, r in enumerate(reqs):
            rec = multi.get_spectrogram_tile(*r)
            assert len(rec) >= 40 and offs[k] + len(rec) <= offs[k + 1] and offs[k] % 64 == 0
            assert buf[offs[k]: offs[k] + len(rec)] == rec, r
            assert set(buf[offs[k] + len(rec): offs[k + 1]]) <= {0xA5}, r
            padding += offs[k + 1] - offs[k] - len(rec)
        assert padding > 0 and set(buf[offs[-1]:]) == {0xA5}


def test_tile_readers_against_a_writer(ctx, cmap):
    """Four reader threads ask for tiles of tracks on both slots while the writer flips the dB range: every tile's pixels are
    those of the state its header's revision names."""
    devices = [0, 0]
    multi = ta.MultiTrackManager(devices)
    one = ta.TrackManager(ctx)
    try:
        for m in (one, multi):
            m.set_colormap(cmap)
            m.add_tracks([(i, sr, x) for i, (sr, x) in TRACKS.items()])
            m.apply_track_list_changes()
        assert {multi.device_of(i) for i in TRACKS} == {0, 1}
        reqs = [(i, 0, lx, ly, 0, 0) for i in TRACKS for lx, ly in [(0, 0), (1, 1)]]
        ranges = (60.0, 90.0)
        want = {}
        for r in ranges:  # the pixels of each state, from one manager
            one.set_dB_range(r)
            want[r] = {q: one.get_spectrogram_tile(*q)[8:] for q in reqs}
        assert any(want[ranges[0]][q] != want[ranges[1]][q] for q in reqs)
        multi.set_dB_range(ranges[0])
        state = {multi.revisions()[1]: ranges[0]}
        seen, errors, stop = [], [], threading.Event()

        def reader(k):
            try:
                j = k
                while not stop.is_set():
                    q = reqs[j % len(reqs)]
                    t = multi.get_spectrogram_tile(*q)
                    seen.append((int.from_bytes(t[:8], "little"), q, t[8:]))
                    j += 1
            except Exception as e:  # noqa: BLE001 (re-raised on the main thread)
                errors.append(e)

        threads = [threading.Thread(target=reader, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        try:
            for n in range(40):
                r = ranges[(n + 1) % 2]
                multi.set_dB_range(r)
                state[multi.revisions()[1]] = r
        finally:
            stop.set()
            for t in threads:
                t.join()
        assert not errors, errors
        assert len(seen) > 40
        for rev, q, body in seen:
            assert rev in state, rev
            assert body == want[state[rev]][q], (rev, q)
    finally:
        multi.close()
        one.close()
