"""A batched reader on MultiTrackManager([0, 0]) against one TrackManager, for a batch whose owners are A, B, A: slot A's two records
are not adjacent in the output, slot B writes between them.  Two tracks of 2048 samples at 8 kHz, one stereo (id 1) and one mono
(id 2), so that each slot owns one.  Through the raw entry points with a canary-filled output: the size query publishes the infos,
a short buffer is left alone, bytes and infos equal the single manager's, and the canaries between and behind the records are intact."""
import ctypes as C

import numpy as np

import thesia_amd as ta
from thesia_amd import _ffi
from tests.synth import synth_track

SR, N, CANARY = 8000, 2048, 0xA5
TRACKS = [(1, SR, np.stack([synth_track(71, SR, N), synth_track(72, SR, N)])), (2, SR, synth_track(73, SR, N)[None])]
A, B = 1, 2


def check(ctx, entry, reqs, info_cls, elem_bytes, length_field, revision_field, images=False, granule=1):
    """entry: the entry's name behind th_tm_ / th_tmg_; reqs: three ctypes requests for tracks A, B, A; elem_bytes: the size of an
    output element; length_field: the info's record length, in elements; granule: a record and the bytes the reader pads it with
    end at the next multiple of this many bytes (the export's zero bytes), the last record at its own end"""
    tm, g = ta.TrackManager(ctx), ta.MultiTrackManager([0, 0])
    try:
        for m in (tm, g):
            m.add_tracks(TRACKS)
            if images:
                m.apply_track_list_changes()
        assert g.device_of(A) != g.device_of(B)
        arr = (type(reqs[0]) * 3)(*reqs)

        def call(m, pfx, cap, with_out=True):
            fn = getattr(_ffi.lib, pfx + entry)
            info, need = (info_cls * 3)(), C.c_size_t(12345)
            C.memset(info, CANARY, C.sizeof(info))
            buf = np.full((cap + 16) * elem_bytes, CANARY, np.uint8)
            out = C.cast(buf.ctypes.data, fn.argtypes[3]) if with_out else None
            return fn(m.handle, arr, 3, out, cap, info, C.byref(need)), buf, info, need.value

        def same_infos(a, b, revision):
            for x, y in zip(a, b):
                assert getattr(y, revision_field) == revision
                assert [getattr(x, k) for k, _ in info_cls._fields_ if k != revision_field] == \
                    [getattr(y, k) for k, _ in info_cls._fields_ if k != revision_field]

        revision = g.revisions()[0 if revision_field == "waveform_revision" else 1]
        rc, _, want_q, need = call(tm, "th_tm_", 0, with_out=False)
        assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need > 0
        rc, buf, got_q, need_g = call(g, "th_tmg_", 0, with_out=False)  # the size query publishes the infos
        assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need_g == need
        same_infos(want_q, got_q, revision)
        rc, buf, got_s, need_g = call(g, "th_tmg_", need - 1)  # a short buffer: the same, and nothing is written
        assert rc == _ffi.ERR_BUFFER_TOO_SMALL and need_g == need and (buf == CANARY).all()
        same_infos(want_q, got_s, revision)
        rc, want, winfo, _ = call(tm, "th_tm_", need)
        assert rc == _ffi.OK, _ffi.last_error()
        rc, got, ginfo, need_g = call(g, "th_tmg_", need)
        assert rc == _ffi.OK and need_g == need, _ffi.last_error()
        same_infos(winfo, ginfo, revision)
        assert np.array_equal(got, want)
        written = np.zeros(got.size, bool)
        for k, o in enumerate(ginfo):
            a, b = o.offset * elem_bytes, (o.offset + getattr(o, length_field)) * elem_bytes
            assert b > a and not (got[a:b] == CANARY).all()
            written[a: b if k == 2 else -(-b // granule) * granule] = True
        assert (got[~written] == CANARY).all() and not written[need * elem_bytes:].any()  # between and behind the records
        assert ginfo[0].offset < ginfo[1].offset < ginfo[2].offset
        return ginfo
    finally:
        g.close()
        tm.close()
