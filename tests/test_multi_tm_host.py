"""th_tmg (TrackManager over several devices of one process): the interface, and the argument checks of th_tmg_create that
come before any device is touched.  CPU only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TMG = ["th_tmg_create", "th_tmg_destroy", "th_tmg_n_devices", "th_tmg_track_device", "th_tmg_set_colormap",
       "th_tmg_set_setting", "th_tmg_set_dB_range", "th_tmg_add_tracks", "th_tmg_remove_track",
       "th_tmg_apply_track_list_changes", "th_tmg_get_db_state", "th_tmg_spec_shape", "th_tmg_img_shape",
       "th_tmg_copy_spec", "th_tmg_copy_img", "th_tmg_revisions", "th_tmg_get_spectrogram_tile",
       "th_tmg_get_spectrogram_tiles", "th_tmg_get_waveform_tile", "th_tmg_get_audio_render_metadata",
       "th_tmg_set_lod_source"]


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"TH_API\s+[\w\s\*]+?\b(th_\w+)\s*\(", txt))


def test_every_tmg_entry_is_declared_exported_and_bound():
    import thesia_amd
    from thesia_amd import _ffi
    product = _declared("thesia_amd.h")
    assert set(TMG) <= product, set(TMG) - product
    assert not {s for s in _declared("thesia_amd_testing.h") if s.startswith("th_tmg_")}
    lib = C.CDLL(thesia_amd.LIB_PATH)
    assert all(hasattr(lib, s) for s in TMG), [s for s in TMG if not hasattr(lib, s)]
    assert set(TMG) <= set(_ffi._SIGS), set(TMG) - set(_ffi._SIGS)


def test_every_th_tm_call_of_the_binding_has_a_tmg_twin():
    """a multi-GPU host swaps th_tm_* for th_tmg_* one for one, with the same argument lists after the handle."""
    from thesia_amd import _ffi
    for s in TMG:
        tm = s.replace("th_tmg_", "th_tm_")
        if tm in _ffi._SIGS and s != "th_tmg_create":
            assert _ffi._SIGS[s][1:] == _ffi._SIGS[tm][1:], s


def _create(devices, n=None):
    from thesia_amd import _ffi
    h = C.c_void_p()
    arr = None if devices is None else (C.c_int * max(len(devices), 1))(*devices)
    rc = _ffi.lib.th_tmg_create(arr, len(devices or []) if n is None else n, C.byref(h))
    if rc == 0:
        _ffi.lib.th_tmg_destroy(h)
    return rc, _ffi.last_error()


@pytest.mark.parametrize("devices, n", [([0], 0), (None, 1), ([-1], 1), ([0, -2], 2), ([0] * 65, 65)])
def test_create_rejects_bad_arguments_before_looking_for_a_device(devices, n):
    rc, msg = _create(devices, n)
    assert rc == -1, (rc, msg)


def test_create_without_gpu_is_no_device():
    import thesia_amd as ta
    if ta.device_count() > 0:
        pytest.skip("GPU present")
    rc, msg = _create([0])
    assert rc == -4 and "no CPU fallback" in msg, (rc, msg)
    with pytest.raises(ta.ThError) as e:
        ta.MultiTrackManager([0, 0])
    assert e.value.code == -4


def test_null_handles_are_invalid_arguments():
    from thesia_amd import _ffi
    n = C.c_size_t()
    assert _ffi.lib.th_tmg_n_devices(None, C.byref(n)) == -1
    assert _ffi.lib.th_tmg_remove_track(None, 0) == -1
    assert _ffi.lib.th_tmg_destroy(None) == 0
