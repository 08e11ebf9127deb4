"""Every batched reader on MultiTrackManager([0, 0]) with a batch whose owners are A, B, A (tests/aba_batch.py): slot A's two records
are not adjacent, slot B writes between them.  Bytes and infos are those of one TrackManager, the size query and a short buffer publish
the infos and write nothing, and the canaries between and behind the records are intact.  The meters are not here: their series of
2048 samples at 8 kHz is empty, and tests/test_gpu_loudness_meter.py::test_independence_and_refusals has two slots taking turns on a
canary-filled series."""
import pytest

import thesia_amd as ta
from thesia_amd import _ffi, api
from tests import aba_batch
from tests.aba_batch import A, B

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    c = ta.Context(0)
    yield c
    c.close()


def test_spectra(ctx):
    reqs = [_ffi.SpectrumRequest(A, 1, ta.SPECTRUM_MEAN_POWER, 0.0, INF), _ffi.SpectrumRequest(B, 0, ta.SPECTRUM_MAX, 0.05, 0.2),
            _ffi.SpectrumRequest(A, 0, ta.SPECTRUM_MEAN_AMP, 0.1, INF)]
    aba_batch.check(ctx, "get_spectra", reqs, _ffi.SpectrumInfo, 4, "height", "spectrogram_revision")


def test_export(ctx):
    """between the records only the zero bytes up to the next multiple of 16"""
    reqs = [api._export_request((A, api.PCM_S24, api.DITHER_TPDF, 3, 0.0, 0.125)), api._export_request((B, api.PCM_S16, api.DITHER_NONE, 0)),
            api._export_request((A, api.PCM_F32, api.DITHER_NONE, 0, 0.125, 0.25))]
    infos = aba_batch.check(ctx, "export_pcm", reqs, _ffi.ExportInfo, 1, "n_bytes", "waveform_revision", granule=16)
    assert [o.n_bytes for o in infos] == [1000 * 6, 2048 * 2, 1000 * 8] and [o.offset for o in infos] == [0, 6000, 6000 + 4096]


def test_figures(ctx):
    """offsets are multiples of 64: the bytes between the records are left alone"""
    reqs = [api._figure_request((A, 1, ta.FIGURE_RGBA, 7, 5, (0.0, 0.0, 4.0, 9.0))), api._figure_request((B, 0, ta.FIGURE_GREY16, 9, 3, (1.5, 2.0, 3.0, 8.0))),
            api._figure_request((A, 0, ta.FIGURE_RGBA, 3, 3, (0.0, 1.0, 2.5, 2.5)))]
    infos = aba_batch.check(ctx, "render_figures", reqs, _ffi.FigureInfo, 1, "bytes", "spectrogram_revision", images=True)
    assert [(o.offset, o.bytes) for o in infos] == [(0, 140), (192, 54), (256, 36)]


def test_envelopes(ctx):
    reqs = [_ffi.EnvelopeRequest(A, 1, 1, 0.0, INF, 7, 0), _ffi.EnvelopeRequest(B, 0, 0, 0.01, 0.2, 5, 0), _ffi.EnvelopeRequest(A, 0, 2, 0.1, INF, 3, 0)]
    aba_batch.check(ctx, "get_envelopes", reqs, _ffi.EnvelopeInfo, 4, "length", "waveform_revision")


def test_waveform_figures(ctx):
    """offsets are multiples of 64: the bytes between the records are left alone"""
    lanes = [api._waveform_figure_request((A, 1, 1, 0.0, INF, 7, 5, -1.0, 1.0, 256, (1, 2, 3, 4), (9, 9, 9, 9))),
             api._waveform_figure_request((B, 0, 1, 0.0, INF, 3, 3, -0.5, 0.5, 100, (255, 200, 0, 255), (0, 0, 0, 255))),
             api._waveform_figure_request((A, 0, 1, 0.05, 0.2, 4, 2, -1.0, 1.0, 0, (1, 2, 3, 4), (7, 7, 7, 7)))]
    infos = aba_batch.check(ctx, "render_waveform_figures", lanes, _ffi.WaveformFigureInfo, 1, "bytes", "waveform_revision")
    assert [(o.offset, o.bytes) for o in infos] == [(0, 140), (192, 36), (256, 32)]


def test_formants(ctx):
    """the two counts of every request come back to its place among the infos"""
    kw = dict(sr_analysis=8000, n_poles=4, win_sec=0.02, step_sec=0.01)
    reqs = [ta.formant_request(A, 1, 0, **kw), ta.formant_request(B, 0, 0, kind=ta.FORMANT_OUT_LPC, end_sec=0.1, **kw),
            ta.formant_request(A, 0, 2, start_sec=0.05, **kw)]
    infos = aba_batch.check(ctx, "get_formants", reqs, _ffi.FormantInfo, 8, "length", "waveform_revision")
    assert all(o.length == (o.frame_end - o.frame_first) * 6 for o in infos)
