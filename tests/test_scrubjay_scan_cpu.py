"""CPU: the host side of scrub-jay scans -- dsp_scan_window_spans (no GPU call) against a plain restatement of the window rule in
samples, for complete and stream framing; each span's frame count against the window's rows; the span count against
dsp_scan_window_offsets; the refusals; the Python wrappers' argument checks."""
import ctypes as C

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from dsp_amd import scrubjay

SHAPES = [(16, 4), (16, 1), (98, 10), (5000, 3)]          # the last: a window longer than most recordings


def _configs():
    return {"512": dsp_amd.default_config(n_mfcc=20), "aubio": scrubjay.scrubjay_infer_config(16000),
            "2048": scrubjay.scrubjay_infer_config(16000, aubio=False)}


def _rows(cfg, n):
    """MFCC rows of n samples: ceil(n / hop) under stream framing, 1 + (n - frame) // hop complete frames"""
    if cfg.framing == dl.FRAMING_STREAM:
        return -(-n // cfg.hop_length)
    return 0 if n < cfg.frame_length else 1 + (n - cfg.frame_length) // cfg.hop_length


def _spans(cfg, offsets, wf, hf):
    """window w of a recording starts w hf hop samples in; frame + (wf - 1) hop samples long (complete) or wf hop (stream), clipped to
    the recording; fewer rows than a window: the whole recording"""
    starts, lengths, rows = [], [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        n = b - a
        r = _rows(cfg, n)
        if r < wf:
            starts.append(a), lengths.append(n), rows.append(r)
            continue
        span = wf * cfg.hop_length if cfg.framing == dl.FRAMING_STREAM else cfg.frame_length + (wf - 1) * cfg.hop_length
        for w in range(1 + (r - wf) // hf):
            s = w * hf * cfg.hop_length
            starts.append(a + s), lengths.append(min(span, n - s)), rows.append(wf)
    return np.array(starts, np.int64), np.array(lengths, np.int64), rows


def _lengths(cfg, wf, hf, seed):
    """0, shorter than a frame, exactly one window, one window + one hop, random 1-60 s, 10 min"""
    hop, frame = cfg.hop_length, cfg.frame_length
    one = wf * hop if cfg.framing == dl.FRAMING_STREAM else frame + (wf - 1) * hop
    rng = np.random.default_rng(seed)
    return [0, frame - 1, 1, one, one - 1, one + 1, one + hf * hop, one + hf * hop - 1] + rng.integers(16000, 60 * 16000, 6).tolist() + [600 * 16000]


@pytest.mark.parametrize("name", ["512", "aubio", "2048"])
@pytest.mark.parametrize("wf,hf", SHAPES)
def test_window_spans_follow_the_rule(name, wf, hf):
    cfg = _configs()[name]
    lens = _lengths(cfg, wf, hf, 7 * wf + hf)
    offsets = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)
    want_s, want_l, want_rows = _spans(cfg, offsets.tolist(), wf, hf)
    starts, lengths = scrubjay.scan_window_spans(cfg, offsets, wf, hf)
    np.testing.assert_array_equal(starts, want_s)
    np.testing.assert_array_equal(lengths, want_l)
    # each span, cut out, has the window's rows; the span count is the row planner's window count
    got_rows = [dsp_amd.frames_for(cfg, int(n), 2**31 - 1) for n in lengths]
    assert got_rows == want_rows
    fo = np.concatenate([[0], np.cumsum([_rows(cfg, n) for n in lens])])
    wo = dsp_amd.scan_window_offsets(fo, wf, hf)
    assert wo[-1] == starts.size
    for r in range(len(lens)):                                  # a recording's windows start inside it and end inside it
        s, n = starts[wo[r]:wo[r + 1]], lengths[wo[r]:wo[r + 1]]
        assert (s >= offsets[r]).all() and (s + n <= offsets[r + 1]).all()


def test_one_hour_of_the_aubio_front_end():
    """scrubjay_infer.c's framing over one hour at 16 kHz: 56 250 rows, 1 s windows (16 rows) every 4 rows -> 14 059 windows"""
    cfg = _configs()["aubio"]
    starts, lengths = scrubjay.scan_window_spans(cfg, [0, 3600 * 16000], 16, 4)
    assert starts.size == 14059 == 1 + (56250 - 16) // 4
    assert (lengths == 16 * 1024).all() and starts[-1] == 14058 * 4 * 1024


def _c_spans(cfg, scfg, offsets, n, starts=None, lengths=None):
    lp = C.POINTER(C.c_long)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).ctypes.data_as(lp)
    return dl.load().dsp_scan_window_spans(None if cfg is None else C.byref(cfg), None if scfg is None else C.byref(scfg), off, n,
                                           starts, lengths)


def test_refusals():
    cfg = _configs()["aubio"]
    good = dl.ScanConfig(16, 4)
    off = [0, 16000, 32000]
    assert _c_spans(cfg, good, off, 2) == 2 * (1 + (16 - 16) // 4)
    assert _c_spans(cfg, good, off, 0) == 0                                      # no recordings
    assert _c_spans(cfg, good, None, 0) == 0
    assert _c_spans(None, good, off, 2) == dl.load().dsp_scan_window_spans(None, C.byref(good), None, 2, None, None) == -1
    for bad in (dl.ScanConfig(0, 4), dl.ScanConfig(16, 0), dl.ScanConfig(-1, 1)):
        assert _c_spans(cfg, bad, off, 2) == -1
        assert "window_frames" in dl.last_error()
    assert _c_spans(cfg, None, off, 2) == -1
    assert _c_spans(cfg, good, None, 2) == -1
    assert _c_spans(cfg, good, off, -1) == -1
    assert _c_spans(cfg, good, [0, 16000, 15999], 2) == -1                        # decreasing offsets name the recording
    assert "clip 1" in dl.last_error()
    assert _c_spans(cfg, good, [-5, 16000], 1) == -1
    broken = scrubjay.scrubjay_infer_config(16000)
    broken.hop_length = 0
    assert _c_spans(broken, good, off, 2) == -1 and "hop_length" in dl.last_error()


def test_python_wrappers_raise_value_error():
    cfg = _configs()["512"]
    with pytest.raises(ValueError):
        scrubjay.scan_window_spans(cfg, [0, 16000], 0, 4)
    with pytest.raises(ValueError):
        scrubjay.scan_window_spans(cfg, [0, 16000], 16, -1)
    with pytest.raises(ValueError):
        scrubjay.scan_window_spans(cfg, [[0, 16000]], 16, 4)
    with pytest.raises(dl.DspError):
        scrubjay.scan_window_spans(cfg, [0, 16000, 100], 16, 4)


def test_exports():
    L = dl.load()
    for name in ("dsp_scan_window_spans", "dsp_svm_scan_device", "dsp_scrubjay_scanner_create", "dsp_scrubjay_scanner_destroy",
                 "dsp_scrubjay_scanner_run_device", "dsp_scrubjay_scanner_run_pcm16_device"):
        assert hasattr(L, name) and name in dl.SYMBOLS
