"""CPU: the host side of stream sessions -- dsp_stream_push_plan (no GPU call) against a plain restatement of the formulas
(tests/stream_ref.py), its additivity against the planners of whole recordings, the bounds of what a session carries, the argument
checks made before any device work, the exports, and the Python wrappers' checks under python -O."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import stream_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_SYMBOLS = ["dsp_stream_push_plan", "dsp_stream_session_create", "dsp_stream_session_destroy", "dsp_stream_session_reset",
                  "dsp_stream_session_counts", "dsp_stream_push_device"]
FL, H = 400, 160
SCANS = [(98, 10), (98, 1), (98, 98), (30, 7), (1, 1)]
LP = C.POINTER(C.c_long)
EINVAL = -1


def _c_plan(cfg, received, co, scan=None, want_windows=True):
    """the C planner, raw: (return value, row_offsets, window_offsets)"""
    L = dl.load()
    co = np.ascontiguousarray(co, np.int64)
    n = co.size - 1
    rec = np.ascontiguousarray(received, np.int64) if received is not None else None
    ro, wo = np.full(n + 1, -7, np.int64), np.full(n + 1, -7, np.int64)
    sc = dl.ScanConfig(*scan) if scan else None
    rc = L.dsp_stream_push_plan(C.byref(cfg) if cfg is not None else None, C.byref(sc) if sc else None,
                                rec.ctypes.data_as(LP) if rec is not None else None, co.ctypes.data_as(LP), n, ro.ctypes.data_as(LP),
                                wo.ctypes.data_as(LP) if want_windows else None)
    return rc, ro, wo


@pytest.mark.parametrize("wf,hf", SCANS)
def test_planner_follows_the_restatement(wf, hf):
    cfg = dsp_amd.default_config()
    assert (cfg.frame_length, cfg.hop_length) == (FL, H)
    rng = np.random.default_rng(wf * 100 + hf)
    n = 37
    received = np.zeros(n, np.int64)
    for _push in range(60):
        lengths = rng.choice(R.CHUNKS, n)
        lengths[rng.integers(0, n, 5)] = 0
        co = np.concatenate([[rng.integers(0, 9)], lengths]).cumsum()
        want_ro, want_wo = R.push_plan(received, lengths, FL, H, wf, hf)
        rc, ro, wo = _c_plan(cfg, received, co, (wf, hf))
        assert rc == want_ro[-1]
        np.testing.assert_array_equal(ro, want_ro)
        np.testing.assert_array_equal(wo, want_wo)
        pro, pwo = dsp_amd.stream_push_plan(cfg, received, co, wf, hf)
        np.testing.assert_array_equal(pro, want_ro)
        np.testing.assert_array_equal(pwo, want_wo)
        received = received + lengths
        # what a session carries stays below a frame / a window: from the restatement and from the C planner's own counts
        for s in range(n):
            e = R.rows_after(int(received[s]), FL, H)
            assert 0 <= R.carried_samples(int(received[s]), FL, H) < FL
            assert 0 <= R.carried_rows(e, wf, hf) < wf
    # received = NULL is "nothing yet"; scan = NULL is "no windows"
    rc, ro, wo = _c_plan(cfg, None, [0, 400, 400, 1000], None)           # 400, 0 and 600 samples: 1, 0 and 2 rows
    assert rc == 3 and ro.tolist() == [0, 1, 1, 3] and wo.tolist() == [0] * 4
    rc, ro, _wo = _c_plan(cfg, None, [0, 16000], (98, 10), want_windows=False)
    assert rc == 98 and ro.tolist() == [0, 98]


@pytest.mark.parametrize("wf,hf", SCANS)
def test_pushes_add_up_to_the_whole_recording(wf, hf):
    """any chunking of a recording: the new rows sum to dsp_mfcc_ragged_frame_offsets of the whole, the new windows to
    dsp_scan_window_offsets of those rows when there are at least wf of them and to 0 otherwise; the carries follow from the C
    planner's own sums"""
    cfg = dsp_amd.default_config()
    rng = np.random.default_rng(7 + wf + hf)
    totals = [0, 1, 399, 400, 401, 559, 560, 15999, 16000, 16001, 16000 + 160 * hf] + rng.integers(1, 200000, 6).tolist()
    for total in totals:
        whole = int(dsp_amd.mfcc.ragged_frame_offsets(cfg, [0, total], 2**31 - 1)[1])
        want_w = int(dsp_amd.scan_window_offsets([0, whole], wf, hf)[1]) if whole >= wf else 0
        for _trial in range(3):
            got_r = got_w = seen = 0
            for c in R.chunking(total, rng) + [0]:
                rc, ro, wo = _c_plan(cfg, [seen], [0, c], (wf, hf))
                assert rc >= 0
                got_r += int(ro[1])
                got_w += int(wo[1])
                seen += c
                assert 0 <= seen - got_r * H < FL, (total, seen)
                assert 0 <= got_r - got_w * hf < wf, (total, seen)
                assert got_r == R.rows_after(seen, FL, H) and got_w == R.windows_after(got_r, wf, hf)
            assert (got_r, got_w) == (whole, want_w), total


def test_planner_refusals():
    L = dl.load()
    cfg = dsp_amd.default_config()
    good = [0, 100, 500]
    assert _c_plan(cfg, [0, 0], good, (98, 10))[0] == 1
    assert _c_plan(None, [0, 0], good, (98, 10))[0] == EINVAL
    co = np.array(good, np.int64)
    ro = np.zeros(3, np.int64)
    assert L.dsp_stream_push_plan(C.byref(cfg), None, None, None, 2, ro.ctypes.data_as(LP), None) == EINVAL
    assert L.dsp_stream_push_plan(C.byref(cfg), None, None, co.ctypes.data_as(LP), 2, None, None) == EINVAL
    assert L.dsp_stream_push_plan(C.byref(cfg), None, None, co.ctypes.data_as(LP), -1, ro.ctypes.data_as(LP), None) == EINVAL
    assert L.dsp_stream_push_plan(C.byref(cfg), None, None, co.ctypes.data_as(LP), 0, ro.ctypes.data_as(LP), None) == 0
    assert _c_plan(cfg, [0, 0], [0, 500, 100], (98, 10))[0] == EINVAL and "stream 1" in dl.last_error()
    assert _c_plan(cfg, [0, 0], [-1, 100, 500], (98, 10))[0] == EINVAL
    assert _c_plan(cfg, [0, -1], good, (98, 10))[0] == EINVAL and "received" in dl.last_error()
    assert _c_plan(cfg, [0, 0], [0, 100, 2**31 + 100], (98, 10))[0] == EINVAL
    assert _c_plan(cfg, [0, 2**63 - 5], good, (98, 10))[0] == EINVAL
    for bad in ((0, 1), (98, 0), (-1, 1)):
        assert _c_plan(cfg, [0, 0], good, bad)[0] == EINVAL and "window_frames" in dl.last_error()
    assert _c_plan(cfg, [0, 0], good, (10, 25))[0] == EINVAL and "hop_frames > window_frames" in dl.last_error()
    for kw in (dict(hop_length=0), dict(frame_length=401), dict(n_fft=300), dict(hop_length=480)):
        assert _c_plan(dsp_amd.default_config(**kw), [0, 0], good, (98, 10))[0] == EINVAL, kw
    assert "hop_length > frame_length" in dl.last_error()
    sj = dl.MfccConfig()
    L.dsp_mfcc_scrubjay_infer_config(C.byref(sj), 16000)           # stream framing: other row counts
    assert _c_plan(sj, [0, 0], good, None)[0] == EINVAL and "DSP_FRAMING_COMPLETE" in dl.last_error()


def test_session_entries_refuse_before_any_device_work():
    L = dl.load()
    cfg = dl.ScanConfig(98, 10)
    h = C.c_void_p(1)
    assert L.dsp_stream_session_create(None, None, None, C.byref(cfg), 4, 1, 0, 0, C.byref(h)) == -1 and h.value is None
    assert L.dsp_stream_session_create(None, None, None, C.byref(cfg), 4, 1, 0, 0, None) == -1
    co = np.array([0, 16000], np.int64)
    assert L.dsp_stream_push_device(None, None, co.ctypes.data_as(LP), None, None, None, None, None, None, None) == -1
    assert L.dsp_stream_session_reset(None, None, 0, None) == -1
    assert L.dsp_stream_session_counts(None, None, None, None) == -1
    L.dsp_stream_session_destroy(None)


def test_stream_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in STREAM_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name


def test_stream_wrapper_checks_raise_under_python_O():
    code = """
import dsp_amd
cfg = dsp_amd.default_config()
for args in ((None, [0, 100, 99]), (None, [-1, 100]), (None, []), (None, [[0, 1]]), ([0, 0], [0, 100]), ([-1], [0, 100]),
             (None, [0, 100], 98), (None, [0, 100], 0, 10), (None, [0, 100], 98, 0), (None, [0, 100], 10, 25)):
    try:
        dsp_amd.stream_push_plan(cfg, *args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for {args}")
class Plan:
    _h, device, cfg = None, 0, cfg
import torch
for kw in (dict(dtype=torch.float64), dict(n_streams=-1), dict(channels=3), dict(channels=2), dict(stereo_mode=2),
           dict(stop=object(), window_frames=0), dict(stop=object(), window_frames=10, hop_frames=25)):
    kw.setdefault("n_streams", 4)
    try:
        dsp_amd.StreamSession(Plan(), **kw)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for {kw}")
s = object.__new__(dsp_amd.StreamSession)
s.n_streams, s.dtype, s.channels, s.device = 2, torch.float32, 1, 0
for chunks, co in ((torch.zeros(8), [0, 4, 8]), ([0.0] * 8, [0, 4, 8])):
    try:
        s.push(chunks, co)
    except ValueError:
        continue
    raise SystemExit("no ValueError for a push of something that is not a CUDA tensor")
try:
    s.reset([2])
except ValueError:
    print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
