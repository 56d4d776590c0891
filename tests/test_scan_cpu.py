"""CPU: the host side of window scans -- dsp_scan_window_offsets (no GPU call) against a plain restatement of the window rule, the
argument checks the scan entry points make before any device work, the exports, and the Python wrappers' checks under python -O."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_SYMBOLS = ["dsp_scan_window_offsets", "dsp_stop_scan_device", "dsp_speaker_scan_device", "dsp_scanner_create", "dsp_scanner_destroy",
                "dsp_scanner_run_device", "dsp_scanner_run_pcm16_device"]


def _count(rows, wf, hop):
    """recording of `rows` MFCC rows: 1 + (rows - wf) // hop windows of wf rows, or one window of all rows when it has fewer"""
    return 1 if rows < wf else 1 + (rows - wf) // hop


def _c_plan(fo, wf, hop):
    L = dl.load()
    fo = np.ascontiguousarray(fo, np.int64)
    wo = np.full(fo.size, -7, np.int64)
    lp = C.POINTER(C.c_long)
    total = L.dsp_scan_window_offsets(C.byref(dl.ScanConfig(wf, hop)), fo.ctypes.data_as(lp), fo.size - 1, wo.ctypes.data_as(lp))
    return total, wo


@pytest.mark.parametrize("wf,hop", [(98, 10), (98, 1), (98, 98), (10, 25), (500, 1), (600, 7), (1, 1)])
def test_window_counts_follow_the_rule(wf, hop):
    rows = [0, wf - 1, wf, wf + hop - 1, wf + hop, 1, 3 * wf + 5, 0, 60000, wf + 2 * hop]
    fo = np.concatenate([[0], np.cumsum(rows)])
    want = np.concatenate([[0], np.cumsum([_count(r, wf, hop) for r in rows])])
    total, wo = _c_plan(fo, wf, hop)
    assert total == want[-1]
    np.testing.assert_array_equal(wo, want)
    np.testing.assert_array_equal(dsp_amd.scan_window_offsets(fo, wf, hop), want)
    # the matrix need not start at row 0: only the recordings' row counts matter
    total2, wo2 = _c_plan(fo + 1234, wf, hop)
    assert total2 == total and np.array_equal(wo2, wo)


def test_edge_cases_by_hand():
    assert dsp_amd.scan_window_offsets([0, 0], 98, 10).tolist() == [0, 1]                 # R = 0: one window, as classify_signal on a short clip
    assert dsp_amd.scan_window_offsets([0, 97], 98, 10).tolist() == [0, 1]                # R < window
    assert dsp_amd.scan_window_offsets([0, 98], 98, 10).tolist() == [0, 1]                # R = window
    assert dsp_amd.scan_window_offsets([0, 98 + 9], 98, 10).tolist() == [0, 1]            # R = window + hop - 1
    assert dsp_amd.scan_window_offsets([0, 98 + 10], 98, 10).tolist() == [0, 2]
    assert dsp_amd.scan_window_offsets([0, 100], 10, 25).tolist() == [0, 4]               # hop larger than the window: rows skipped
    assert dsp_amd.scan_window_offsets([5], 98, 10).tolist() == [0]                       # no recordings
    # one hour at 16 kHz: 359 998 rows, 1 s windows every 100 ms
    rows = 1 + (3600 * 16000 - 400) // 160
    assert dsp_amd.scan_window_offsets([0, rows], 98, 10).tolist() == [0, 1 + (rows - 98) // 10]


def test_planner_refusals():
    L = dl.load()
    lp = C.POINTER(C.c_long)
    fo = np.array([0, 100, 200], np.int64)
    wo = np.zeros(3, np.int64)
    f, w = fo.ctypes.data_as(lp), wo.ctypes.data_as(lp)
    good = dl.ScanConfig(98, 10)
    assert L.dsp_scan_window_offsets(C.byref(good), f, 0, w) == 0                            # n_recordings = 0
    assert L.dsp_scan_window_offsets(None, f, 2, w) == -1
    for bad in (dl.ScanConfig(0, 10), dl.ScanConfig(98, 0), dl.ScanConfig(-1, 1)):
        assert L.dsp_scan_window_offsets(C.byref(bad), f, 2, w) == -1
        assert "window_frames" in dl.last_error()
    assert L.dsp_scan_window_offsets(C.byref(good), None, 2, w) == -1
    assert L.dsp_scan_window_offsets(C.byref(good), f, 2, None) == -1
    assert L.dsp_scan_window_offsets(C.byref(good), f, -1, w) == -1
    dec = np.array([0, 100, 99, 200], np.int64)
    assert L.dsp_scan_window_offsets(C.byref(good), dec.ctypes.data_as(lp), 3, np.zeros(4, np.int64).ctypes.data_as(lp)) == -1
    assert "recording 1" in dl.last_error()
    neg = np.array([-1, 100], np.int64)
    assert L.dsp_scan_window_offsets(C.byref(good), neg.ctypes.data_as(lp), 1, w) == -1


def test_device_entries_refuse_before_any_device_work():
    L = dl.load()
    lp = C.POINTER(C.c_long)
    fo = np.array([0, 100], np.int64)
    f = fo.ctypes.data_as(lp)
    cfg = dl.ScanConfig(98, 10)
    assert L.dsp_stop_scan_device(None, None, 1, f, C.byref(cfg), None, None) == -1
    assert L.dsp_speaker_scan_device(None, None, 1, f, C.byref(cfg), None, None, None) == -1
    h = C.c_void_p(1)
    assert L.dsp_scanner_create(None, None, None, C.byref(cfg), C.byref(h)) == -1 and h.value is None
    assert L.dsp_scanner_create(None, None, None, C.byref(cfg), None) == -1
    off = np.array([0, 16000], np.int64)
    assert L.dsp_scanner_run_device(None, None, 1, off.ctypes.data_as(lp), None, None, None, None) == -1
    assert L.dsp_scanner_run_pcm16_device(None, None, 1, off.ctypes.data_as(lp), 3, 0, None, None, None, None) == -1
    assert L.dsp_scanner_run_pcm16_device(None, None, 1, off.ctypes.data_as(lp), 2, 7, None, None, None, None) == -1
    L.dsp_scanner_destroy(None)


def test_scan_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in SCAN_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name


def test_wrapper_checks_raise_under_python_O():
    code = """
import dsp_amd
for args in (([0, 100], 0, 10), ([0, 100], 98, 0), ([0, 100, 99], 98, 10), ([-1, 100], 98, 10), ([], 98, 10), ([[0, 1]], 98, 10)):
    try:
        dsp_amd.scan_window_offsets(*args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for {args}")
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
