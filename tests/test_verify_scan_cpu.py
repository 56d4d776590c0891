"""CPU: the float speaker scan (include/dsp_amd.h dsp_speaker_float_scan_device) -- that the window-sum form of its numpy
restatement (tests/verify_scan_ref.py) is verify_ref.verify on the cut-out windows, exactly; that its window counts are
dsp_scan_window_offsets'; that the shared cases decide `best` on most windows by the restatement alone; the export; and the argument
checks the entry makes before it touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import verify_ref as V
from tests import verify_scan_ref as VS
from tests.enroll_util import ROOT
from tests.verify_scan_util import SCAN_CONFIGS, SCAN_KD, SCAN_LEAD, SCAN_LENS, SCAN_OTHER_D, SCAN_SPEAKERS, scan_case, scan_ref
from tests.verify_util import decided, subset

NAME = "dsp_speaker_float_scan_device"


def test_window_sums_are_clip_sums():
    """the array form of the window sum is verify_ref.clip_sum per (window, model), bit for bit -- part tiles, one tile, several"""
    rng = np.random.default_rng(5)
    ll = rng.normal(-20.0, 5.0, (3, 300)).astype(np.float32)
    for n, hop, count in ((1, 1, 300), (63, 7, 34), (64, 64, 4), (65, 1, 236), (130, 100, 2), (300, 9, 1)):
        got = VS.window_sums(ll, n, hop, count)
        want = np.array([[V.clip_sum(ll[m, w * hop:w * hop + n]) for w in range(count)] for m in range(3)])
        assert got.shape == (3, count) and got.dtype == np.float64 and np.array_equal(got, want), (n, hop)


@pytest.mark.parametrize("window,hop", [(98, 10), (30, 45)])
def test_restatement_is_verify_on_the_cut_out_windows(window, hop):
    """both arithmetics, all five outputs, exactly: the scan of the (5, 13) case and verify_ref.verify on its windows as clips"""
    case = scan_case(5, 13)
    rows, clip_fo = VS.cut_windows(case["feats"], case["fo"], window, hop)
    assert not np.any(rows == 77.0)
    for dtype, ref in zip((np.float64, np.float32), scan_ref(5, 13, window, hop)):
        clips = V.verify(rows, clip_fo, case["ubm"], case["means"], dtype)
        direct = VS.scan(case["feats"], case["fo"], case["ubm"], case["means"], window, hop, dtype)
        for key in V.OUTPUTS:
            assert ref[key].dtype == clips[key].dtype and np.array_equal(ref[key], clips[key]), (dtype, key)
            assert np.array_equal(direct[key], clips[key]), (dtype, key)


def test_window_counts_are_the_librarys():
    fo = scan_case(1, 1)["fo"]
    assert np.diff(fo).tolist() == SCAN_LENS and fo[0] == SCAN_LEAD
    for window, hop in SCAN_CONFIGS + [(700, 3), (701, 1), (2, 5)]:
        wo = dsp_amd.scan_window_offsets(fo, window, hop)
        assert np.array_equal(np.diff(wo), VS.window_counts(fo, window, hop)), (window, hop)
        start, n = VS.window_spans(fo, window, hop)
        assert start.size == n.size == wo[-1]
        for r in range(fo.size - 1):                                               # every window lies inside its recording
            s, m = start[wo[r]:wo[r + 1]], n[wo[r]:wo[r + 1]]
            assert s[0] == fo[r] and np.all(s + m <= fo[r + 1]) and np.all(np.diff(s) == hop) and np.all(m == min(window, fo[r + 1] - fo[r]))
    assert VS.window_counts(fo, 1, 1).sum() == 1431 and VS.window_counts(fo, 98, 10).tolist() == [1, 1, 1, 1, 1, 2, 16, 61]


@pytest.mark.parametrize("k,d", SCAN_KD)
def test_scan_inputs_decide_best_by_the_restatement_alone(k, d):
    """for every scan configuration and speaker count the float64 runner-up is more than 2 gates below the maximum on at least half of
    the windows, and there the float32 model names the float64 argmax; `best` changes inside the longest recording"""
    case = scan_case(k, d)
    assert np.isclose((1.0 / case["ubm"]["inv_covs"]).min(), 1e-6) and case["means"].shape == (SCAN_SPEAKERS[-1], k, d)
    for window, hop in SCAN_CONFIGS:
        want_all, model_all = scan_ref(k, d, window, hop)
        for n_spk in SCAN_SPEAKERS:
            want, model = subset(want_all, n_spk), subset(model_all, n_spk)
            gates = V.gates(want, model)
            sure = decided(want["llr"], gates["llr"])
            print(f"\nk {k} d {d} window {window} hop {hop} S {n_spk}: llr gate {gates['llr']:.3e}, decided {int(sure.sum())} of {sure.size}")
            assert np.isfinite(want["llr"]).all() and np.isfinite(model["llr"]).all()
            assert sure.sum() * 2 >= sure.size, (k, d, window, hop, n_spk)
            assert np.array_equal(model["best"][sure], want["best"][sure])
        wo = dsp_amd.scan_window_offsets(case["fo"], window, hop)
        assert np.unique(want_all["best"][wo[-2]:wo[-1]]).size > 1, (window, hop)


@pytest.mark.parametrize("d", SCAN_OTHER_D)
def test_other_d_inputs_decide_best_too(d):
    """the cases of the GPU test of the other d, against all 33 speakers at (98, 10)"""
    want, model = scan_ref(5, d, 98, 10)
    sure = decided(want["llr"], V.gates(want, model)["llr"])
    assert sure.sum() * 2 >= sure.size and np.array_equal(model["best"][sure], want["best"][sure])


def test_scan_symbol_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\b" + NAME + r"\(", header)
    assert NAME in dl.SYMBOLS and hasattr(L, NAME) and NAME in set(re.findall(r"\bT (\w+)$", nm, re.M))
    assert hasattr(dsp_amd.SpeakerVerifier, "scan")


def _einval(rc, *words):
    assert rc == -1 and dl.last_error() != "" and all(w in dl.last_error() for w in words), (rc, dl.last_error())


def test_bad_arguments_are_einval_before_any_device_work():
    L = dl.load()
    arr = np.ones(4 * 3)
    v = C.c_void_p()
    p = dl.GmmFloatParams(4, 3, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)
    assert L.dsp_speaker_verifier_create(C.byref(p), 0, C.byref(v)) == 0 and v.value, dl.last_error()      # no device is needed
    off = lambda *a: (C.c_long * len(a))(*a)                                    # noqa: E731
    X, M, O = 0x1000, 0x2000, 0x3000                                             # never dereferenced: every call below is refused first
    good = dl.ScanConfig(98, 10)

    def call(n_rec=2, offsets=off(0, 5, 9), n_spk=3, ver=v, feats=X, means=M, cfg=good, outs=(O, None, None, None, None)):
        return L.dsp_speaker_float_scan_device(ver, feats, n_rec, offsets, C.byref(cfg) if cfg is not None else None, means, n_spk, *outs, None)

    _einval(call(ver=None), "verifier")
    _einval(call(cfg=None), "dsp_scan_config")
    _einval(call(cfg=dl.ScanConfig(0, 10)), "window_frames")
    _einval(call(cfg=dl.ScanConfig(98, 0)), "hop_frames")
    _einval(call(cfg=dl.ScanConfig(-1, -1)), "window_frames", "hop_frames")
    _einval(call(feats=None), "d_feats")
    _einval(call(means=None), "d_means")
    _einval(call(offsets=None), "frame_offsets")
    _einval(call(outs=(None,) * 5), "every output", "NULL")
    _einval(call(offsets=off(0, 9, 5)), "frame_offsets", "decrease", "recording 1")
    _einval(call(offsets=off(-1, 5, 9)), "frame_offsets", "non-negative")
    _einval(call(n_rec=3, offsets=off(0, 5, 5, 9)), "recording 1", "no rows")
    _einval(call(n_rec=1, offsets=off(4, 4)), "recording 0", "no rows")
    _einval(call(n_rec=-1), "n_recordings", ">= 0")
    _einval(call(n_spk=-2), "n_speakers", ">= 0")
    _einval(call(n_spk=(1 << 19) + 1), "speakers", "2^19")
    _einval(call(n_rec=(1 << 30) + 1), "recordings", "2^30")
    # zero recordings or zero speakers: DSP_OK, no launch, no device -- whatever else is passed
    assert call(n_rec=0, offsets=None) == 0 and call(n_spk=0) == 0
    assert call(n_rec=0, offsets=None, feats=None, means=None, cfg=None, outs=(None,) * 5) == 0
    if L.dsp_device_count() <= 0:
        for out in range(5):                                                     # any single output will do: the next refusal is the device's
            outs = tuple(O if i == out else None for i in range(5))
            for cfg in (good, dl.ScanConfig(1, 1), dl.ScanConfig(3, 7)):
                assert call(outs=outs, cfg=cfg) == -2 and "no HIP device" in dl.last_error()      # DSP_ENODEV, after every argument check
    L.dsp_speaker_verifier_destroy(v)


def test_scan_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
ubm = {"log_consts": np.zeros(4), "means": np.zeros((4, 3)), "inv_covs": np.ones((4, 3))}
v = dsp_amd.SpeakerVerifier(ubm)                       # touches no device
x, m = torch.zeros(8, 3), torch.zeros(2, 4, 3)
for call in (lambda: v.scan(x, [0, 8], m, 98, 10), lambda: v.scan(np.zeros((8, 3), np.float32), [0, 8], m, 98, 10),
             lambda: v.scan(x, [0, 8, 4], m, 98, 10), lambda: v.scan(x, [], m, 98, 10), lambda: v.scan(x, [0, 8], m, 98, 10, want=()),
             lambda: v.scan(x, [0, 8], m, 98, 10, want=("llr", "score")), lambda: v.scan(x, [0, 8], m, 0, 10),
             lambda: v.scan(x, [0, 8], m, 98, 0), lambda: v.scan(x, [0, 4, 4, 8], m, 98, 10)):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for a bad scan argument")
try:
    v.scan(x, [0, 4, 4, 8], m, 98, 10)
except ValueError as e:
    if "recording 1" not in str(e):
        raise SystemExit(f"the recording without rows is not named: {e}")
v.close()
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
