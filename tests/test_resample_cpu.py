"""CPU: the host side of the polyphase FIR resampler (include/dsp_amd.h dsp_resample_*) -- ratio, taps and output offsets against
scipy.signal, the definition's numpy restatement (tests/resample_ref.py) against scipy.signal.resample_poly and the pinned golden, the
argument checks made before any device work, the exports, the Python wrappers' checks under python -O, and the choice of clips for
the GPU composition test."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from oracle import oracle as O
from tests import resample_ref as R
from tests.conftest import gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = R.RATE_PAIRS + [(1, 1024), (1024, 1)]
RESAMPLE_SYMBOLS = ["dsp_resample_ratio", "dsp_resample_geometry", "dsp_resample_taps", "dsp_resample_offsets", "dsp_resampler_create", "dsp_resampler_destroy",
                    "dsp_resample_ragged_device", "dsp_resample_ragged_pcm16_device", "dsp_resample_clips_device",
                    "dsp_resample_clips_pcm16_device", "dsp_resample_host"]
COMPOSITION_CLIPS = ("chirp", "stop1")       # tests/test_gpu_resample.py resamples these on the GPU


def composition_clip(golden, name):
    """a golden 16 kHz clip in float64"""
    if name == "chirp":
        return golden("mfcc_ref.npz")["input__chirp"].astype(np.float64)
    return golden("stop_ref.npz")["clip1__pcm"].astype(np.float64) / 32768.0


def lengths(up, half):
    return [0, 1, 7, half // up + 3, 997]


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_ratio_is_the_reduced_fraction(rate_in, rate_out):
    from fractions import Fraction
    up, down, half = dsp_amd.resample_ratio(rate_in, rate_out)
    f = Fraction(rate_out, rate_in)
    assert (up, down, half) == (f.numerator, f.denominator, 10 * max(f.numerator, f.denominator)) == R.ratio(rate_in, rate_out)
    L = dl.load()
    assert L.dsp_resample_ratio(rate_in, rate_out, None, None, None) == 0          # any pointer may be NULL
    assert L.dsp_resample_taps(rate_in, rate_out, None, 0) == 2 * half + 1


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_taps_are_firwin_times_up(rate_in, rate_out):
    """The taps are a closed formula evaluated in float64: the budget is rounding only.  Measured here, worst deviation from
    scipy 1.15.3's firwin(2 half + 1, 1 / m, window=("kaiser", 5.0)) * up relative to the largest tap over the thirteen pairs:
    9.2e-16 for the library (22050 and 44100 -> 16000), 6.2e-16 for the numpy restatement.  The gate is 16 x 9.2e-16 = 1.5e-14, under the
    hard cap of 1e-12.  16000 -> 16000 has m = 1, a cutoff firwin refuses (resample_poly copies): there the library and the restatement
    are held to each other."""
    from scipy.signal import firwin
    up, down, half = dsp_amd.resample_ratio(rate_in, rate_out)
    h = dsp_amd.resample_taps(rate_in, rate_out)
    assert h.shape == (2 * half + 1,) and h.dtype == np.float64
    want = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up if max(up, down) > 1 else R.taps(rate_in, rate_out)
    tol = min(16 * 9.2e-16, 1e-12)
    worst = np.abs(h - want).max() / np.abs(want).max()
    worst_ref = np.abs(R.taps(rate_in, rate_out) - want).max() / np.abs(want).max()
    print(f"taps {rate_in} -> {rate_out}: library {worst:.2e}, restatement {worst_ref:.2e} of the largest tap")
    assert worst <= tol and worst_ref <= tol
    assert np.array_equal(h, h[::-1]) or np.abs(h - h[::-1]).max() <= tol * np.abs(h).max()      # zero phase: symmetric


@pytest.mark.parametrize("rate_in,rate_out", PAIRS)
def test_offsets_are_resample_polys_lengths(rate_in, rate_out):
    from scipy.signal import resample_poly
    up, down, half = dsp_amd.resample_ratio(rate_in, rate_out)
    ns = lengths(up, half)
    offs = np.concatenate([[5], 5 + np.cumsum(ns)])
    got = dsp_amd.resample_offsets(rate_in, rate_out, offs)
    want = [0]
    for n in ns:
        want.append(want[-1] + len(resample_poly(np.zeros(n), up, down)))
    assert got.tolist() == want == R.offsets(rate_in, rate_out, offs).tolist()
    out = (C.c_long * 1)(-7)
    assert dl.load().dsp_resample_offsets(rate_in, rate_out, None, 0, out) == 0 and out[0] == 0       # zero recordings


@pytest.mark.parametrize("rate_in,rate_out", R.RATE_PAIRS)
def test_restatement_is_resample_poly(rate_in, rate_out):
    """tests/resample_ref.py in float64 against scipy.signal.resample_poly on seeded |x| <= 1.  Both are float64 sums of at most
    2 half / up + 1 products of the same taps: the budget is rounding only.  Measured here over the eleven pairs and these lengths:
    at most 8.9e-16 (11025 -> 16000).  The gate is 16 x that, 1.5e-14."""
    from scipy.signal import resample_poly
    up, down, half = R.ratio(rate_in, rate_out)
    rng = np.random.default_rng(2024 + rate_in)
    worst = 0.0
    for n in lengths(up, half) + [5000]:
        x = rng.uniform(-1, 1, n)
        want = resample_poly(x, up, down)
        got = R.resample(x, rate_in, rate_out)
        assert got.shape == want.shape == (R.out_len(n, up, down),)
        if n:
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"restatement {rate_in} -> {rate_out}: {worst:.2e}")
    assert worst <= 16 * 8.9e-16


def test_restatement_reproduces_the_golden(golden):
    """the reference's capture dump through scipy, pinned (tests/golden/make_golden_resample.py)"""
    z = golden("resample_kat.npz")
    x = z["x"]
    assert x.shape == (6768,) and x.dtype == np.float64
    for rate_in, key in ((10000, "y_10000"), (9000, "y_9000")):
        got = R.resample(x, rate_in, 16000)
        assert got.shape == z[key].shape
        assert np.abs(got - z[key]).max() <= 16 * 8.9e-16, key
        # and the float32 model stays inside the GPU tests' derived bound
        y, mag, terms = R.resample(x.astype(np.float32), rate_in, 16000, with_bound=True)
        y32 = R.resample(x.astype(np.float32), rate_in, 16000, dtype=np.float32)
        assert np.all(np.abs(y32 - y) <= (terms + 2) * 2.0 ** -24 * mag)


def test_copy_ratio_and_float32_model():
    x = np.random.default_rng(3).uniform(-1, 1, 100).astype(np.float32)
    assert np.array_equal(R.resample(x, 16000, 16000, dtype=np.float32), x)
    assert R.resample(np.zeros(0), 48000, 16000).shape == (0,)


def _einval(rc):
    assert rc == -1 and dl.last_error() != "", (rc, dl.last_error())


def test_bad_arguments_are_einval_with_a_reason():
    L = dl.load()
    i = C.c_int()
    h = (C.c_double * 64)()
    out = (C.c_long * 4)()
    off = lambda *a: (C.c_long * len(a))(*a)       # noqa: E731
    for ri, ro in ((0, 16000), (16000, 0), (-1, 16000), (16000, -5), (1, 1025), (1025, 1), (2049, 2050), (44101, 16000)):
        _einval(L.dsp_resample_ratio(ri, ro, C.byref(i), C.byref(i), C.byref(i)))
        _einval(L.dsp_resample_taps(ri, ro, None, 0))
        _einval(L.dsp_resample_offsets(ri, ro, off(0, 4), 1, out))
        hnd = C.c_void_p()
        _einval(L.dsp_resampler_create(0, ri, ro, C.byref(hnd)))
        assert not hnd.value
        _einval(L.dsp_resample_host(ri, ro, h, 4, h))
    assert "1024" in dl.last_error()
    _einval(L.dsp_resample_taps(8000, 16000, h, 40))                                # 41 taps do not fit
    for bad in (off(0, 4, 3), off(-1, 4, 5), off(0, 2**31, 2**31 + 1)):               # decreasing, negative, a recording of 2^31 samples
        _einval(L.dsp_resample_offsets(48000, 16000, bad, 2, out))
    _einval(L.dsp_resample_offsets(48000, 16000, None, 2, out))
    _einval(L.dsp_resample_offsets(48000, 16000, off(0, 4, 8), 2, None))
    _einval(L.dsp_resample_offsets(48000, 16000, off(0, 4, 8), -1, out))
    _einval(L.dsp_resampler_create(0, 48000, 16000, None))
    # the device entries refuse a NULL resampler / bad PCM layout before they touch a GPU
    _einval(L.dsp_resample_ragged_device(None, None, 1, off(0, 4), None, None))
    _einval(L.dsp_resample_ragged_pcm16_device(None, None, 1, off(0, 4), 3, 0, None, None))
    _einval(L.dsp_resample_ragged_pcm16_device(None, None, 1, off(0, 4), 2, 7, None, None))
    _einval(L.dsp_resample_clips_device(None, None, 1, 4, 4, None, 4, None))
    _einval(L.dsp_resample_clips_pcm16_device(None, None, 1, 4, 4, 0, 0, None, 4, None))
    _einval(L.dsp_resample_host(48000, 16000, None, 4, h))
    _einval(L.dsp_resample_host(48000, 16000, h, -1, h))
    _einval(L.dsp_resample_host(48000, 16000, h, 2**31, h))
    assert L.dsp_resample_host(48000, 16000, None, 0, None) == 0                    # no samples: no output, no GPU


def test_resample_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in RESAMPLE_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_resampl")) == sorted(RESAMPLE_SYMBOLS)


def test_resample_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
for f, args in ((dsp_amd.resample_ratio, (0, 16000)), (dsp_amd.resample_ratio, (16000, -1)), (dsp_amd.resample_ratio, (48000.0, 16000)),
                (dsp_amd.resample_taps, (0, 0)), (dsp_amd.resample_taps, (True, 16000)), (dsp_amd.resample_offsets, (0, 16000, [0, 4])),
                (dsp_amd.resample_offsets, (48000, 16000, [])), (dsp_amd.resample_offsets, (48000, 16000, [[0, 4]])),
                (dsp_amd.Resampler, (0, 16000)), (dsp_amd.Resampler, (48000, 2**31))):
    try:
        f(*args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for {f.__name__}{args}")
for f, args in ((dsp_amd.resample_ratio, (1, 1025)), (dsp_amd.resample_offsets, (48000, 16000, [0, 4, 3])), (dsp_amd.Resampler, (1025, 1))):
    try:
        f(*args)
    except dsp_amd.DspError:
        continue
    raise SystemExit(f"no DspError for {f.__name__}{args}")
r = object.__new__(dsp_amd.Resampler)
r.rate_in, r.rate_out, r.up, r.down, r.half, r.device, r._h = 48000, 16000, 1, 3, 30, 0, None
for args in ((torch.zeros(8), [0, 8]), ([0.0] * 8, [0, 8]), (np.zeros(8, np.float32), [0, 8])):
    try:
        r.ragged(*args)
    except ValueError:
        continue
    raise SystemExit("no ValueError for a ragged signal that is not a CUDA tensor")
for args in ((torch.zeros(2, 8),), (torch.zeros(2, 8, dtype=torch.int16),), (np.zeros((2, 8), np.float32),)):
    try:
        r.clips(*args)
    except ValueError:
        continue
    raise SystemExit("no ValueError for clips that are not a CUDA tensor")
for call in (lambda: r.ragged(torch.zeros(8), [0, 8], stereo_mode=2), lambda: r.clips(torch.zeros(2, 8), stereo_mode=-1), lambda: r.out_samples(-1)):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for a bad stereo_mode / length")
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.parametrize("name", COMPOSITION_CLIPS)
def test_composition_clips_pass_the_mfcc_gate_in_the_float32_model(golden, name):
    """The GPU composition test (48 kHz -> 16 kHz, then MfccPlan.clips) compares MFCC rows of the GPU's resampling with MFCC rows of the
    float64 resampling under the 1e-4-of-frame-L-inf gate.  That is only a fair demand on clips where float32 resampling itself -- the
    sequential model of tests/resample_ref.py -- passes it: checked here, through the oracle's MFCC."""
    x48 = R.resample(composition_clip(golden, name), 16000, 48000).astype(np.float32)
    want = R.resample(x48, 48000, 16000).astype(np.float32)
    model = R.resample(x48, 48000, 16000, dtype=np.float32)
    assert want.shape == model.shape == (16000,)
    gate(O.compute_mfcc(model, 98), O.compute_mfcc(want, 98), f"resample_model_{name}")
