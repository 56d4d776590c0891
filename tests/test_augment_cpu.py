"""CPU: the host side of the clip augmenter (include/dsp_amd.h dsp_augment_*, dsp_stft_frames ...) against its numpy
restatement (tests/augment_ref.py) -- frame counts and stretched lengths with their rint ties, the pitch ratio against a brute-force
search, the normal draws and the policy's ops, the refusals made before any device work, the exports -- and properties of the
restatement itself: a stretched sine keeps its frequency, rate 1 reproduces the input, silence stays silence."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import augment_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUGMENT_SYMBOLS = ["dsp_stft_frames", "dsp_stretch_frames", "dsp_stretch_length", "dsp_pitch_ratio", "dsp_augment_normal", "dsp_augment_out_offsets",
                   "dsp_augment_draw", "dsp_augmenter_create", "dsp_augmenter_destroy", "dsp_stft_ragged_device", "dsp_istft_ragged_device",
                   "dsp_time_stretch_ragged_device", "dsp_augment_ragged_device"]
LENGTHS = [1, 5, 511, 512, 513, 1024, 1025, 1536, 2047, 2048, 2049, 2560, 5000, 22050]
RATES = [0.5, 0.8, 1.0, 1.2, 2.0, 196 / 185, 49 / 55, 0.125, 8.0, 1.25]


def test_frames_and_lengths_follow_the_restatement():
    for n in LENGTHS:
        T = dsp_amd.stft_frames(n)
        assert T == A.stft_frames(n) == 1 + n // 512
        for rate in RATES:
            assert dsp_amd.stretch_frames(T, rate) == A.stretch_frames(T, rate), (n, rate)
            assert dsp_amd.stretch_length(n, rate) == A.stretch_length(n, rate), (n, rate)
    # rint ties go to even, and the result is at least 1
    assert dsp_amd.stretch_length(5, 2.0) == 2 and dsp_amd.stretch_length(7, 2.0) == 4 and dsp_amd.stretch_length(3, 2.0) == 2
    assert dsp_amd.stretch_length(1, 2.0) == 1 and dsp_amd.stretch_length(1, 8.0) == 1 and dsp_amd.stretch_length(0, 1.0) == 1
    assert dsp_amd.stretch_frames(44, 2.0) == 22 and dsp_amd.stretch_frames(43, 2.0) == 22 and dsp_amd.stretch_frames(3, 0.8) == 4


@pytest.mark.parametrize("max_term", [256, 1024, 16])
def test_pitch_ratio_is_the_nearest_fraction(max_term):
    for n_steps in range(-12, 13):
        got = dsp_amd.pitch_ratio(n_steps, 12, max_term)
        if max_term == 1024 and n_steps % 4:
            continue                                       # (the brute force over 1024 x 1024 fractions: a few steps are enough)
        assert got == A.pitch_ratio(n_steps, 12, max_term), (n_steps, max_term)
    assert dsp_amd.pitch_ratio(0) == (1, 1) and dsp_amd.pitch_ratio(12) == (1, 2) and dsp_amd.pitch_ratio(-12) == (2, 1)


def test_pitch_ratios_of_one_and_two_semitones():
    want = {1: (185, 196), -1: (196, 185), 2: (49, 55), -2: (55, 49)}
    for n_steps, (up, down) in want.items():
        assert dsp_amd.pitch_ratio(n_steps) == (up, down)
        cents = abs(1200.0 * np.log2((up / down) / 2.0 ** (-n_steps / 12)))
        assert cents < (0.007 if abs(n_steps) == 1 else 0.03), (n_steps, cents)


def test_normal_draws_are_the_restatement():
    for seed, key in ((0, 0), (7, 3), (2**63 + 5, 2**64 - 1)):
        got = dsp_amd.augment_normal(seed, key, np.arange(257))
        want = A.normal(seed, key, 257)
        assert np.abs(got - want).max() <= 1e-14, (seed, key)
    # the draws are dsp_stop_train_uniform's generator: the same 64 bits
    d = int(A.draw(7, 3, 11))
    assert dsp_amd.stop_train_uniform(7, 3, 11) == (d >> 11) * 2.0 ** -53
    z = A.normal(1, 2, 65536)
    assert abs(z.mean()) < 5 / 256 and abs(z.std() - 1) < 0.02 and np.isfinite(z).all()


def test_policy_ops_are_the_restatement():
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 2, 400)
    for seed, prob in ((0, 0.5), (9, 1.0), (9, 0.0), (3, 0.25)):
        ops = dsp_amd.augment_draw(labels, prob, seed)
        want = A.augment_draw(seed, labels, prob)
        assert len(ops) == len(want)
        for got, w in zip(ops, want):
            assert (int(got["clip"]), int(got["kind"]), int(got["n_steps"]), int(got["key"])) == (w[0], w[1], w[3], w[5])
            assert got["rate"] == w[2] and got["sigma"] == np.float32(w[4])
    ops = dsp_amd.augment_draw(np.ones(3000, int), 1.0, 1)
    assert len(ops) == 3000 and set(ops["kind"]) == {0, 1, 2} and set(ops["n_steps"][ops["kind"] == 1]) == {-2, -1, 0, 1, 2}
    r = ops["rate"][ops["kind"] == 0]
    assert 0.8 <= r.min() < 0.81 and 1.19 < r.max() <= 1.2
    assert len(dsp_amd.augment_draw(np.zeros(50, int), 1.0, 1)) == 0
    # a cap that is too small is refused
    L = dl.load()
    buf = (dl.AugmentOp * 2)()
    lab = (C.c_int * 8)(*([1] * 8))
    assert L.dsp_augment_draw(1, lab, 8, 1.0, None, 0) == 8
    assert L.dsp_augment_draw(1, lab, 8, 1.0, buf, 2) == -1 and "cap" in dl.last_error()


def test_out_offsets_follow_the_ops():
    offsets = [3, 2003, 2003, 7003]
    lens = np.diff(offsets)
    ops = [(0, 0, 0.8, 0, 0.0, 0), (2, 1, 1.0, 2, 0.0, 1), (1, 2, 1.0, 0, 0.005, 2), (2, 0, 2.0, 0, 0.0, 3), (0, 2, 1.0, 0, 0.0, 4)]
    got = dsp_amd.augment_out_offsets(offsets, ops)
    assert got.tolist() == np.concatenate([[0], np.cumsum(A.out_lengths(lens, ops))]).tolist() == [0, 2500, 7500, 7500, 10000, 12000]
    assert dsp_amd.augment_out_offsets(offsets, []).tolist() == [0]


def _einval(rc):
    assert rc == -1 and dl.last_error() != "", (rc, dl.last_error())


def test_bad_arguments_are_einval_with_a_reason():
    L = dl.load()
    i = C.c_int()
    out = (C.c_long * 4)()
    off = (C.c_long * 3)(0, 2000, 2**24 + 2000)
    _einval(L.dsp_stft_frames(-1))
    for rate in (0.1249, 8.01, float("nan"), float("inf"), 0.0, -1.0):
        _einval(L.dsp_stretch_frames(10, rate))
        _einval(L.dsp_stretch_length(10, rate))
        op = (dl.AugmentOp * 1)(dl.AugmentOp(0, dl.AUGMENT_STRETCH, rate, 0, 0.0, 0))
        _einval(L.dsp_augment_out_offsets(off, 2, op, 1, out))
        assert "rate" in dl.last_error()
    _einval(L.dsp_pitch_ratio(1, 0, 256, C.byref(i), C.byref(i)))
    _einval(L.dsp_pitch_ratio(1, 12, 0, C.byref(i), C.byref(i)))
    _einval(L.dsp_pitch_ratio(1, 12, 1025, C.byref(i), C.byref(i)))
    _einval(L.dsp_pitch_ratio(4, 1, 256, C.byref(i), C.byref(i)))                  # 2^-4 lies outside [1/8, 8]
    assert L.dsp_pitch_ratio(1, 12, 256, None, None) == 0                          # any pointer may be NULL
    for bad in (dl.AugmentOp(0, dl.AUGMENT_PITCH, 1.0, 13, 0.0, 0), dl.AugmentOp(0, dl.AUGMENT_PITCH, 1.0, -13, 0.0, 0),
                dl.AugmentOp(0, dl.AUGMENT_NOISE, 1.0, 0, -0.001, 0), dl.AugmentOp(0, dl.AUGMENT_NOISE, 1.0, 0, float("nan"), 0),
                dl.AugmentOp(2, dl.AUGMENT_NOISE, 1.0, 0, 0.0, 0), dl.AugmentOp(-1, dl.AUGMENT_NOISE, 1.0, 0, 0.0, 0),
                dl.AugmentOp(0, 3, 1.0, 0, 0.0, 0), dl.AugmentOp(1, dl.AUGMENT_NOISE, 1.0, 0, 0.0, 0)):      # (the last: a clip of 2^24 samples)
        _einval(L.dsp_augment_out_offsets(off, 2, (dl.AugmentOp * 1)(bad), 1, out))
    empty = (C.c_long * 2)(5, 5)
    _einval(L.dsp_augment_out_offsets(empty, 1, (dl.AugmentOp * 1)(dl.AugmentOp(0, dl.AUGMENT_STRETCH, 1.0, 0, 0.0, 0)), 1, out))      # n < 1
    assert L.dsp_augment_out_offsets(empty, 1, (dl.AugmentOp * 1)(dl.AugmentOp(0, dl.AUGMENT_NOISE, 1.0, 0, 0.0, 0)), 1, out) == 0
    _einval(L.dsp_augment_out_offsets(off, 2, None, 1, out))
    _einval(L.dsp_augment_out_offsets(off, 2, None, 0, None))
    _einval(L.dsp_augment_draw(0, None, 3, 0.5, None, 0))
    _einval(L.dsp_augment_draw(0, (C.c_int * 1)(1), 1, 1.5, None, 0))
    # the handle and the device entries refuse before they touch a GPU
    _einval(L.dsp_augmenter_create(0, dl.PAD_REFLECT, 256, None))
    h = C.c_void_p()
    _einval(L.dsp_augmenter_create(0, 2, 256, C.byref(h)))
    _einval(L.dsp_augmenter_create(0, dl.PAD_ZERO, 1025, C.byref(h)))
    assert not h.value
    _einval(L.dsp_stft_ragged_device(None, None, 1, off, None, None, None))
    _einval(L.dsp_istft_ragged_device(None, None, 1, off, off, None, off, None))
    _einval(L.dsp_time_stretch_ragged_device(None, None, 1, off, None, None, None))
    _einval(L.dsp_augment_ragged_device(None, None, 1, off, None, 1, 0, None, None))
    assert C.sizeof(dl.AugmentOp) == 40 == np.dtype(dl.AUGMENT_OP_DTYPE).itemsize


def test_wrapper_checks_raise_value_errors():
    for f, args in ((dsp_amd.stft_frames, (-1,)), (dsp_amd.stretch_frames, (4, 0.1)), (dsp_amd.stretch_length, (4, float("nan"))),
                    (dsp_amd.pitch_ratio, (1.5,)), (dsp_amd.pitch_ratio, (1, 12, 2000)), (dsp_amd.augment_draw, ([1, 0], 1.5)),
                    (dsp_amd.augment_draw, ([[1, 0]], 0.5)), (dsp_amd.Augmenter, (0, "wrap")), (dsp_amd.Augmenter, (0, "zero", 0)),
                    (dsp_amd.augment_out_offsets, ([0, 4], [{"clip": 0}])), (dsp_amd.augment_out_offsets, ([0, 4], [{"clip": 0, "kind": "echo"}]))):
        with pytest.raises(ValueError):
            f(*args)
    with pytest.raises(dsp_amd.DspError):
        dsp_amd.augment_out_offsets([0, 4], [{"clip": 1, "kind": "noise"}])


def test_augment_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in AUGMENT_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert "Augmenter" in dsp_amd.__all__ and "augment_kernels.hip" in dl._build.SOURCES and "capi_augment.cpp" in dl._build.SOURCES
    assert "augment_kernels.hpp" in dl._build.HEADERS


# ---- properties of the restatement itself --------------------------------------------------------------------------------------------
def _peak_hz(y, sr):
    spec = np.abs(np.fft.rfft(y * np.hanning(y.size)))
    return np.argmax(spec) * sr / y.size, sr / y.size


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_a_stretched_sine_keeps_its_frequency(rate):
    sr, n = 22050, 22050
    y = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)).astype(np.float32)
    out = A.time_stretch(y, rate)
    assert out.size == A.stretch_length(n, rate) == int(round(n / rate))
    peak, bin_hz = _peak_hz(out[2048:-2048], sr)
    assert abs(peak - 1000.0) <= bin_hz, (peak, bin_hz)


def test_rate_one_reproduces_the_interior_and_silence_stays_silent():
    rng = np.random.default_rng(8)
    y = (0.3 * rng.standard_normal(5000) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(5000) / 22050)).astype(np.float32)
    for pad in ("reflect", "zero"):
        out = A.time_stretch(y, 1.0, pad)
        assert out.size == y.size
        err = np.abs(out - y)[2048:-2048].max()
        print(f"rate 1.0, pad {pad}: interior error {err:.2e}")
        assert err <= 1e-9
    # the transform pair alone is exact everywhere (the window's squares never vanish inside the clip)
    assert np.abs(A.istft(A.stft(y), y.size) - y).max() <= 1e-12
    assert np.abs(A.istft(A.stft(y, dtype=np.float32), y.size, np.float32) - y).max() <= 1e-5
    for dtype in (np.float64, np.float32):
        z = A.time_stretch(np.zeros(3000, np.float32), 0.8, dtype=dtype)
        assert z.size == 3750 and not z.any() and np.isfinite(z).all()
    assert not A.pitch_shift(np.zeros(3000, np.float32), 2).any()


def test_the_float32_switch_stays_near_float64():
    """the float32 dataflow is only a yardstick for the GPU tests' bounds: it must itself be a float32-sized step from the float64 one"""
    rng = np.random.default_rng(9)
    y = (0.3 * rng.standard_normal(2560) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(2560) / 22050)).astype(np.float32)
    D64, D32 = A.stft(y), A.stft(y, dtype=np.float32)
    rel = (np.abs(D32 - D64).max(axis=1) / np.abs(D64).max(axis=1)).max()
    assert 0 < rel < 1e-5, rel
    S64, S32 = A.phase_vocoder(D32, 0.8), A.phase_vocoder(D32, 0.8, np.float32)
    y64, y32 = A.istft(S64, 3200), A.istft(S32, 3200, np.float32)
    assert 0 < np.abs(y32 - y64).max() < 1e-4
    z64, z32 = A.normal(3, 4, 4096), A.normal(3, 4, 4096, np.float32)
    assert 0 < np.abs(z32 - z64).max() < 1e-5
