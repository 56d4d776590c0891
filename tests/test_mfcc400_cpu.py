"""CPU: the host side of the 400-point MFCC front end (dsp_mfcc_speaker_config, DSP_FRAMING_CENTER, the n_fft 400 plans' tables and the
lane model of mfcc400_kernel.hip's FFT) -- configuration and refusals, frame counts, every table against its float64 formula, the FFT
dataflow against np.fft.rfft.  No GPU call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from dsp_amd import mfcc as M

from tests import mfcc400_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _valid(cfg):
    """what dsp_mfcc_plan_create's validation says, through a host-only entry that runs it: (ok, message)"""
    off, n = dl.c_offsets([0, 400])
    fo = (C.c_long * 2)()
    rc = dl.load().dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, 10, fo)
    return rc >= 0, dl.last_error()


def test_speaker_config_is_gmm_utils_librosa_call():
    c = dsp_amd.speaker_config()
    assert (c.sample_rate, c.n_fft, c.frame_length, c.hop_length, c.n_mels, c.n_mfcc) == (16000, 400, 400, 160, 128, 13)
    assert (c.window, c.mel_norm, c.log_mode, c.spectrum, c.framing) == (dl.WINDOW_HANN, dl.MELNORM_LIBROSA, dl.LOG_GLOBAL_REF1,
                                                                         dl.SPECTRUM_POWER, dl.FRAMING_CENTER)
    assert dl.FRAMING_CENTER == 2
    assert (c.fmin, c.fmax, c.top_db, c.win_length, c.prefilter) == (0.0, 8000.0, 80.0, 0, dl.PREFILTER_NONE)
    assert c.amin == np.float32(1e-10)
    assert dl.load().dsp_abi_sizeof(0) == C.sizeof(dl.MfccConfig) == 17 * 4
    with pytest.raises(AttributeError):
        dsp_amd.speaker_config(no_such_field=1)


@pytest.mark.parametrize("over", [{}, dict(n_mels=40, n_mfcc=20), dict(n_mels=1, n_mfcc=1), dict(n_mels=128, n_mfcc=32),
                                  dict(mel_norm=dl.MELNORM_NONE), dict(mel_norm=dl.MELNORM_SLANEY), dict(log_mode=dl.LOG_PER_FRAME_MAX),
                                  dict(framing=dl.FRAMING_COMPLETE), dict(sample_rate=8000, fmax=4000.0), dict(sample_rate=44100, fmax=8000.0),
                                  dict(window=dl.WINDOW_HAMMING), dict(hop_length=200)])
def test_accepted_400_point_configurations(over):
    ok, why = _valid(dsp_amd.speaker_config(**over))
    assert ok, why


@pytest.mark.parametrize("over,field", [(dict(frame_length=398), "frame_length"), (dict(win_length=200), "win_length"), (dict(n_mels=129), "n_mels"),
                                        (dict(n_mfcc=33), "n_mfcc"), (dict(n_mels=20, n_mfcc=21), "n_mfcc"),
                                        (dict(spectrum=dl.SPECTRUM_MAGNITUDE), "spectrum"), (dict(log_mode=dl.LOG_LOG10_FLOOR), "log_mode"),
                                        (dict(framing=dl.FRAMING_STREAM), "framing"), (dict(prefilter=dl.PREFILTER_BUTTER_1000_3000), "prefilter"),
                                        (dict(mel_norm=dl.MELNORM_AUBIO_SLANEY, n_mels=40), "mel_norm"), (dict(sample_rate=8000), "fmax")])
def test_refused_400_point_configurations_name_the_field(over, field):
    cfg = dsp_amd.speaker_config(**over)
    ok, why = _valid(cfg)
    assert not ok and field in why, why
    h = C.c_void_p()
    assert dl.load().dsp_mfcc_plan_create(C.byref(cfg), 0, C.byref(h)) == -1 and field in dl.last_error()      # before any device call


def test_center_framing_belongs_to_n_fft_400_and_other_sizes_stay_refused():
    ok, why = _valid(dsp_amd.default_config(framing=dl.FRAMING_CENTER))                  # n_fft 512
    assert not ok and "framing" in why and "400" in why
    for over in (dict(n_fft=256, frame_length=256), dict(n_fft=300, frame_length=300)):
        ok, why = _valid(dsp_amd.default_config(**over))
        assert not ok and "n_fft" in why and "400" in why                               # the message lists 400 with the others
    ok, why = _valid(dsp_amd.default_config(frame_length=401))
    assert not ok and "even" in why
    ok, why = _valid(dsp_amd.default_config(framing=7))
    assert not ok and "framing" in why


def test_frame_counts():
    c = dsp_amd.speaker_config()
    assert [dsp_amd.frames_for(c, n, 500) for n in (0, 1, 159, 160, 161, 399, 400, 6129)] == [0, 1, 1, 2, 2, 3, 3, 39]
    assert dsp_amd.frames_for(c, -5, 500) == 0
    assert [dsp_amd.frames_for(c, 6129, mx) for mx in (0, -1, 1, 2, 38, 39, 40)] == [0, 0, 1, 2, 38, 39, 39]
    assert dsp_amd.frames_for(c, 2**31 - 1, 2**31 - 1) == 1 + (2**31 - 1) // 160
    k = dsp_amd.speaker_config(framing=dl.FRAMING_COMPLETE)
    assert [dsp_amd.frames_for(k, n, 500) for n in (399, 400, 559, 560)] == [0, 1, 1, 2]
    for cfg in (c, k):
        for n in (0, 1, 160, 399, 400, 6129):
            assert R.frames_for(cfg, n) == dsp_amd.frames_for(cfg, n, 2**31 - 1)


def test_ragged_frame_offsets_follow_center_framing():
    c = dsp_amd.speaker_config()
    lens = [0, 1, 159, 160, 0, 400, 6129, 1]
    offsets = np.concatenate([[3], 3 + np.cumsum(lens)])
    assert M.ragged_frame_offsets(c, offsets, 500).tolist() == [0, 0, 1, 2, 4, 4, 7, 46, 47]
    assert M.ragged_frame_offsets(c, offsets, 2).tolist() == [0, 0, 1, 2, 4, 4, 6, 8, 9]
    k = dsp_amd.speaker_config(framing=dl.FRAMING_COMPLETE)
    assert M.ragged_frame_offsets(k, offsets, 500).tolist() == [0, 0, 0, 0, 0, 0, 1, 37, 37]


CONFIGS = {"speaker": {}, "htk128": dict(mel_norm=dl.MELNORM_NONE), "htk128_area": dict(mel_norm=dl.MELNORM_SLANEY),
           "htk40": dict(mel_norm=dl.MELNORM_NONE, n_mels=40), "mel40": dict(n_mels=40), "sr8000": dict(sample_rate=8000, fmax=4000.0)}
ULP4 = 4 * 2.0 ** -24


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_tables_are_the_float64_formulas_rounded_once(name):
    """|table - float32(formula)| <= 4 * 2^-24 * the table's largest magnitude; the DCT's generator works in float32 like the reference's
    exporter (its argument pi (m + 0.5) k / n_mels is rounded three times), so it gets SURVEY 8a's figure for that table, 5.9e-7.  That
    figure is for 13 rows, which every case here has: the argument's rounding grows with the row index (20 rows of 40: 7.7e-7)."""
    cfg = dsp_amd.speaker_config(**CONFIGS[name])
    win, mel, dct = dsp_amd.tables(cfg)
    assert win.shape == (400,) and mel.shape == (cfg.n_mels, 201) and dct.shape == (cfg.n_mfcc, cfg.n_mels)
    want_w = R.window(cfg.window, 400).astype(np.float32)
    assert np.abs(win.astype(np.float64) - want_w).max() <= ULP4 * np.abs(want_w).max()
    want_m = R.mel_bank(cfg.sample_rate, 400, cfg.n_mels, cfg.fmin, cfg.fmax, cfg.mel_norm).astype(np.float32)
    assert np.abs(mel.astype(np.float64) - want_m).max() <= ULP4 * np.abs(want_m).max()
    want_d = R.dct_basis(cfg.n_mfcc, cfg.n_mels).astype(np.float32)
    assert np.abs(dct.astype(np.float64) - want_d).max() <= 5.9e-7
    empty = np.flatnonzero(~mel.any(axis=1)).tolist()
    assert empty == np.flatnonzero(~want_m.any(axis=1)).tolist()
    assert len(empty) == (4 if name.startswith("htk128") else 0)
    if name == "speaker":
        nnz = (mel != 0).sum(axis=1)
        assert nnz.max() <= 9 and nnz.sum() == 394
    if name in ("mel40", "htk40"):
        assert (mel != 0).sum(axis=1).max() <= 28


def test_the_reference_bank_agrees_with_the_oracles_and_the_pinned_slaney_formula():
    from oracle import oracle as O
    import pin_svm_libsvm as P
    want = R.mel_bank(16000, 400, 128, 0.0, 8000.0, R.MELNORM_LIBROSA)
    assert np.abs(O.mel_filterbank(16000, 400, 128, 0.0, 8000.0, 2).astype(np.float64) - want).max() <= 4 * 2.0 ** -24 * want.max()
    assert np.abs(np.asarray(P.slaney_mel(16000, 400, 128), np.float64) - want).max() <= 4 * 2.0 ** -24 * want.max()


def test_kernel_tables_hold_the_bank_as_runs_and_the_empty_filters():
    import emulate_400_fft as E
    for name in ("speaker", "htk128", "mel40_20"):
        cfg = dsp_amd.speaker_config(**CONFIGS.get(name, dict(n_mels=40, n_mfcc=20)))
        T = E.load_tables(cfg)
        _, mel, dct = dsp_amd.tables(cfg)
        assert (T["n_mels"], T["n_mfcc"]) == (cfg.n_mels, cfg.n_mfcc) and T["n_weights"] <= 416
        back = np.zeros_like(mel)
        for m in range(cfg.n_mels):
            lo, ln, off = T["mel_lo"][m], T["mel_len"][m], T["mel_off"][m]
            assert 0 <= lo and lo + ln <= 201 and off + ln <= T["n_weights"]
            back[m, lo:lo + ln] = T["mel_w"][off:off + ln]
        assert np.array_equal(back, mel)
        assert (T["mel_len"][:cfg.n_mels] == 0).sum() == (4 if name == "htk128" else 0)
        assert np.array_equal(T["dct"][:cfg.n_mfcc, :cfg.n_mels], dct)
        half = (cfg.n_mels + 1) // 2
        for lane in range(64):
            c, h = lane >> 1, lane & 1
            row = np.zeros(half, np.float32)
            if c < cfg.n_mfcc:
                seg = dct[c, h * half:min((h + 1) * half, cfg.n_mels)]
                row[:seg.size] = seg
            assert np.array_equal(T["dct_t"][:half, lane], row)
    L = dl.load()
    t = E.Tables400()
    assert L.dsp_mfcc400_tables(C.byref(dsp_amd.default_config()), C.byref(t), C.sizeof(t)) == -1 and "400" in dl.last_error()
    assert L.dsp_mfcc400_tables(C.byref(dsp_amd.speaker_config()), C.byref(t), 12) == -1
    assert L.dsp_mfcc_lane_tables(C.byref(dsp_amd.speaker_config()), None, 0) == -1 and "400" in dl.last_error()


def _fft_frames():
    rng = np.random.default_rng(400)
    n = np.arange(400)
    return {"noise0": rng.uniform(-1, 1, 400), "noise1": rng.uniform(-1, 1, 400), "noise_small": 1e-4 * rng.uniform(-1, 1, 400),
            "impulse0": (n == 0).astype(float), "impulse399": (n == 399).astype(float), "dc": np.ones(400),
            "nyquist": np.where(n % 2 == 0, 1.0, -1.0), "bin37": np.cos(2 * np.pi * 37 * n / 400 + 0.3)}


@pytest.mark.parametrize("kind", sorted(_fft_frames()))
def test_fft_lane_model_with_the_librarys_tables_is_the_real_fft(kind):
    """float64 arithmetic, the library's float32 window and twiddles: every bin within 4 * 2^-23 * sum |x w| of np.fft.rfft (a term passes
    through at most four rounded factors of relative error 2^-24 each)."""
    import emulate_400_fft as E
    cfg = dsp_amd.speaker_config()
    T = E.load_tables(cfg)
    x = _fft_frames()[kind]
    xw = x * R.window(cfg.window, 400)
    got = E.wave_rfft400(x, T)
    assert got.shape == (201,)
    assert np.abs(got - np.fft.rfft(xw)).max() <= 4 * 2.0 ** -23 * np.abs(xw).sum()


def test_new_symbols_are_exported():
    lib = os.path.join(ROOT, "dsp_amd", "libdsp_amd.so")
    dl.load()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"dsp_mfcc_speaker_config", "dsp_mfcc400_tables"} <= names
    assert {"dsp_mfcc_speaker_config", "dsp_mfcc400_tables"} <= set(dl.SYMBOLS)


def test_speaker_front_end_is_exported_and_needs_a_device():
    assert "SpeakerFrontEnd" in dsp_amd.__all__ and "speaker_config" in dsp_amd.__all__
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(dsp_amd.DspError, match="no HIP device"):
            dsp_amd.SpeakerFrontEnd()
