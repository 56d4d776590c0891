"""CPU: the host side of DSP_FRAMING_CENTER at n_fft 2048 (dsp_mfcc_librosa_config: librosa.feature.mfcc with librosa's default n_fft, hop
and centring) -- the configuration, what validation accepts and refuses, frame counts -- and the inputs of the GPU test held to the gate
by a float32 numpy evaluation of the chain, without the library.  No GPU call."""
import ctypes as C

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from dsp_amd import mfcc as M

from tests import mfcc2048_center_cases as K
from tests import mfcc400_ref as R
from tests.conftest import gate


def _valid(cfg):
    """what dsp_mfcc_plan_create's validation says, through a host-only entry that runs it: (ok, message)"""
    off, n = dl.c_offsets([0, 400])
    fo = (C.c_long * 2)()
    rc = dl.load().dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, 10, fo)
    return rc >= 0, dl.last_error()


def test_librosa_config_is_librosas_default_mfcc_call():
    c = dsp_amd.librosa_config()
    assert (c.sample_rate, c.n_fft, c.frame_length, c.hop_length, c.n_mels, c.n_mfcc) == (22050, 2048, 2048, 512, 128, 13)
    assert (c.window, c.mel_norm, c.log_mode, c.spectrum, c.framing) == (dl.WINDOW_HANN, dl.MELNORM_LIBROSA, dl.LOG_GLOBAL_REF1,
                                                                         dl.SPECTRUM_POWER, dl.FRAMING_CENTER)
    assert (c.fmin, c.fmax, c.top_db, c.win_length, c.prefilter) == (0.0, 11025.0, 80.0, 0, dl.PREFILTER_NONE)
    assert c.amin == np.float32(1e-10)
    k = dsp_amd.librosa_config(16000, 20)                                # cepstrum/train.py:38-40
    assert (k.sample_rate, k.n_mfcc, k.fmax, k.n_fft, k.hop_length) == (16000, 20, 8000.0, 2048, 512)
    assert dl.load().dsp_abi_sizeof(0) == C.sizeof(dl.MfccConfig) == 17 * 4      # the struct is what it was
    with pytest.raises(AttributeError):
        dsp_amd.librosa_config(no_such_field=1)


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_the_cases_namespaces_are_librosa_config_with_overrides(name):
    sr, n_mfcc, over = K.CONFIGS[name]
    got, want = dsp_amd.librosa_config(sr, n_mfcc, **over), K.cfg_of(name)
    for field, _ in dl.MfccConfig._fields_:
        assert getattr(got, field) == (np.float32(getattr(want, field)) if field in ("fmin", "fmax", "amin", "top_db") else getattr(want, field)), field
    ok, why = _valid(got)
    assert ok, why


@pytest.mark.parametrize("over", [{}, dict(n_mels=40, n_mfcc=20), dict(n_mels=1, n_mfcc=1), dict(n_mels=128, n_mfcc=32), dict(mel_norm=dl.MELNORM_NONE),
                                  dict(mel_norm=dl.MELNORM_SLANEY), dict(log_mode=dl.LOG_PER_FRAME_MAX), dict(window=dl.WINDOW_HAMMING),
                                  dict(hop_length=1024), dict(hop_length=2), dict(sample_rate=44100, fmax=8000.0)])
def test_accepted_centred_2048_point_configurations(over):
    ok, why = _valid(dsp_amd.librosa_config(**over))
    assert ok, why


@pytest.mark.parametrize("over,field", [(dict(frame_length=2046), "frame_length"), (dict(win_length=1024), "win_length"), (dict(n_mels=129), "n_mels"),
                                        (dict(n_mfcc=33), "n_mfcc"), (dict(spectrum=dl.SPECTRUM_MAGNITUDE), "spectrum"),
                                        (dict(log_mode=dl.LOG_LOG10_FLOOR), "log_mode"), (dict(mel_norm=dl.MELNORM_AUBIO_SLANEY, n_mels=40), "mel_norm"),
                                        (dict(prefilter=dl.PREFILTER_BUTTER_1000_3000), "prefilter"), (dict(hop_length=511), "hop_length")])
def test_refused_centred_2048_point_configurations_name_the_field(over, field):
    cfg = dsp_amd.librosa_config(**over)
    ok, why = _valid(cfg)
    assert not ok and field in why, why
    h = C.c_void_p()
    assert dl.load().dsp_mfcc_plan_create(C.byref(cfg), 0, C.byref(h)) == -1 and field in dl.last_error()      # before any device call
    assert not h.value


def test_center_framing_stays_refused_at_512_and_1024():
    for over in (dict(n_fft=512, frame_length=512), dict(n_fft=1024, frame_length=1024), dict(n_fft=512, frame_length=400, hop_length=160)):
        ok, why = _valid(dsp_amd.librosa_config(**over))
        assert not ok and "framing" in why and "400 and 2048" in why, why


def test_frame_counts_at_hop_512():
    c = dsp_amd.librosa_config()
    lens = (0, 1, 511, 512, 513, 1023, 1024, 2047, 2048, 5000)
    assert [dsp_amd.frames_for(c, n, 2**31 - 1) for n in lens] == [0, 1, 1, 2, 2, 2, 3, 4, 5, 10]
    assert [dsp_amd.frames_for(c, 5000, mx) for mx in (0, -1, 1, 9, 10, 11)] == [0, 0, 1, 9, 10, 10]
    assert [R.frames_for(K.cfg_of("keyword_22k_13"), n) for n in lens] == [0, 1, 1, 2, 2, 2, 3, 4, 5, 10]
    assert [dsp_amd.frames_for(c, n, 500) for n in K.LENGTHS] == list(K.FRAMES)
    offsets = np.concatenate([[3], 3 + np.cumsum(lens)])
    assert M.ragged_frame_offsets(c, offsets, 2**31 - 1).tolist() == np.concatenate([[0], np.cumsum([0, 1, 1, 2, 2, 2, 3, 4, 5, 10])]).tolist()
    assert M.ragged_frame_offsets(c, offsets, 3).tolist() == np.concatenate([[0], np.cumsum([0, 1, 1, 2, 2, 2, 3, 3, 3, 3])]).tolist()


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_the_gpu_tests_inputs_are_inside_the_gate_without_the_library(name):
    """a float32 numpy evaluation of the chain against the float64 one, on every clip of the GPU test: an input that misses here is the
    wrong input (the gate stays)"""
    cfg = K.cfg_of(name)
    for y, ref in zip(K.clips(name), K.oracle(name)):
        assert ref.shape == (1 + y.size // K.HOP, cfg.n_mfcc)
        gate(R.features(y, cfg, dtype=np.float32), ref, f"numpy32_center2048_{name}_{y.size}")
    y = K.half_silent_clip(name)
    ref = R.features(y, cfg)
    gate(R.features(y, cfg, dtype=np.float32), ref, f"numpy32_center2048_{name}_half_silent")
    if cfg.log_mode == R.LOG_GLOBAL_REF1:       # frames 8, 9 lie wholly in the silence: every filter on the clip floor, one value -> c0 alone
        assert np.abs(ref[8:, 1:]).max() < 1e-9 and ref[8, 0] == ref[9, 0] < ref[0, 0]
