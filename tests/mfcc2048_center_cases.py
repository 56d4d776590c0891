"""The configurations and inputs of the centred 2048-point MFCC tests (tests/test_mfcc2048_center_cpu.py holds a float32 numpy evaluation
of the chain to the gate on them, tests/test_gpu_mfcc2048_center.py the kernel).  Nothing of the library is imported: the configurations
are plain namespaces with dsp_mfcc_config's fields, what dsp_mfcc_librosa_config(sample_rate, n_mfcc) is specified to fill in."""
from types import SimpleNamespace

import numpy as np

from tests import mfcc400_ref as R

HOP = 512
LENGTHS = (1, 511, 1023, 1024, 1025, 2048, 3000, 5000)       # a clip shorter than half a frame .. several frames; odd lengths: offsets of both parities
FRAMES = (1, 1, 2, 3, 3, 5, 6, 10)                          # 1 + n // 512
GUARD = 2051                                                # samples in front of clip 0 and behind the last clip (odd: the batch starts at an odd sample)


def librosa_cfg(sample_rate, n_mfcc, **over):
    c = SimpleNamespace(sample_rate=sample_rate, n_fft=2048, frame_length=2048, hop_length=HOP, n_mels=128, n_mfcc=n_mfcc, window=R.WINDOW_HANN,
                        mel_norm=R.MELNORM_LIBROSA, log_mode=R.LOG_GLOBAL_REF1, prefilter=0, win_length=0, fmin=0.0, fmax=0.5 * sample_rate, amin=1e-10,
                        top_db=80.0, spectrum=0, framing=R.FRAMING_CENTER)
    c.__dict__.update(over)
    return c


# name -> (sample_rate, n_mfcc, overrides of librosa_config)
CONFIGS = {
    "keyword_22k_13": (22050, 13, {}),                                       # keyword_classifier.py:41-44
    "cepstrum_16k_20": (16000, 20, {}),                                      # cepstrum/train.py:38-40
    "keyword_22k_13_frame_max": (22050, 13, {"log_mode": R.LOG_PER_FRAME_MAX}),
    "cepstrum_16k_20_frame_max": (16000, 20, {"log_mode": R.LOG_PER_FRAME_MAX}),
    "slaney40_22k_13": (22050, 13, {"n_mels": 40, "mel_norm": R.MELNORM_SLANEY}),
}


def cfg_of(name):
    sr, n_mfcc, over = CONFIGS[name]
    return librosa_cfg(sr, n_mfcc, **over)


def clip(name, n, sample_rate):
    """seeded chirp + noise: a sweep from 100 Hz to 0.45 sample_rate over the clip at half scale, uniform noise at 1e-2 of full scale (every
    filter holds signal well above the transform's own float32 noise)"""
    seed = 97 * list(CONFIGS).index(name) + n
    t = np.arange(n, dtype=np.float64) / sample_rate
    dur = max(n, 2) / sample_rate
    f0, f1 = 100.0, 0.45 * sample_rate
    phase = 2.0 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / dur)
    return (0.5 * np.cos(phase) + 1e-2 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)).astype(np.float32)


def clips(name):
    sr = CONFIGS[name][0]
    return [clip(name, n, sr) for n in LENGTHS]


def half_silent_clip(name, n=5000):
    """the second half exactly silent: more than top_db below the clip's maximum"""
    y = clip(name, n, CONFIGS[name][0]).copy()
    y[n // 2:] = 0.0
    return y


_ORACLE = {}


def oracle(name):
    """float64 rows of every clip of clips(name), made once"""
    if name not in _ORACLE:
        _ORACLE[name] = [R.features(y, cfg_of(name)) for y in clips(name)]
    return _ORACLE[name]
