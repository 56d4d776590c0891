"""The 400-point MFCC front end of the speaker models (include/dsp_amd.h dsp_mfcc_speaker_config) restated in float64
from the published formulas of librosa.feature.mfcc(y, sr, n_mfcc, n_fft = 400, hop_length) with pad_mode = "constant":

    frames    DSP_FRAMING_CENTER: the clip padded by n_fft / 2 zeros at both ends, T = 1 + n // hop frames of n_fft samples from t hop;
              DSP_FRAMING_COMPLETE: the frames that lie inside the clip, T = 1 + (n - n_fft) // hop
    spectrum  periodic Hann, np.fft.rfft(n = 400), |X|^2 (201 bins)
    mel       triangles between n_mels + 2 points evenly spaced on the mel scale: weight = max(0, min(rise, fall)); HTK scale
              2595 log10(1 + f / 700) with peak 1 (NONE) or unit area (SLANEY: x 2 / (f[m + 2] - f[m])), or Slaney's scale (200 / 3 Hz
              per mel below 1 kHz, log(6.4) / 27 per mel above) with unit area (LIBROSA)
    dB        PER_FRAME_MAX: 10 log10(max(E, amin) / max(max E, amin)) clipped at -top_db;  GLOBAL_REF1: 10 log10(max(E, amin)), clipped at
              the CLIP's maximum - top_db (power_to_db(ref = 1))
    DCT       scipy.fft.dct(type = 2, norm = "ortho"), the first n_mfcc coefficients

and sliding_cmvn as 2fa/audio/speaker/gmm_utils.py:14-25 states it.  numpy and scipy only; nothing of the library."""
import numpy as np
import scipy.fft

N_FFT = 400
MELNORM_NONE, MELNORM_SLANEY, MELNORM_LIBROSA = 0, 1, 2
LOG_PER_FRAME_MAX, LOG_GLOBAL_REF1 = 0, 1
FRAMING_COMPLETE, FRAMING_CENTER = 0, 2
WINDOW_HANN, WINDOW_HAMMING, WINDOW_RECT = 0, 1, 2


def window(kind, n):
    ph = 2.0 * np.pi * np.arange(n) / n           # periodic (fftbins = True)
    if kind == WINDOW_HANN:
        return 0.5 - 0.5 * np.cos(ph)
    if kind == WINDOW_HAMMING:
        return 0.54 - 0.46 * np.cos(ph)
    return np.ones(n)


def _mel_scale(slaney):
    if not slaney:
        return (lambda f: 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)), (lambda m: 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0))
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def to_mel(f):
        f = np.asarray(f, np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)

    def to_hz(m):
        m = np.asarray(m, np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    return to_mel, to_hz


def mel_bank(sample_rate, n_fft, n_mels, fmin, fmax, mel_norm):
    """float64 [n_mels][n_fft // 2 + 1]"""
    to_mel, to_hz = _mel_scale(mel_norm == MELNORM_LIBROSA)
    edges = to_hz(np.linspace(float(to_mel(fmin)), float(to_mel(fmax)), n_mels + 2))
    freqs = np.linspace(0.0, 0.5 * sample_rate, n_fft // 2 + 1)
    ramps = edges[:, None] - freqs[None, :]
    fdiff = np.diff(edges)
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    if mel_norm != MELNORM_NONE:
        w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w


def dct_basis(n_mfcc, n_mels):
    """float64 [n_mfcc][n_mels]: the rows scipy.fft.dct(type = 2, norm = "ortho") applies"""
    return scipy.fft.dct(np.eye(n_mels), type=2, norm="ortho", axis=1).T[:n_mfcc]


def frames_for(cfg, n, max_frames=None):
    if cfg.framing == FRAMING_CENTER:
        t = 1 + n // cfg.hop_length if n >= 1 else 0
    else:
        t = 1 + (n - cfg.frame_length) // cfg.hop_length if n >= cfg.frame_length else 0
    return t if max_frames is None else min(t, max_frames)


def cut(y, cfg, max_frames=None):
    """the clip's frames, float64 [T][n_fft]"""
    y = np.asarray(y, np.float64)
    t = frames_for(cfg, y.size, max_frames)
    if cfg.framing == FRAMING_CENTER:
        y = np.concatenate([np.zeros(cfg.n_fft // 2), y, np.zeros(cfg.n_fft // 2)])
    return np.stack([y[i * cfg.hop_length: i * cfg.hop_length + cfg.n_fft] for i in range(t)]) if t else np.zeros((0, cfg.n_fft))


def mel_energies(frames, cfg, dtype=np.float64):
    """dtype = np.float32: a float32 model of the chain (tables rounded once, scipy's float32 transforms, float32 products and sums)"""
    xw = (np.asarray(frames).astype(dtype) * window(cfg.window, cfg.n_fft).astype(dtype)).astype(dtype)
    if dtype == np.float64:
        spec = np.abs(np.fft.rfft(xw, n=cfg.n_fft, axis=-1)) ** 2
    else:
        z = scipy.fft.rfft(xw, n=cfg.n_fft, axis=-1)
        spec = (z.real * z.real + z.imag * z.imag).astype(dtype)
    return (spec @ mel_bank(cfg.sample_rate, cfg.n_fft, cfg.n_mels, cfg.fmin, cfg.fmax, cfg.mel_norm).T.astype(dtype)).astype(dtype)


def _rows(e, cfg, one_clip):
    """mel energies [T][n_mels] -> MFCC rows [T][n_mfcc] in e's dtype; one_clip: the GLOBAL_REF1 floor over all rows, else per row"""
    dtype = e.dtype.type
    amin, top_db, ten = dtype(cfg.amin), dtype(cfg.top_db), dtype(10.0)
    if e.shape[0] == 0:
        return np.zeros((0, cfg.n_mfcc), dtype)
    if cfg.log_mode == LOG_PER_FRAME_MAX:
        ref = np.maximum(e.max(axis=1, keepdims=True), amin)
        db = np.maximum(ten * np.log10(np.maximum(e, amin) / ref), -top_db)
    else:
        db = ten * np.log10(np.maximum(e, amin))
        top = db.max() if one_clip else db.max(axis=1, keepdims=True)
        db = np.maximum(db, top - top_db)
    return scipy.fft.dct(db.astype(dtype), type=2, norm="ortho", axis=1)[:, :cfg.n_mfcc].astype(dtype)


def frames_features(frames, cfg, dtype=np.float64):
    """independent frames [n][400]: every frame its own clip"""
    return _rows(mel_energies(frames, cfg, dtype), cfg, False)


def features(y, cfg, max_frames=None, dtype=np.float64):
    """one clip -> [T][n_mfcc] in dtype"""
    return _rows(mel_energies(cut(y, cfg, max_frames), cfg, dtype), cfg, True)


def sliding_cmvn(feats, win_size=300, eps=1e-8):
    """gmm_utils.py:14-25: row t by the mean and the population standard deviation of rows [t - win // 2, t + win // 2) of the clip"""
    feats = np.asarray(feats, np.float64)
    n = feats.shape[0]
    out = np.empty_like(feats)
    for t in range(n):
        seg = feats[max(0, t - win_size // 2): min(n, t + win_size // 2)]
        out[t] = (feats[t] - seg.mean(axis=0)) / (seg.std(axis=0) + eps)
    return out
