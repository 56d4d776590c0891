"""The augmenter's definition (include/dsp_amd.h dsp_augment_*) restated in numpy from the formulas there: the centred
STFT (n_fft 2048, hop 512, periodic Hann), the phase vocoder with its float64 accumulator, the inverse STFT with the overlap-add in
ascending frame order, time stretch, pitch shift (through tests/resample_ref.py) and the noise from the library's counter-based draws.

float64 by default.  dtype=np.float32 runs the same dataflow with every array in float32 (window, transform, magnitudes, angles,
sin / cos, overlap-add) and the accumulator still in float64, as the kernels do: it is used only to measure error floors."""
import math

import numpy as np

from tests import resample_ref as R

N_FFT, HOP, BINS, PAD = 2048, 512, 1025, 1024
GOLDEN = 0x9E3779B97F4A7C15
POLICY_STREAM = 0xA000000000000000
MASK = (1 << 64) - 1


def window(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


def stft_frames(n):
    return 1 + n // HOP


def stretch_frames(frames, rate):
    return int(math.ceil(frames / rate))


def stretch_length(n, rate):
    return max(1, int(round(n / rate)))          # Python 3's round: ties to even


def pitch_ratio(n_steps, bins_per_octave=12, max_term=256):
    """brute force over every fraction: the nearest to 2^(-n_steps / bins_per_octave), ties to the smaller denominator"""
    f = 2.0 ** (-n_steps / bins_per_octave)
    best = None
    for down in range(1, max_term + 1):
        for up in range(1, max_term + 1):
            key = (abs(up / down - f), down, up)
            if best is None or key < best:
                best = key
    return best[2], best[1]


# ---- transforms: numpy's in float64; a radix-2 Stockham autosort in float32 (numpy < 2 would compute a float32 input in float64) ----------
def _fft32(x):
    """forward DFT over the last axis (a power of two) of a complex64 array, every operation in float32"""
    x = np.ascontiguousarray(x, np.complex64)
    n = x.shape[-1]
    lead = x.shape[:-1]
    ns = 1
    while ns < n:
        half = n // 2
        j = np.arange(half)
        w = np.exp(-2j * np.pi * (j % ns) / (2 * ns)).astype(np.complex64)
        a, b = x[..., :half], (x[..., half:] * w).astype(np.complex64)
        y = np.empty(lead + (n,), np.complex64)
        dst = (j // ns) * 2 * ns + (j % ns)
        y[..., dst] = a + b
        y[..., dst + ns] = a - b
        x = y
        ns *= 2
    return x


def _rfft(frames, dtype):
    if dtype == np.float64:
        return np.fft.rfft(frames.astype(np.float64), axis=-1)
    return _fft32(frames.astype(np.float32))[..., :BINS]


def _irfft(S, dtype):
    S = np.array(S, np.complex128 if dtype == np.float64 else np.complex64)
    S[..., 0] = S[..., 0].real
    S[..., BINS - 1] = S[..., BINS - 1].real
    if dtype == np.float64:
        return np.fft.irfft(S, n=N_FFT, axis=-1)
    full = np.concatenate([S, np.conj(S[..., BINS - 2:0:-1])], axis=-1)
    return (np.conj(_fft32(np.conj(full))).real * np.float32(1.0 / N_FFT)).astype(np.float32)


def stft(y, pad="reflect", dtype=np.float64):
    """y [n] -> D [T][1025] complex"""
    y = np.asarray(y).astype(dtype)
    n = y.size
    assert n >= (PAD + 1 if pad == "reflect" else 1)
    yp = np.pad(y, PAD, mode="reflect") if pad == "reflect" else np.pad(y, PAD)
    idx = HOP * np.arange(stft_frames(n))[:, None] + np.arange(N_FFT)[None, :]
    return _rfft((yp[idx] * window(dtype)).astype(dtype), dtype)


def phase_vocoder(D, rate, dtype=np.float64):
    """D [T][1025] -> S [ceil(T / rate)][1025]"""
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    D = np.asarray(D).astype(ctype)
    T = D.shape[0]
    T_out = stretch_frames(T, rate)
    Dp = np.concatenate([D, np.zeros((2, BINS), ctype)])
    mag = np.abs(Dp).astype(dtype)
    ang = np.where((Dp.real == 0) & (Dp.imag == 0), 0, np.angle(Dp)).astype(dtype)
    phi = np.pi * 512 * np.arange(BINS) / 1024
    two_pi = 2.0 * np.pi
    acc = ang[0].astype(np.float64)
    S = np.zeros((T_out, BINS), ctype)
    for t in range(T_out):
        s = t * rate
        i = int(math.floor(s))
        a = dtype(s - i)
        m = ((dtype(1) - a) * mag[i] + a * mag[i + 1]).astype(dtype)
        ph = (acc - two_pi * np.rint(acc / two_pi)).astype(dtype)
        S[t] = (m * np.cos(ph)).astype(dtype) + 1j * (m * np.sin(ph)).astype(dtype)
        d = ang[i + 1].astype(np.float64) - ang[i].astype(np.float64) - phi
        d = d - two_pi * np.rint(d / two_pi)
        acc = acc + phi + d
    return S


def istft(S, length, dtype=np.float64):
    """S [T][1025] -> y [length]"""
    S = np.asarray(S)
    T = S.shape[0]
    if T == 0:
        return np.zeros(length, dtype)
    w = window(dtype)
    frames = (_irfft(S, dtype) * w).astype(dtype)
    w2 = (w * w).astype(dtype)
    y = np.zeros(HOP * (T - 1) + N_FFT, dtype)
    wss = np.zeros_like(y)
    for t in range(T):                                   # ascending t
        y[HOP * t:HOP * t + N_FFT] += frames[t]
        wss[HOP * t:HOP * t + N_FFT] += w2
    nz = wss > np.finfo(np.float32).tiny
    y[nz] = y[nz] / wss[nz]
    y = y[PAD:]
    out = np.zeros(length, dtype)
    out[:min(length, y.size)] = y[:length]
    return out


def time_stretch(y, rate, pad="reflect", dtype=np.float64):
    return istft(phase_vocoder(stft(y, pad, dtype), rate, dtype), stretch_length(np.asarray(y).size, rate), dtype)


def fit(y, n, dtype=np.float64):
    out = np.zeros(n, dtype)
    out[:min(n, y.size)] = y[:n]
    return out


def pitch_shift(y, n_steps, max_term=256, pad="reflect", dtype=np.float64):
    up, down = pitch_ratio(n_steps, 12, max_term)
    ys = time_stretch(y, up / down, pad, dtype)
    if up != down:
        ys = R.resample(ys, down, up, dtype=dtype)
    return fit(ys, np.asarray(y).size, dtype)


# ---- the library's draws (dsp_stop_train_uniform's generator) ---------------------------------------------------------------------------
def _mix(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(seed, stream, counter):
    """the 64-bit draw at (seed, stream, counter); counter may be an array"""
    with np.errstate(over="ignore"):
        base = _mix(np.uint64((seed + (stream + 1) * GOLDEN) & MASK))
        return _mix(base + (np.asarray(counter, np.uint64) + np.uint64(1)) * np.uint64(GOLDEN))


def uniform(seed, stream, counter):
    return (draw(seed, stream, counter) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def normal(seed, key, n, dtype=np.float64):
    """z_0 .. z_{n-1} of stream `key`: Box-Muller, one draw per pair of samples"""
    d = draw(seed, key, np.arange((n + 1) // 2))
    u1 = (((d >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24).astype(dtype)
    u2 = (((d >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24).astype(dtype)
    r = np.sqrt(dtype(-2) * np.log(u1)).astype(dtype)
    t = (dtype(2.0 * np.pi) * u2).astype(dtype)
    z = np.empty(2 * d.size, dtype)
    z[0::2] = r * np.cos(t)
    z[1::2] = r * np.sin(t)
    return z[:n]


def add_noise(y, sigma, seed, key, dtype=np.float64):
    y = np.asarray(y).astype(dtype)
    return (y + (dtype(sigma) * normal(seed, key, y.size, dtype)).astype(dtype)).astype(dtype)


def augment_draw(seed, labels, prob=0.5):
    """cepstrum/train.py's policy with the library's draws -> [(clip, kind, rate, n_steps, sigma, key)]"""
    ops = []
    for r, lab in enumerate(labels):
        if lab != 1 or not float(uniform(seed, POLICY_STREAM + 0, r)) < prob:
            continue
        kind = min(2, int(math.floor(3.0 * float(uniform(seed, POLICY_STREAM + 1, r)))))
        rate, n_steps, sigma = 1.0, 0, 0.0
        if kind == 0:
            rate = 0.8 + 0.4 * float(uniform(seed, POLICY_STREAM + 2, r))
        elif kind == 1:
            n_steps = min(4, int(math.floor(5.0 * float(uniform(seed, POLICY_STREAM + 3, r))))) - 2
        else:
            sigma = float(np.float32(0.005))
        ops.append((r, kind, rate, n_steps, sigma, r))
    return ops


def out_lengths(lens, ops):
    return [stretch_length(lens[c], rate) if kind == 0 else lens[c] for (c, kind, rate, _n, _s, _k) in ops]
