"""The resampler's definition (include/dsp_amd.h) restated in numpy, from the formula:

    g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, m = max(up, down), half = 10 m
    v[n] = sinc((n - half) / m) / m * I0(5 sqrt(1 - ((n - half) / half)^2)) / I0(5),   h = up v / sum(v)        (2 half + 1 taps)
    y[k] = sum_i x[i] h[k down + half - i up],   0 <= i < n,  0 <= k down + half - i up <= 2 half,   k < ceil(n up / down)

float64 by default.  dtype=np.float32 is the model of the GPU arithmetic: the taps rounded once to float32, every product and every
partial sum rounded to float32, in ascending i."""
import math

import numpy as np

RATE_PAIRS = [(8000, 16000), (9000, 16000), (10000, 16000), (11025, 16000), (22050, 16000), (24000, 16000), (32000, 16000),
              (44100, 16000), (48000, 16000), (96000, 16000), (16000, 16000)]


def ratio(rate_in, rate_out):
    """-> (up, down, half)"""
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    return up, down, 10 * max(up, down)


def taps(rate_in, rate_out):
    up, down, half = ratio(rate_in, rate_out)
    m = max(up, down)
    t = (np.arange(2 * half + 1, dtype=np.float64) - half)
    arg = np.pi * t / m
    sinc = np.ones_like(t)
    nz = t != 0
    sinc[nz] = np.sin(arg[nz]) / arg[nz]
    v = sinc / m * np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(5.0)
    return up * v / v.sum()


def out_len(n, up, down):
    return -((-n * up) // down)


def offsets(rate_in, rate_out, offs):
    up, down, _ = ratio(rate_in, rate_out)
    offs = np.asarray(offs, np.int64)
    return np.concatenate([[0], np.cumsum([out_len(int(n), up, down) for n in np.diff(offs)])]).astype(np.int64)


def resample(x, rate_in, rate_out, dtype=np.float64, with_bound=False, h64=None):
    """y[ceil(n up / down)] of x[n] in `dtype` arithmetic; with_bound: also sum_i |x[i] h[.]| (float64) and the terms L_k per output.
    h64: other float64 taps than the definition's, 2 half + 1 of them (the mutants of tests/resample_shapes.py)."""
    up, down, half = ratio(rate_in, rate_out)
    h64 = taps(rate_in, rate_out) if h64 is None else np.asarray(h64, np.float64)
    assert h64.shape == (2 * half + 1,)
    x64 = np.asarray(x, np.float64)
    n = x64.size
    n_out = out_len(n, up, down)
    if up == 1 and down == 1:
        y = np.asarray(x, dtype).copy()
        return (y, np.abs(x64), np.ones(n, np.int64)) if with_bound else y
    h = h64.astype(dtype)
    xs = x64.astype(dtype)
    per_branch = (2 * half + up) // up
    k = np.arange(n_out, dtype=np.int64)
    a = k * down + half
    i_max, p = a // up, a % up
    y = np.zeros(n_out, dtype)
    mag = np.zeros(n_out, np.float64)
    terms = np.zeros(n_out, np.int64)
    for jj in range(per_branch):                           # ascending input sample
        i = i_max - (per_branch - 1) + jj
        t = p + (per_branch - 1 - jj) * up
        ok = (i >= 0) & (i < n) & (t <= 2 * half)
        if not ok.any():
            continue
        io, to = i[ok], t[ok]
        y[ok] = (y[ok] + (xs[io] * h[to]).astype(dtype)).astype(dtype)
        if with_bound:
            mag[ok] += np.abs(x64[io] * h64[to])
            terms[ok] += 1
    return (y, mag, terms) if with_bound else y


def decode_pcm16(pcm, stereo_mode=0):
    """int16 [n] or interleaved [n][2] -> the float32 samples the kernels decode (exact in float32)."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 1:
        return (pcm.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    left, right = pcm[:, 0].astype(np.float32) / np.float32(32768.0), pcm[:, 1].astype(np.float32) / np.float32(32768.0)
    return left if stereo_mode == 0 else (np.float32(0.5) * (left + right)).astype(np.float32)
