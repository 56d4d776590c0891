#!/usr/bin/env python3
"""Lane-level numpy model of the 400-point real FFT dataflow of dsp_amd/csrc/mfcc400_kernel.hip: which lane holds which point in each
pass, the exchanges through the wave's LDS image, the untangling of the packed transform.  The arithmetic is float64; the window and
every twiddle are the library's own float32 tables (dsp_mfcc400_tables, struct dsp::Tables400 of csrc/tables.hpp), so what the model
misses of np.fft.rfft is the tables' rounding and nothing else (tests/test_mfcc400_cpu.py bounds it).

64 lanes x up to 8 complex slots.  200 = 5 x 5 x 8, Stockham autosort: in the pass with Ns points done and radix R, butterfly j < 200 / R
takes x[j + (200 / R) t] W_{R Ns}^(t k), k = j % Ns, and writes y[(j - k) R + k + q Ns]."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = np.arange(64)


class Tables400(C.Structure):
    _fields_ = [("win", (C.c_float * 64) * 10), ("tw1", (C.c_float * 64) * 8), ("tw2", (C.c_float * 64) * 14), ("twu", (C.c_float * 64) * 4),
                ("mel_lo", C.c_int32 * 128), ("mel_len", C.c_int32 * 128), ("mel_off", C.c_int32 * 128), ("mel_w", C.c_float * 416),
                ("dct", (C.c_float * 128) * 32), ("dct_t", (C.c_float * 64) * 64), ("n_mels", C.c_int32), ("n_mfcc", C.c_int32),
                ("n_weights", C.c_int32)]


def load_tables(cfg):
    """the library's Tables400 for `cfg` as a dict of numpy arrays (float32 / int32, as stored)"""
    from dsp_amd import lib as dl
    lib = dl.load()
    t = Tables400()
    assert lib.dsp_mfcc400_tables(C.byref(cfg), None, 0) == C.sizeof(t), "Tables400 here and in csrc/tables.hpp differ"
    dl.check(lib.dsp_mfcc400_tables(C.byref(cfg), C.byref(t), C.sizeof(t)), "dsp_mfcc400_tables")
    out = {name: np.ctypeslib.as_array(getattr(t, name)).copy() for name, ty in Tables400._fields_ if not name.startswith("n_")}
    out.update(n_mels=t.n_mels, n_mfcc=t.n_mfcc, n_weights=t.n_weights)
    return out


def _pairs(tab):
    """[2 n][64] (cos, sin) rows -> complex [n][64]"""
    tab = tab.astype(np.float64)
    return tab[0::2] + 1j * tab[1::2]


def radix4(s):
    t0, t1 = s[0] + s[2], s[0] - s[2]
    t2, t3 = s[1] + s[3], (s[1] - s[3]) * (-1j)
    return np.stack([t0 + t2, t1 + t3, t0 - t2, t1 - t3])


def radix5(s):
    """s: [5][64] complex; the kernel's forward 5-point butterfly over axis 0"""
    c1, c2 = np.cos(2 * np.pi / 5), np.cos(4 * np.pi / 5)
    s1, s2 = np.sin(2 * np.pi / 5), np.sin(4 * np.pi / 5)
    a1, a2, b1, b2 = s[1] + s[4], s[2] + s[3], s[1] - s[4], s[2] - s[3]
    m1, m2 = s[0] + c1 * a1 + c2 * a2, s[0] + c2 * a1 + c1 * a2
    n1, n2 = s1 * b1 + s2 * b2, s2 * b1 - s1 * b2
    return np.stack([s[0] + a1 + a2, m1 - 1j * n1, m2 - 1j * n2, m2 + 1j * n2, m1 + 1j * n1])


def radix8(s):
    """s: [8][64] complex; two radix-4 butterflies and W8, natural order in and out"""
    e, o = radix4(s[0::2]), radix4(s[1::2])
    r2 = np.sqrt(0.5)
    o = o * np.array([1, r2 * (1 - 1j), -1j, r2 * (-1 - 1j)])[:, None]
    return np.concatenate([e + o, e - o])


def wave_rfft400(x, T):
    """x: [400] real samples, T: load_tables(cfg) -> X[0..200] complex, the kernel's bins before the power spectrum"""
    x = np.asarray(x, np.float64)
    win = T["win"].astype(np.float64)
    tw1, tw2, twu = _pairs(T["tw1"]), _pairs(T["tw2"]), _pairs(T["twu"])
    on5, on8 = L < 40, L < 25
    j5, j8 = np.minimum(L, 39), np.minimum(L, 24)
    # load + window (the table holds window / 2): lane j < 40, slot t: z[j + 40 t]; idle lanes hold 0
    n = np.minimum(L[None, :] + 40 * np.arange(5)[:, None], 199)
    v = np.where(on5, x[2 * n] * win[0::2] + 1j * x[2 * n + 1] * win[1::2], 0)
    lds = np.zeros(201, complex)
    # pass 0: R = 5, Ns = 1
    v = radix5(v)
    for q in range(5):
        lds[5 * L[on5] + q] = v[q][on5]
    # pass 1: R = 5, Ns = 5, k = lane % 5
    v = np.stack([lds[j5 + 40 * t] for t in range(5)])
    v[1:] = v[1:] * tw1
    v = radix5(v)
    k = L % 5
    for q in range(5):
        lds[(5 * (L - k) + k + 5 * q)[on5]] = v[q][on5]
    # pass 2: R = 8, Ns = 25, k = lane: natural order out
    v = np.stack([lds[j8 + 25 * t] for t in range(8)])
    v[1:] = v[1:] * tw2
    v = radix8(v)
    for q in range(8):
        lds[L[on8] + 25 * q] = v[q][on8]
    lds[200] = lds[0]
    # untangle: bins k = l + 64 t < 100 with 200 - k, bin 100 alone
    X = np.zeros(201, complex)
    for t in range(2):
        kk = L + 64 * t
        live = kk < 100
        kk = kk[live]
        a, b = lds[kk], lds[200 - kk]
        E, O = a + np.conj(b), a - np.conj(b)
        Tw = O * twu[t][live]
        X[kk] = E - 1j * Tw
        X[200 - kk] = np.conj(E + 1j * Tw)
    X[100] = 2 * np.conj(lds[100])
    return X


def main():
    from dsp_amd.mfcc import speaker_config
    cfg = speaker_config()
    T = load_tables(cfg)
    rng = np.random.default_rng(0)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)
    worst = 0.0
    for _ in range(8):
        x = rng.uniform(-1, 1, 400)
        err = np.abs(wave_rfft400(x, T) - np.fft.rfft(x * w)).max() / np.abs(x * w).sum()
        worst = max(worst, err)
    print(f"lane model vs np.fft.rfft on 8 noise frames: worst |err| / sum |x w| = {worst:.3e} (2^-23 = {2.0 ** -23:.3e})")


if __name__ == "__main__":
    main()
