"""The instantiations of the 512-point wave kernel (mfcc_kernels.hip, DSP_FOR_SHAPES) by name: one configuration per variant the host
table builder (build_lane_tables_512, tables.cpp) can select, and the inputs the shape tests run on them.

A variant is (dct_split, dct_len, mel_gather, mel_conflict_free, empty_filters):
    (dct_split, dct_len, mel_gather)  the kernel's template shape; (4,16,.) and (2,20,.) keep the MFMA A operand in LDS
    mel_conflict_free                 1: the matching placed every 12-bin window on its own bank residue; 0: the builder's fallback
    empty_filters                     filters without a single bin (every gather source is the zero slot)

SHAPES maps a name to (default_config overrides, variant).  tests/test_mfcc512_shapes_cpu.py holds every name to its variant, so a
change to the builder that moves a name to another instantiation fails there and not on a GPU; tests/test_gpu_mfcc512_shapes.py
runs every name at frame lengths 512 / 400 / 320 (FLEN 512, 400 where compiled in, the run-time predicate) and both log modes.

Nothing is unreachable: all six shapes occur with both placement states, and SHAPES has a name for each of the twelve.  The search
ran the builder over the fuzz's grid (tests/test_gpu_fuzz.py) -- sample rates 8000 / 16000 / 22050 / 44100, fmin 0 / 20 / 300, fmax
sr/2 / 0.45 sr / 0.3 sr, the three mel norms -- with n_mels 8..64 and n_mfcc 13 and 17.  (4,16,6,1): 2592 configurations with
n_mels 41..64, 24 of them (4,16,6,.), 10 of those conflict free; "mels41_g6" is the first on the HTK scale.  (4,10,3,0) and (2,20,3,0)
are the rarest, four configurations each, all 40 filters at 44.1 kHz up to 19 845 Hz.  Empty filters at n_fft 512: of 1609
configurations of that grid (fmax also 8000 / 4000 / 2000 / 1000) whose dense bank has an empty row, the builder accepts 1569;
"mels64_empty" (44.1 kHz, fmax 8000, 64 Slaney-normalised filters; filters 0, 3 and 6 lie between two bins) is also the (4,16,3,1)
name."""
import ctypes as C

import numpy as np

from tests import signals as S

HOP = 160
FRAME_LENGTHS = (512, 400, 320)
LOG_MODES = (0, 1)


def _bank(n_mels, n_mfcc, sample_rate, fmin, fmax, mel_norm):
    return dict(n_mels=n_mels, n_mfcc=n_mfcc, sample_rate=sample_rate, fmin=float(fmin), fmax=float(fmax), mel_norm=mel_norm)


# name -> (overrides, (dct_split, dct_len, mel_gather, mel_conflict_free, empty_filters))
SHAPES = {
    "default": (dict(), (4, 10, 3, 1, 0)),
    "mels32": (dict(n_mels=32), (4, 10, 6, 1, 0)),
    "mels16_8k_fallback": (_bank(16, 13, 8000, 0, 4000, 0), (4, 10, 6, 0, 0)),
    "mels64_empty": (_bank(64, 16, 44100, 0, 8000, 1), (4, 16, 3, 1, 3)),               # n_mfcc 16: the last count of split 4
    "mels41_fallback": (_bank(41, 13, 16000, 0, 8000, 0), (4, 16, 3, 0, 0)),            # the first n_mels past DCT_LEN 10
    "mels41_g6": (_bank(41, 13, 44100, 300, 22050, 0), (4, 16, 6, 1, 0)),
    "mels42_g6_fallback": (_bank(42, 13, 44100, 0, 22050, 0), (4, 16, 6, 0, 0)),
    "mfcc17": (dict(n_mfcc=17), (2, 20, 3, 1, 0)),                                       # the split switches from 4 to 2 here
    "mels40_44k_fallback_mfcc32": (_bank(40, 32, 44100, 0, 19845, 0), (2, 20, 3, 0, 0)),   # the most coefficients, both tiles full
    "mels17_mfcc17": (_bank(17, 17, 16000, 0, 8000, 0), (2, 20, 6, 1, 0)),              # n_mfcc == n_mels
    "mels20_mfcc17_fallback": (_bank(20, 17, 8000, 0, 4000, 0), (2, 20, 6, 0, 0)),
    "mfcc1": (dict(n_mfcc=1), (4, 10, 3, 1, 0)),
    "mels40_44k_fallback_mfcc16": (_bank(40, 16, 44100, 0, 19845, 0), (4, 10, 3, 0, 0)),
}
NAMES = list(SHAPES)
KERNEL_SHAPES = [(4, 10, 3), (4, 10, 6), (4, 16, 3), (4, 16, 6), (2, 20, 3), (2, 20, 6)]      # DSP_FOR_SHAPES


def overrides(name, frame_length=None, log_mode=None):
    over = dict(SHAPES[name][0])
    if frame_length is not None:
        over.update(frame_length=frame_length, hop_length=HOP)
    if log_mode is not None:
        over.update(log_mode=log_mode)
    return over


def config(name, frame_length=None, log_mode=None):
    import dsp_amd
    return dsp_amd.default_config(**overrides(name, frame_length, log_mode))


def oracle_cfg(name, frame_length=None, log_mode=None, fft_mode=None):
    from oracle import oracle as O
    return O.default_cfg(fft_mode=O.FFT_FLOAT64 if fft_mode is None else fft_mode, **overrides(name, frame_length, log_mode))


def lane_tables(cfg):
    """dsp_mfcc_lane_tables -> (LaneTables512, return code)"""
    import dsp_amd
    from dsp_amd import lib as dl
    L = dsp_amd.load()
    t = dl.LaneTables512()
    assert L.dsp_mfcc_lane_tables(C.byref(cfg), None, 0) == C.sizeof(t)
    return t, L.dsp_mfcc_lane_tables(C.byref(cfg), C.byref(t), C.sizeof(t))


def variant_of(t):
    src = np.array([list(t.mel_src[g]) for g in range(6)])
    empty = int((src[:, :t.n_mels] == 64).all(axis=0).sum())
    return (t.dct_split, t.dct_len, t.mel_gather, t.mel_conflict_free, empty)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# Every input is a function of the name's band and the frame length only, so that the CPU test that holds the reference to the
# gate on them and the GPU tests see the same samples.

def _seed(name, frame_length):
    return 7 * NAMES.index(name) + {512: 0, 400: 1, 320: 2}[frame_length]


def _chirp(name, n):
    """a sweep inside the bank: a tone outside [fmin, fmax] leaves every filter at the FFT's own float32 noise (test_gpu_fuzz.py)"""
    over = SHAPES[name][0]
    sr, fmin, fmax = over.get("sample_rate", 16000), over.get("fmin", 0.0), over.get("fmax", 8000.0)
    return S.chirp(n, fmin + 100.0, 0.9 * fmax, fs=float(sr))


# Row 5 of the 67-row input is full-scale noise times 1e-6: its mel energies lie within 10 dB of amin (1e-10), some filters on the
# floor and some above it, ||frame||_inf about 40.  At a third of that level (the row's level in the 1 / 0.3 / 0.03 turn) nearly every
# filter sits at amin, ||frame||_inf drops below 10 -- the regime of conftest.py's "tiny" golden -- and the reference's float32 FFT
# itself missed the pure gate of its float64 evaluation on two draws (default and mfcc1 at frame length 400: 1.1e-4 and 5.1e-4).
def frames_input(name, frame_length, n):
    """n independent frames: noise at levels 1 / 0.3 / 0.03 in turn and every fourth a piece of the in-band sweep; with 67 rows, row 33
    is all zeros and row 5 is noise scaled by 1e-6"""
    seed = 1000 + _seed(name, frame_length)
    x = S.uniform_pm1(n * frame_length, seed).reshape(n, frame_length).copy()
    sweep = _chirp(name, n * frame_length).reshape(n, frame_length)
    for i in range(n):
        if i % 4 == 3:
            x[i] = sweep[i]
        else:
            x[i] *= np.float32((1.0, 0.3, 0.03)[i % 4])
    if n == 67:
        x[33] = 0.0
        x[5] = S.uniform_pm1(frame_length, seed + 5000) * np.float32(1e-6)
    return np.ascontiguousarray(x, np.float32)


CLIP_FRAMES = 19
CLIP_KINDS = ("noise", "chirp", "quiet_half_silent")


def clips_input(name, frame_length):
    """three clips of 19 frames: noise, the in-band sweep, and 0.003 x noise with a silent second half"""
    n = frame_length + (CLIP_FRAMES - 1) * HOP
    seed = 2000 + _seed(name, frame_length)
    quiet = S.uniform_pm1(n, seed + 500) * np.float32(0.003)
    quiet[n // 2:] = 0.0
    return [S.uniform_pm1(n, seed), _chirp(name, n), quiet.astype(np.float32)]


RAGGED_START = 3


def ragged_lengths(frame_length):
    """no frame, exactly one, one and a hop less one sample, about 7 frames, about 23 frames"""
    return [frame_length - 1, frame_length, frame_length + HOP - 1, frame_length + 6 * HOP + 57, frame_length + 22 * HOP + 101]


def ragged_input(name, frame_length):
    """-> (buffer with NaN outside the clips, offsets): five clips back to back from the odd sample RAGGED_START; the clips are noise
    at levels 0.7 / 0.7 / 0.1, a sweep, and noise whose middle third is 0.01 of the rest"""
    lens = ragged_lengths(frame_length)
    offsets = np.concatenate([[RAGGED_START], RAGGED_START + np.cumsum(lens)]).astype(np.int64)
    seed = 3000 + _seed(name, frame_length)
    buf = np.full(int(offsets[-1]) + 5, np.nan, np.float32)
    for c, n in enumerate(lens):
        if c == 3:
            x = _chirp(name, n)
        else:
            x = S.uniform_pm1(n, seed + 100 * c) * np.float32((0.7, 0.7, 0.1, 0.0, 0.5)[c])
        if c == 4:
            x[n // 3: 2 * n // 3] *= np.float32(0.01)
        buf[offsets[c]:offsets[c + 1]] = x
    return buf, offsets
