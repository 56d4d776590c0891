"""The forms of the three wide MFCC kernels by name -- mfcc1024_wave_kernel.hip and mfcc1024_kernel.hip (tables: build_gen_tables_1024) and
mfcc2048_kernel.hip (build_gen_tables_2048) -- one configuration per form the host table builders can select, and the inputs the
shape tests run on them.  The same shape as tests/mfcc512_shapes.py: SHAPES_1024 / SHAPES_2048 map a name to (default_config
overrides, variant); tests/test_mfcc_wide_shapes_cpu.py holds every name to its variant through dsp_mfcc1024_tables /
dsp_mfcc2048_tables, so a change to a builder that moves a name to another form fails there and not on a GPU;
tests/test_gpu_mfcc1024_shapes.py and tests/test_gpu_mfcc2048_shapes.py run every name.

1024 variant: (n_chunk_slots, max gather pieces of any filter, conflict_free, empty_filters, n_mels > 64)
    n_chunk_slots   12-bin chunk slots per lane in use; <= 3 fits the wave kernel, 4 would select the Stockham kernel by itself
    gather pieces   chunks of the widest filter: <= 3, or 4..6 (6: a filter of 61..72 bins)
    conflict_free   1: within each slot and each 32-lane half the windows of the lanes with a non-zero weight start at distinct
                    addresses mod 32 (the Kuhn matching placed every chunk); 0: the builder's fallback
    empty_filters   filters without a bin: all six gather sources are the zero slot (256; the wave kernel remaps it to its slot 192)
    n_mels > 64     the lane's second filter is in use
2048 variant: (aubio family, seg_ok, max pieces of any filter, total segments, empty_filters, n_mels > 64, n_mels odd)
    aubio family    the plan runs mfcc2048_kernel<AUB> (magnitude spectrum, log10 floor or stream framing): weights in LDS, samples
                    requested a frame ahead
    seg_ok          1: the kernel dots 16-bin segments on all lanes; 0: it walks the CSR rows, because a filter has more than 12
                    pieces (more than 192 bins) or the bank more than 192 segments

The search ran both exporters over the fuzz's grid (tests/test_gpu_fuzz.py): sample rates 8000 / 16000 / 22050 / 44100, fmin 0 / 20 /
300, fmax sr/2 / 0.45 sr / 0.3 sr and 8000 / 4000 / 2000 / 1000 where lower than 0.3 sr, the three mel norms, n_mels 8..128: 26 136
configurations per kernel.
  1024: the builder accepts 23 757 and refuses 2379 ("a mel filter spans more than 72 bins").  Slots 1 / 2 / 3 occur 7232 / 14 069 / 2456
        times, never 4; the fallback placement with 1 slot (329) and with 2 slots (11), never with 3; filters of 4..5 pieces with every
        slot count (792 / 2164 / 187), of 6 pieces with 1 and 2 slots (240 / 541); empty filters with every slot count (1067 / 2101 / 86).
  2048: the builder accepts all 26 136.  seg_ok 0 by a filter of more than 12 pieces: 1425 (n_mels 8..38); by more than 192 segments:
        104 (n_mels 114..128, 193..202 segments), never by both; a filter of exactly 12 pieces: 261 (n_mels 8..42); 191 and 192 segments
        with seg_ok 1 both occur; empty filters: 819, all on the segment path (at most 127 segments, filters of one piece).
UNREACHABLE lists what no accepted configuration of that grid reaches, UNLAUNCHED the kernel instantiations no path launches.

Which form the shipped front ends run (test_product_configurations_and_their_forms): the 128-filter 1024-point bank has 3 slots, every
chunk placed; scrubjay_infer.c's aubio front end (130 segments) and the 128-filter librosa front end at 16 kHz (190 segments) run the
segment path, the librosa front end at 22.05 kHz (195 segments) walks the CSR rows."""
import ctypes as C

import numpy as np

from tests import signals as S

FRAME_LENGTHS = {1024: (1024, 800), 2048: (2048, 1200)}
HOPS = {1024: 512, 800: 320, 2048: 512, 1200: 400}


def _bank(n_fft, n_mels, n_mfcc, sample_rate, fmin, fmax, mel_norm, **more):
    return dict(n_fft=n_fft, n_mels=n_mels, n_mfcc=n_mfcc, sample_rate=sample_rate, fmin=float(fmin), fmax=float(fmax), mel_norm=mel_norm, **more)


# name -> (overrides, (n_chunk_slots, max gather pieces, conflict_free, empty_filters, n_mels > 64))
SHAPES_1024 = {
    "htk128": (_bank(1024, 128, 13, 16000, 0, 8000, 0), (3, 2, 1, 0, 1)),                      # the product bank (BASELINE config 3)
    "mels31_8k_fallback": (_bank(1024, 31, 13, 8000, 0, 2400, 0), (1, 3, 0, 0, 0)),
    "mels15_8k_g6_mfcc1": (_bank(1024, 15, 1, 8000, 0, 2400, 0), (1, 6, 1, 0, 0)),
    "mels18_8k_g5_fallback": (_bank(1024, 18, 13, 8000, 0, 2400, 0), (1, 5, 0, 0, 0)),
    "mels40_librosa_g6_fallback_mfcc16": (_bank(1024, 40, 16, 16000, 0, 8000, 2), (2, 6, 0, 0, 0)),
    "mels64_8k": (_bank(1024, 64, 13, 8000, 0, 4000, 0), (2, 3, 1, 0, 0)),                     # the last n_mels with the second filter idle
    "mels65_8k": (_bank(1024, 65, 13, 8000, 0, 4000, 0), (2, 3, 1, 0, 1)),
    "mels65_44k_librosa_g6": (_bank(1024, 65, 13, 44100, 0, 22050, 2), (2, 6, 1, 0, 1)),        # filter 64, a lane's second, has 6 pieces
    "mels84_22k_librosa_g4": (_bank(1024, 84, 13, 22050, 0, 11025, 2), (3, 4, 1, 0, 1)),
    "mels116_44k_empty": (_bank(1024, 116, 16, 44100, 0, 22050, 0), (3, 3, 1, 1, 1)),
    "mels63_44k_empty_fallback": (_bank(1024, 63, 13, 44100, 0, 2000, 0), (1, 1, 0, 3, 0)),
    "mels8_8k_mfcc16": (_bank(1024, 8, 16, 8000, 0, 1000, 0), (1, 4, 1, 0, 0)),                 # n_mfcc > n_mels: valid_cfg, the builder and the oracle all take it
}
NAMES_1024 = list(SHAPES_1024)
# wanted form -> does (overrides, variant) have it
WANTED_1024 = {
    "1 slot": lambda o, v: v[0] == 1, "2 slots": lambda o, v: v[0] == 2, "3 slots": lambda o, v: v[0] == 3, "4 slots": lambda o, v: v[0] == 4,
    "1 slot placed": lambda o, v: v[0] == 1 and v[2] == 1, "1 slot fallback": lambda o, v: v[0] == 1 and v[2] == 0,
    "2 slots placed": lambda o, v: v[0] == 2 and v[2] == 1, "2 slots fallback": lambda o, v: v[0] == 2 and v[2] == 0,
    "3 slots placed": lambda o, v: v[0] == 3 and v[2] == 1, "3 slots fallback": lambda o, v: v[0] == 3 and v[2] == 0,
    "gather <= 3": lambda o, v: v[1] <= 3, "gather 4..5": lambda o, v: v[1] in (4, 5), "gather 6": lambda o, v: v[1] == 6,
    "gather 6 on a lane's second filter": lambda o, v: v[1] == 6 and v[4] == 1,
    "empty filters, n_mels <= 64": lambda o, v: v[3] > 0 and v[4] == 0, "empty filters, n_mels > 64": lambda o, v: v[3] > 0 and v[4] == 1,
    "n_mels 64": lambda o, v: o["n_mels"] == 64, "n_mels 65": lambda o, v: o["n_mels"] == 65, "n_mels 128": lambda o, v: o["n_mels"] == 128,
    "n_mfcc 1": lambda o, v: o["n_mfcc"] == 1, "n_mfcc 16": lambda o, v: o["n_mfcc"] == 16, "n_mfcc > n_mels": lambda o, v: o["n_mfcc"] > o["n_mels"],
    "the wave kernel's slot 191 in use": lambda o, v: False,
}
UNREACHABLE_1024 = {
    "4 slots": "more than 192 chunks: the grid's fullest bank has 167 (128 librosa filters, 44.1 kHz, 20 .. 22 050 Hz), and neither 48 / 96 kHz nor "
               "fmin 1000 / 2000 nor fmax down to 0.2 sr (another 70 000 configurations, n_mels 70..128) gets past it; only "
               "DSP_KERNEL_ROW runs the Stockham kernel",
    "3 slots fallback": "0 of the grid's 2456 three-slot configurations: the matching always places them",
    "the wave kernel's slot 191 in use": "lane 63 of slot 2 holds a chunk in none of the grid's three-slot banks (at most 167 chunks), so partial "
                                         "191 is always 0 and remapping the zero slot to it computes the same values",
}
# kernel instantiations no path launches
UNLAUNCHED = {
    "mfcc1024_wave_kernel<true, false, true> (six scan steps everywhere)": "both literal filters have an instantiation of their own "
                                                                           "(<.., 1, 3, 3, 5> and <.., 2, 3, 3, 4>); the plan knows no other coefficients",
}
# name -> (overrides, (aubio family, seg_ok, max pieces, total segments, empty_filters, n_mels > 64, n_mels odd))
_AUBIO = dict(n_fft=2048, n_mels=40, n_mfcc=20, sample_rate=16000, fmin=0.0, fmax=8000.0, mel_norm=3, log_mode=2, spectrum=1, framing=1)
SHAPES_2048 = {
    "aubio": (_AUBIO, (1, 1, 8, 130, 0, 0, 0)),                                             # dsp_mfcc_scrubjay_infer_config(16000)
    "stream_only40": (_bank(2048, 40, 13, 16000, 0, 8000, 0, framing=1), (1, 1, 9, 142, 0, 0, 0)),   # one aubio option alone
    "librosa128": (_bank(2048, 128, 20, 16000, 0, 8000, 2), (0, 1, 3, 190, 0, 1, 0)),            # cepstrum/train.py's front end at 16 kHz
    "librosa128_22k_csr": (_bank(2048, 128, 20, 22050, 0, 11025, 2), (0, 0, 4, 195, 0, 1, 0)),   # the same at 22.05 kHz: more than 192 segments
    "htk128_22k_192seg_mfcc32": (_bank(2048, 128, 32, 22050, 0, 11025, 0), (0, 1, 3, 192, 0, 1, 0)),
    "mels127_22k_csr": (_bank(2048, 127, 13, 22050, 0, 11025, 2), (0, 0, 4, 194, 0, 1, 1)),
    "mels127_22k_191seg": (_bank(2048, 127, 13, 22050, 0, 11025, 0), (0, 1, 3, 191, 0, 1, 1)),
    "mels8_8k_wide_csr": (_bank(2048, 8, 8, 8000, 0, 4000, 0), (0, 0, 26, 113, 0, 0, 0)),
    "mels22_8k_p12_mfcc1": (_bank(2048, 22, 1, 8000, 0, 4000, 0), (0, 1, 12, 130, 0, 0, 0)),
    "mels63_librosa": (_bank(2048, 63, 13, 16000, 300, 8000, 2), (0, 1, 6, 146, 0, 0, 1)),
    "mels64_librosa": (_bank(2048, 64, 13, 16000, 20, 8000, 2), (0, 1, 6, 147, 0, 0, 0)),
    "mels65_8k": (_bank(2048, 65, 13, 8000, 0, 4000, 0), (0, 1, 5, 154, 0, 1, 1)),
    "mels58_44k_empty": (_bank(2048, 58, 13, 44100, 0, 1000, 0), (0, 1, 1, 57, 1, 0, 0)),
    "mels117_22k_empty": (_bank(2048, 117, 13, 22050, 0, 1000, 0), (0, 1, 1, 116, 1, 1, 1)),
    "stream_only8_csr": (_bank(2048, 8, 8, 8000, 0, 4000, 0, framing=1), (1, 0, 26, 113, 0, 0, 0)),   # the aubio kernels' CSR walk
}
NAMES_2048 = list(SHAPES_2048)
# n_mfcc 1 sits on the 22-filter bank: with one coefficient the gate is relative to |c0| alone, and on the 8-filter CSR bank the reference's
# float32 evaluation missed the gate of its float64 one on the sweep clip in log mode 1 (5.3e-4 at frame length 2048; 4.0e-5 here).
WANTED_2048 = {
    "segments": lambda o, v: v[1] == 1, "CSR by a filter of more than 12 pieces": lambda o, v: v[1] == 0 and v[2] > 12,
    "CSR by more than 192 segments": lambda o, v: v[1] == 0 and v[2] <= 12 and v[3] > 192,
    "a filter of exactly 12 pieces": lambda o, v: v[1] == 1 and v[2] == 12, "191 segments": lambda o, v: v[1] == 1 and v[3] == 191,
    "192 segments": lambda o, v: v[1] == 1 and v[3] == 192,
    "empty filters, n_mels <= 64": lambda o, v: v[4] > 0 and v[5] == 0, "empty filters, n_mels > 64": lambda o, v: v[4] > 0 and v[5] == 1,
    "empty filters on the CSR path": lambda o, v: v[4] > 0 and v[1] == 0,
    "n_mels 63": lambda o, v: o["n_mels"] == 63, "n_mels 64": lambda o, v: o["n_mels"] == 64, "n_mels 65": lambda o, v: o["n_mels"] == 65,
    "n_mels 127": lambda o, v: o["n_mels"] == 127, "n_mels 128": lambda o, v: o["n_mels"] == 128,
    "CSR, n_mels odd and > 64": lambda o, v: v[1] == 0 and v[5] == 1 and v[6] == 1, "CSR, n_mels <= 64": lambda o, v: v[1] == 0 and v[5] == 0,
    "n_mfcc 1": lambda o, v: o["n_mfcc"] == 1, "n_mfcc 32": lambda o, v: o["n_mfcc"] == 32,
    "the aubio family": lambda o, v: v[0] == 1 and (o.get("spectrum"), o.get("log_mode"), o.get("framing"), o["mel_norm"]) == (1, 2, 1, 3),
    "one aubio option alone": lambda o, v: v[0] == 1 and [o.get("spectrum", 0) == 1, o.get("log_mode", 0) == 2, o.get("framing", 0) == 1].count(True) == 1,
    "the aubio family on the CSR path": lambda o, v: v[0] == 1 and v[1] == 0,
    "seg_ok 1 at 128 filters": lambda o, v: o["n_mels"] == 128 and v[:2] == (0, 1), "seg_ok 0 at 128 filters": lambda o, v: o["n_mels"] == 128 and v[:2] == (0, 0),
}
UNREACHABLE_2048 = {
    "empty filters on the CSR path": "0 of the grid's 819 banks with an empty filter: they have at most 127 segments and filters of one piece",
}
SHAPES = {1024: SHAPES_1024, 2048: SHAPES_2048}
WANTED = {1024: WANTED_1024, 2048: WANTED_2048}
UNREACHABLE = {1024: UNREACHABLE_1024, 2048: UNREACHABLE_2048}


def overrides(n_fft, name, frame_length=None, log_mode=None):
    over = dict(SHAPES[n_fft][name][0])
    if frame_length is not None:
        over.update(frame_length=frame_length, hop_length=HOPS[frame_length])
    if log_mode is not None:
        over.update(log_mode=log_mode)
    return over


def config(n_fft, name, frame_length=None, log_mode=None, **more):
    import dsp_amd
    return dsp_amd.default_config(**dict(overrides(n_fft, name, frame_length or n_fft, log_mode), **more))


def is_aubio(name):
    return SHAPES_2048[name][1][0] == 1


def log_modes(name):
    """the log modes the name's family takes: both reference modes for plain plans, its own for the aubio family"""
    return (SHAPES_2048[name][0].get("log_mode", 0),) if is_aubio(name) else (0, 1)


def gen_tables(cfg):
    """dsp_mfcc1024_tables / dsp_mfcc2048_tables by cfg.n_fft -> (GenTables1024 | GenTables2048, return code)"""
    import dsp_amd
    from dsp_amd import lib as dl
    L = dsp_amd.load()
    t, fn = (dl.GenTables1024(), L.dsp_mfcc1024_tables) if cfg.n_fft == 1024 else (dl.GenTables2048(), L.dsp_mfcc2048_tables)
    assert fn(C.byref(cfg), None, 0) == C.sizeof(t), "the ctypes mirror and csrc/tables.hpp differ"
    return t, fn(C.byref(cfg), C.byref(t), C.sizeof(t))


def arr(field):
    return np.ctypeslib.as_array(field)


ZERO_SLOT_1024 = 256


def variant_1024(t):
    src = arr(t.mel_src).transpose(0, 2, 1).reshape(128, 6)[:t.n_mels]        # filter m = lane + 64 i -> its six sources
    pieces = (src != ZERO_SLOT_1024).sum(axis=1)
    k0, w = arr(t.mel_k0), arr(t.mel_w)
    conflict_free = 1
    for s in range(t.n_chunk_slots):
        for half in (slice(0, 32), slice(32, 64)):
            busy = w[s][:, half].any(axis=0)
            starts = k0[s][half][busy] % 32
            if len(set(starts.tolist())) != starts.size:
                conflict_free = 0
    return (t.n_chunk_slots, int(pieces.max()), conflict_free, int((pieces == 0).sum()), int(t.n_mels > 64))


def variant_2048(t, cfg):
    ln = arr(t.mel_len)[:t.n_mels]
    pieces = -(-ln // 16)
    aubio = int(cfg.spectrum != 0 or cfg.log_mode == 2 or cfg.framing == 1)
    return (aubio, t.seg_ok, int(pieces.max()), int(pieces.sum()), int((ln == 0).sum()), int(t.n_mels > 64), t.n_mels & 1)


def variant_of(t, cfg):
    return variant_1024(t) if cfg.n_fft == 1024 else variant_2048(t, cfg)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
# Plain plans: the oracle's chain with its float64 FFT.  The aubio family has two references: the canonical front end is
# oracle/aubio_oracle.c (float64 FFT; its window is the transform's length, so the name runs at frame length 2048 only), and a plan
# with stream framing alone is the plain oracle on the frames written out (the vocoder's zero history in front, zeros past the end).

def is_stream(n_fft, name):
    return SHAPES[n_fft][name][0].get("framing", 0) == 1


def frame_lengths(n_fft, name):
    return (2048,) if name == "aubio" else FRAME_LENGTHS[n_fft]


def oracle_cfg(n_fft, name, frame_length, log_mode=None, fft_mode=None, **more):
    from oracle import oracle as O
    over = {k: v for k, v in overrides(n_fft, name, frame_length, log_mode).items() if k not in ("spectrum", "framing")}
    return O.default_cfg(fft_mode=O.FFT_FLOAT64 if fft_mode is None else fft_mode, **dict(over, **more))


def stream_frames(x, frame_length, hop):
    """DSP_FRAMING_STREAM written out: frame t = samples [(t + 1) hop - frame_length, (t + 1) hop) of the clip, zeros outside it"""
    t = -(-x.size // hop)
    padded = np.concatenate([np.zeros(frame_length - hop, np.float32), x, np.zeros(t * hop - x.size, np.float32)])
    return np.stack([padded[i * hop: i * hop + frame_length] for i in range(t)]) if t else np.zeros((0, frame_length), np.float32)


def reference_frames(n_fft, name, frame_length, log_mode, x, fft_mode=None, **more):
    """the oracle on independent frames x[n][frame_length]"""
    from oracle import oracle as O
    if name == "aubio":
        over = SHAPES_2048[name][0]
        assert frame_length == 2048 and fft_mode is None and not more
        return O.aubio_mfcc_clip(x.reshape(-1), over["sample_rate"], 2048, 2048, over["n_mels"], over["n_mfcc"])     # hop = frame: the frames as they are
    return O.mfcc_frames(x, oracle_cfg(n_fft, name, frame_length, log_mode, fft_mode, **more))


def reference_clip(n_fft, name, frame_length, log_mode, x, fft_mode=None):
    """the oracle on one clip, every frame the name's framing gives it"""
    from oracle import oracle as O
    if name == "aubio":
        over = SHAPES_2048[name][0]
        assert frame_length == 2048 and fft_mode is None
        return O.aubio_mfcc_clip(x, over["sample_rate"], 2048, HOPS[frame_length], over["n_mels"], over["n_mfcc"])
    cfg = oracle_cfg(n_fft, name, frame_length, log_mode, fft_mode)
    if is_stream(n_fft, name):
        assert cfg.log_mode == 0, "a clip-global floor would need the clip's frames together"
        return O.mfcc_frames(stream_frames(x, frame_length, HOPS[frame_length]), cfg)
    return O.compute_mfcc(x, 1000, cfg)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# Every input is a function of the name's band and the frame length only, so that the CPU test that holds the reference to the
# gate on them and the GPU tests see the same samples.

def _seed(n_fft, name, frame_length):
    return n_fft + 7 * list(SHAPES[n_fft]).index(name) + FRAME_LENGTHS[n_fft].index(frame_length)


# Under DSP_LOG_LOG10_FLOOR ("aubio") the sweep carries noise at 1e-3 of full scale, as the "chirp+noise" clip of
# tests/test_gpu_scrubjay.py does.  aubio's log10 has no floor relative to the frame's maximum, so in a frame of a bare sweep the filters
# away from the tone show the transform's own rounding at full size: a float32 numpy evaluation of the chain misses the pure gate of
# oracle/aubio_oracle.c on every bare sweep row of frames_input (2e-3 .. 1.7e-2; a float64 one, which does not round the spectrum to
# float as aubio does, 2e-4 .. 2e-3), and the kernel by the same 1.3e-2.  tests/test_mfcc_wide_shapes_cpu.py holds the float32
# evaluation to the gate on the inputs as they are now.
def _chirp(n_fft, name, n, seed):
    """a sweep inside the bank, fmin + 100 to 0.9 fmax at the name's rate (outside it every filter holds the FFT's own float32 noise)"""
    over = SHAPES[n_fft][name][0]
    sweep = S.chirp(n, over["fmin"] + 100.0, 0.9 * over["fmax"], fs=float(over["sample_rate"]))
    if over.get("log_mode", 0) == 2:
        sweep = sweep + np.float32(1e-3) * S.uniform_pm1(n, seed + 7000)
    return sweep.astype(np.float32)


FRAME_ROWS = {1024: (1, 7, 8, 9, 16, 17, 67), 2048: (1, 3, 4, 5, 67)}       # around the wave kernel's 8-frame granule and 16-frame tile; the 2048 block's four waves
ZERO_ROW, QUIET_ROW = 33, 2


def frames_input(n_fft, name, frame_length):
    """67 independent frames (the smaller counts take the first rows): noise at levels 1 / 0.3 / 0.03 in turn and every fourth a piece of
    the in-band sweep; row 33 is all zeros and row 2 is noise scaled by 1e-6"""
    n = 67
    seed = 1000 + _seed(n_fft, name, frame_length)
    x = S.uniform_pm1(n * frame_length, seed).reshape(n, frame_length).copy()
    sweep = _chirp(n_fft, name, n * frame_length, seed).reshape(n, frame_length)
    for i in range(n):
        if i % 4 == 3:
            x[i] = sweep[i]
        else:
            x[i] *= np.float32((1.0, 0.3, 0.03)[i % 4])
    x[ZERO_ROW] = 0.0
    x[QUIET_ROW] = S.uniform_pm1(frame_length, seed + 5000) * np.float32(1e-6)
    return np.ascontiguousarray(x, np.float32)


CLIP_FRAMES = 19
CLIP_KINDS = ("noise", "chirp", "quiet_half_silent")


def clip_samples(n_fft, name, frame_length):
    """19 complete frames; under stream framing 101 samples more, so that the clip is odd and its last hop partial"""
    return frame_length + (CLIP_FRAMES - 1) * HOPS[frame_length] + (101 if is_stream(n_fft, name) else 0)


# The third clip's level.  On the 2048-point names it has to make DSP_LOG_GLOBAL_REF1's floor, 80 dB below the clip's maximum, lie above
# amin (-100 dB), or the silent half sits at amin and the floor clips nothing: at 0.003 the Slaney-normalised banks' loudest filter is at
# -20 dB ("mels64_librosa": silent rows at exactly -100 dB).  At 0.1 the floor lies 10 dB or more above amin on every name.
QUIET_LEVEL = {1024: 0.003, 2048: 0.1}


def clips_input(n_fft, name, frame_length):
    """three clips: noise, the in-band sweep, and QUIET_LEVEL x noise with a silent second half"""
    n = clip_samples(n_fft, name, frame_length)
    seed = 2000 + _seed(n_fft, name, frame_length)
    quiet = S.uniform_pm1(n, seed + 500) * np.float32(QUIET_LEVEL[n_fft])
    quiet[n // 2:] = 0.0
    return [S.uniform_pm1(n, seed), _chirp(n_fft, name, n, seed), quiet.astype(np.float32)]


RAGGED_START = 3


def ragged_lengths(n_fft, name, frame_length):
    """no frame, exactly one, one and a hop less one sample, 7 frames, 23 frames"""
    hop = HOPS[frame_length]
    if is_stream(n_fft, name):          # a frame per started hop
        return [0, hop, 2 * hop - 1, 6 * hop + 57, 22 * hop + 101]
    return [frame_length - 1, frame_length, frame_length + hop - 1, frame_length + 6 * hop + 57, frame_length + 22 * hop + 101]


def ragged_input(n_fft, name, frame_length):
    """-> (buffer with NaN outside the clips, offsets): five clips back to back from the odd sample RAGGED_START; the clips are noise
    at levels 0.7 / 0.7 / 0.1, a sweep, and noise whose middle third is 0.01 of the rest"""
    lens = ragged_lengths(n_fft, name, frame_length)
    offsets = np.concatenate([[RAGGED_START], RAGGED_START + np.cumsum(lens)]).astype(np.int64)
    seed = 3000 + _seed(n_fft, name, frame_length)
    buf = np.full(int(offsets[-1]) + 5, np.nan, np.float32)
    for c, n in enumerate(lens):
        if c == 3:
            x = _chirp(n_fft, name, n, seed)
        else:
            x = S.uniform_pm1(n, seed + 100 * c) * np.float32((0.7, 0.7, 0.1, 0.0, 0.5)[c])
        if c == 4:
            x[n // 3: 2 * n // 3] *= np.float32(0.01)
        buf[offsets[c]:offsets[c + 1]] = x
    return buf, offsets
