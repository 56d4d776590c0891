"""CPU: every named configuration of tests/mfcc_wide_shapes.py against the host table builders (build_gen_tables_1024 /
build_gen_tables_2048, tables.cpp, through dsp_mfcc1024_tables / dsp_mfcc2048_tables) -- the variant each name selects, the sparse mel
tables against the dense bank, the DCT layouts -- the exporters' refusals against dsp_mfcc_plan_create's rules, and the oracle's own
float32 noise on the inputs the GPU shape tests use, so that their gate is a statement about the kernels."""
import ctypes as C

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from oracle import oracle as O
from tests import mfcc_wide_shapes as M
from tests.conftest import RTOL, frame_linf_close

CASES = [(n_fft, name) for n_fft in (1024, 2048) for name in M.SHAPES[n_fft]]


def _tables(n_fft, name, **more):
    cfg = M.config(n_fft, name, **more)
    t, rc = M.gen_tables(cfg)
    assert rc == 0, dl.last_error()
    return cfg, t


@pytest.mark.parametrize("n_fft,name", CASES)
def test_name_selects_its_variant(n_fft, name):
    cfg, t = _tables(n_fft, name)
    assert M.variant_of(t, cfg) == M.SHAPES[n_fft][name][1]
    assert (t.n_mels, t.n_mfcc) == (cfg.n_mels, cfg.n_mfcc)
    # the frame length and the log mode choose the load and the epilogue, never the tables' shape
    for frame_length in M.FRAME_LENGTHS[n_fft]:
        for log_mode in (M.log_modes(name) if n_fft == 2048 else (0,)):
            cfg2 = M.config(n_fft, name, frame_length, log_mode)
            t2, rc = M.gen_tables(cfg2)
            assert rc == 0 and M.variant_of(t2, cfg2) == M.SHAPES[n_fft][name][1]


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_every_wanted_form_has_a_name_or_is_listed_unreachable(n_fft):
    for form, has in M.WANTED[n_fft].items():
        names = [name for name, (over, v) in M.SHAPES[n_fft].items() if has(over, v)]
        if form in M.UNREACHABLE[n_fft]:
            assert not names, f"{form}: listed as unreachable, but {names} reach it"
        else:
            assert names, f"{form}: no name"
    assert set(M.UNREACHABLE[n_fft]) <= set(M.WANTED[n_fft])
    assert len(M.SHAPES[n_fft]) <= 16


def test_product_configurations_and_their_forms():
    """what the shipped front ends run: the 128-filter 1024-point bank in three slots, every chunk placed; scrubjay_infer.c's aubio front
    end and the librosa front end at 16 kHz on the segment path, the librosa front end at 22.05 kHz on the CSR path"""
    from dsp_amd import scrubjay
    cfg = dsp_amd.default_config(n_fft=1024, frame_length=1024, hop_length=1024, n_mels=128)
    t, rc = M.gen_tables(cfg)
    assert rc == 0 and M.variant_1024(t) == M.SHAPES_1024["htk128"][1] == (3, 2, 1, 0, 1)
    cfg = scrubjay.scrubjay_infer_config(16000)
    t, rc = M.gen_tables(cfg)
    assert rc == 0 and M.variant_2048(t, cfg) == M.SHAPES_2048["aubio"][1] and t.seg_ok == 1
    for sr, name in ((16000, "librosa128"), (22050, "librosa128_22k_csr")):
        cfg = dsp_amd.default_config(sample_rate=sr, n_fft=2048, frame_length=2048, hop_length=512, n_mels=128, n_mfcc=20, fmin=0.0, fmax=sr / 2.0,
                                     mel_norm=dl.MELNORM_LIBROSA, log_mode=dl.LOG_GLOBAL_REF1)
        t, rc = M.gen_tables(cfg)
        assert rc == 0 and M.variant_2048(t, cfg) == M.SHAPES_2048[name][1] and t.seg_ok == (sr == 16000)


def test_both_literal_prefilters_have_their_own_wave_kernel():
    """M.UNLAUNCHED: launch_mfcc1024_wave's two step patterns cover both literal filters, so the generic six-step form is never launched"""
    L = dsp_amd.load()
    for pre in (dl.PREFILTER_BUTTER_1000_3000, dl.PREFILTER_BUTTER_3000_7500):
        st = (C.c_int * 4)()
        assert L.dsp_prefilter_scan_check(pre, st) == 3
        s = list(st)
        assert (s[0] <= 1 and s[1] <= 3 and s[2] <= 3 and s[3] <= 5) or (s[0] <= 2 and s[1] <= 3 and s[2] <= 3 and s[3] <= 4), s


@pytest.mark.parametrize("name", M.NAMES_1024)
def test_1024_chunks_reproduce_dense_filterbank(name):
    cfg, t = _tables(1024, name)
    k0, w, src = M.arr(t.mel_k0), M.arr(t.mel_w), M.arr(t.mel_src)
    _win, mel, _dct = dsp_amd.tables(cfg)
    assert mel.shape == (cfg.n_mels, 513)
    rec = np.zeros_like(mel)
    used = []
    for m in range(128):
        for g in range(6):
            idx = int(src[m // 64][g][m % 64])
            if idx == M.ZERO_SLOT_1024:
                continue
            assert m < cfg.n_mels and 0 <= idx < 64 * t.n_chunk_slots       # filters past n_mels gather nothing
            used.append(idx)
            slot, lane = divmod(idx, 64)
            rec[m, k0[slot][lane]: k0[slot][lane] + 12] += w[slot][:, lane]
    assert len(set(used)) == len(used), "a chunk is gathered twice"
    assert np.array_equal(rec, mel)
    assert ((k0 >= 0) & (k0 <= 513 - 12)).all()                            # every window, idle ones too, reads inside P[0..512]
    idle = np.ones(256, bool)
    idle[used] = False
    assert not w.transpose(0, 2, 1).reshape(256, 12)[idle].any()            # idle (slot, lane)s carry zero weights
    assert int((~mel.any(axis=1)).sum()) == M.SHAPES_1024[name][1][3]
    assert 1 <= t.n_chunk_slots <= 3 and len(used) > 64 * (t.n_chunk_slots - 1)
    if M.SHAPES_1024[name][1][1] == 6:
        runs = [np.flatnonzero(row)[[0, -1]] for row in mel if row.any()]
        assert max(b - a + 1 for a, b in runs) in range(61, 73)


@pytest.mark.parametrize("name", M.NAMES_2048)
def test_2048_segments_and_csr_rows_reproduce_dense_filterbank(name):
    cfg, t = _tables(2048, name)
    _win, mel, _dct = dsp_amd.tables(cfg)
    assert mel.shape == (cfg.n_mels, 1025)
    lo, ln, off, w = M.arr(t.mel_lo), M.arr(t.mel_len), M.arr(t.mel_off), M.arr(t.mel_w)
    rec = np.zeros_like(mel)
    for m in range(cfg.n_mels):
        assert 0 <= lo[m] and lo[m] + ln[m] <= 1025 and off[m] + ln[m] <= 4096
        rec[m, lo[m]: lo[m] + ln[m]] = w[off[m]: off[m] + ln[m]]
    assert np.array_equal(rec, mel)
    assert int((ln[:cfg.n_mels] == 0).sum()) == int((~mel.any(axis=1)).sum()) == M.SHAPES_2048[name][1][4]
    if not t.seg_ok:
        return
    s0, cnt, k0, sw = M.arr(t.mel_s0), M.arr(t.mel_cnt), M.arr(t.seg_k0), M.arr(t.seg_w)
    assert ((k0 >= 0) & (k0 <= 1025 - 16)).all()                           # every window reads inside P[0..1024]
    rec = np.zeros_like(mel)
    nxt = 0
    for m in range(cfg.n_mels):
        assert s0[m] == nxt and 0 <= cnt[m] <= 12                          # consecutive: the filter's lane adds [s0, s0 + cnt) in ascending order
        for s in range(s0[m], s0[m] + cnt[m]):
            slot, lane = divmod(s, 64)
            rec[m, k0[slot][lane]: k0[slot][lane] + 16] += sw[slot][:, lane]
        nxt += cnt[m]
    assert nxt <= 192 and np.array_equal(rec, mel)
    assert not sw.transpose(0, 2, 1).reshape(192, 16)[nxt:].any()           # segments past the last carry zero weights


@pytest.mark.parametrize("n_fft,name", CASES)
def test_dct_tables(n_fft, name):
    """1024: dct_w, the row split over four neighbouring lanes of 32 mels each, and dct_a, the MFMA A operand (step s, lane l ->
    dct[l % 16][4 s + l / 16]); 2048: dct_t, two lanes per coefficient, half = ceil(n_mels / 2) mels each"""
    cfg, t = _tables(n_fft, name)
    _win, _mel, d = dsp_amd.tables(cfg)
    assert np.array_equal(d, O.dct_ortho(cfg.n_mfcc, cfg.n_mels))
    if n_fft == 1024:
        w, a = M.arr(t.dct_w), M.arr(t.dct_a)
        want_w, want_a = np.zeros_like(w), np.zeros_like(a)
        for c in range(cfg.n_mfcc):
            for m in range(cfg.n_mels):
                want_w[m % 32, 4 * c + m // 32] = d[c, m]
                want_a[m // 4, c + 16 * (m % 4)] = d[c, m]
        assert np.array_equal(w, want_w) and np.array_equal(a, want_a)
    else:
        tt, full = M.arr(t.dct_t), M.arr(t.dct)
        half = (cfg.n_mels + 1) // 2
        want = np.zeros_like(tt)
        for c in range(cfg.n_mfcc):
            for m in range(cfg.n_mels):
                want[m % half, 2 * c + m // half] = d[c, m]
        assert np.array_equal(tt, want)
        want = np.zeros_like(full)
        want[:cfg.n_mfcc, :cfg.n_mels] = d
        assert np.array_equal(full, want)


def _reference_noise(n_fft, name, frame_length, log_mode):
    """the reference-order float32 oracle against the float64-FFT oracle on every input of the GPU tests -> [(what, ok, worst)]"""
    both = lambda fn, *a: frame_linf_close(fn(*a, fft_mode=O.FFT_REFERENCE_ORDER), fn(*a), RTOL)
    out = [("frames",) + both(M.reference_frames, n_fft, name, frame_length, log_mode, M.frames_input(n_fft, name, frame_length))]
    for kind, x in zip(M.CLIP_KINDS, M.clips_input(n_fft, name, frame_length)):
        out.append((f"clip {kind}",) + both(M.reference_clip, n_fft, name, frame_length, log_mode, x))
    if n_fft == 2048:
        buf, off = M.ragged_input(n_fft, name, frame_length)
        for c in range(len(off) - 1):
            x = buf[off[c]:off[c + 1]]
            assert np.isfinite(x).all()
            out.append((f"ragged clip {c}",) + both(M.reference_clip, n_fft, name, frame_length, log_mode, x))
    return out


@pytest.mark.parametrize("n_fft,name", [c for c in CASES if c[1] != "aubio"])
def test_inputs_admit_the_gate(n_fft, name):
    """On every input of the two GPU shape suites the reference's own float32 evaluation is inside the project's pure gate of the float64
    one: the GPU tests' gate then measures the kernel, not the reference's noise.  (The canonical aubio front end's oracle has one
    evaluation, with aubio's float64 transform; its inputs are the ones "stream_only40" passes here.)"""
    misses, worst_of_all = [], 0.0
    for frame_length in M.frame_lengths(n_fft, name):
        for log_mode in (M.log_modes(name) if n_fft == 2048 else (0,)):
            if log_mode == 1 and M.is_stream(n_fft, name):
                continue
            for what, ok, worst in _reference_noise(n_fft, name, frame_length, log_mode):
                worst_of_all = max(worst_of_all, worst)
                if not ok:
                    misses.append((frame_length, log_mode, what, worst))
    print(f"reference float32 against float64 on the inputs of {n_fft} {name}: worst {worst_of_all:.2e} of {RTOL:.0e}")
    assert not misses, misses


def _aubio_float32(frames):
    """the canonical aubio front end on frames[n][2048] with a float32 transform (scipy.fft computes float32 input in single precision):
    what oracle/aubio_oracle.c evaluates with aubio's float64 transform"""
    import scipy.fft
    over = M.SHAPES_2048["aubio"][0]
    v = np.fft.fftshift(frames.astype(np.float32) * O.aubio_window_hanningz(2048), axes=-1)
    spec = scipy.fft.rfft(v, axis=-1)
    assert spec.dtype == np.complex64
    e = np.abs(spec) @ O.aubio_filterbank_slaney(over["sample_rate"], 2048).T
    return (np.log10(np.maximum(e, np.float32(2e-42))) @ O.dct_ortho(over["n_mfcc"], 40).T).astype(np.float32)


def test_aubio_inputs_admit_the_gate():
    """test_inputs_admit_the_gate for "aubio", whose oracle has no float32 mode: a float32 numpy evaluation of the chain is inside the
    pure gate of the oracle on every input of the GPU tests"""
    worst_of_all, misses = 0.0, []
    hop = M.HOPS[2048]
    x = M.frames_input(2048, "aubio", 2048)
    cases = [("frames", x, M.reference_frames(2048, "aubio", 2048, 2, x))]
    buf, off = M.ragged_input(2048, "aubio", 2048)
    clips = list(zip(M.CLIP_KINDS, M.clips_input(2048, "aubio", 2048))) + [(f"ragged clip {c}", buf[off[c]:off[c + 1]]) for c in range(1, 5)]
    for what, clip in clips:
        cases.append((f"clip {what}", M.stream_frames(clip, 2048, hop), M.reference_clip(2048, "aubio", 2048, 2, clip)))
    for what, frames, ref in cases:
        ok, worst = frame_linf_close(_aubio_float32(frames), ref, RTOL)
        worst_of_all = max(worst_of_all, worst)
        if not ok:
            misses.append((what, worst))
    print(f"float32 numpy against the oracle on the inputs of 2048 aubio: worst {worst_of_all:.2e} of {RTOL:.0e}")
    assert not misses, misses


def test_inputs_have_the_edges_the_gpu_tests_name():
    for n_fft, name in ((1024, "htk128"), (2048, "librosa128"), (2048, "stream_only40")):
        for frame_length in M.FRAME_LENGTHS[n_fft]:
            cfg = M.config(n_fft, name, frame_length)
            x = M.frames_input(n_fft, name, frame_length)
            assert x.shape == (67, frame_length) and not x[M.ZERO_ROW].any() and 0 < np.abs(x[M.QUIET_ROW]).max() < 2e-6
            assert M.QUIET_ROW < min(n for n in M.FRAME_ROWS[n_fft] if n > 1)
            clips = M.clips_input(n_fft, name, frame_length)
            frames = dsp_amd.mfcc.frames_for(cfg, clips[0].size, 1000)
            stream = M.is_stream(n_fft, name)
            assert frames == (M.CLIP_FRAMES + (3 if frame_length == 2048 else 2) + 1 if stream else M.CLIP_FRAMES)
            assert (not stream or clips[0].size % M.HOPS[frame_length] != 0) and not clips[2][clips[2].size // 2:].any()
            buf, off = M.ragged_input(n_fft, name, frame_length)
            assert off[0] % 2 == 1 and np.isnan(buf[:off[0]]).all() and np.isnan(buf[off[-1]:]).all()
            assert [dsp_amd.mfcc.frames_for(cfg, int(n), 1000) for n in np.diff(off)] == [0, 1, 2 if stream else 1, 7, 23]


@pytest.mark.parametrize("name", [n for n in M.NAMES_2048 if not M.is_aubio(n)])
def test_the_clip_floor_clips_on_the_third_clip(name):
    """DSP_LOG_GLOBAL_REF1 over clips: the silent half of the third clip lies on the clip's floor, 10 dB or more above amin in every filter"""
    for frame_length in M.FRAME_LENGTHS[2048]:
        x = M.clips_input(2048, name, frame_length)[2]
        ref = M.reference_clip(2048, name, frame_length, 1, x)
        silent = -(-(x.size // 2) // M.HOPS[frame_length])
        n_mels = M.SHAPES_2048[name][0]["n_mels"]
        assert (ref[silent:] == ref[silent]).all() and ref[silent, 0] >= (-100.0 + 10.0) * np.sqrt(n_mels)      # c0 = sqrt(n_mels) x the floor in dB


def _refusal(cfg):
    """the return code and reason of the exporter of cfg.n_fft"""
    L = dsp_amd.load()
    t, fn = (dl.GenTables1024(), L.dsp_mfcc1024_tables) if cfg.n_fft != 2048 else (dl.GenTables2048(), L.dsp_mfcc2048_tables)
    return fn(C.byref(cfg), C.byref(t), C.sizeof(t)), dl.last_error()


@pytest.mark.parametrize("over,reason", [
    (dict(n_fft=1024, n_mels=0), "n_mels and n_mfcc must be positive"), (dict(n_fft=1024, n_mels=129), "n_mels must be in [1, 128]"),
    (dict(n_fft=1024, n_mels=128, n_mfcc=0), "n_mels and n_mfcc must be positive"),
    (dict(n_fft=1024, n_mels=128, n_mfcc=17), "n_mfcc must be in [1, 16] for n_fft = 1024"),
    (dict(n_fft=1024, n_mels=128, log_mode=1), "DSP_LOG_GLOBAL_REF1 is implemented for n_fft = 512 and 2048"),
    (dict(n_fft=1024, n_mels=16, fmax=8000.0), "a mel filter spans more than 72 bins"),
    (dict(n_fft=1024, n_mels=128, frame_length=1026), "frame_length must not exceed n_fft"),
    (dict(n_fft=2048, n_mels=0), "n_mels and n_mfcc must be positive"), (dict(n_fft=2048, n_mels=129), "n_mels must be in [1, 128] for n_fft = 2048"),
    (dict(n_fft=2048, n_mfcc=0), "n_mels and n_mfcc must be positive"), (dict(n_fft=2048, n_mfcc=33), "n_mfcc must be in [1, 32] for n_fft = 2048"),
    (dict(n_fft=2048, prefilter=1), "the per-frame prefilter is implemented for n_fft = 512 and 1024"),
    (dict(n_fft=2048, mel_norm=3, n_mels=41), "DSP_MELNORM_AUBIO_SLANEY is aubio's 40-filter bank: n_mels must be 40"),
])
def test_exporters_refuse_what_plan_create_refuses(over, reason):
    cfg = dsp_amd.default_config(**over)
    rc, why = _refusal(cfg)
    assert rc == -1 and why == reason
    # dsp_mfcc_plan_create refuses the same configuration before it looks at the device, in the same words
    plan = C.c_void_p()
    assert dsp_amd.load().dsp_mfcc_plan_create(C.byref(cfg), 0, C.byref(plan)) == -1 and not plan.value
    assert dl.last_error() == reason


def test_exporters_refuse_the_other_transform_lengths_and_bad_sizes():
    L = dsp_amd.load()
    for n_fft in (400, 512, 1024, 2048, 333):
        cfg = dsp_amd.default_config(n_fft=n_fft, frame_length=min(n_fft, 400) & ~1, n_mels=64)
        for fn, own, t in ((L.dsp_mfcc1024_tables, 1024, dl.GenTables1024()), (L.dsp_mfcc2048_tables, 2048, dl.GenTables2048())):
            rc = fn(C.byref(cfg), C.byref(t), C.sizeof(t))
            assert (rc == 0) == (n_fft == own), (n_fft, own, dl.last_error())
            if rc:
                assert rc == -1 and "n_fft" in dl.last_error()
    t = dl.GenTables1024()
    cfg = dsp_amd.default_config(n_fft=1024, n_mels=128)
    assert L.dsp_mfcc1024_tables(C.byref(cfg), C.byref(t), 12) == -1 and "sizeof(GenTables1024)" in dl.last_error()
    assert L.dsp_mfcc2048_tables(C.byref(cfg), C.byref(t), 12) == -1 and "sizeof(GenTables2048)" in dl.last_error()
    assert L.dsp_mfcc1024_tables(None, None, 0) == -1 and L.dsp_mfcc2048_tables(None, None, 0) == -1
    assert {"dsp_mfcc1024_tables", "dsp_mfcc2048_tables"} <= set(dl.SYMBOLS)
