"""CPU: every named configuration of tests/mfcc512_shapes.py against the host table builder (build_lane_tables_512, tables.cpp, through
dsp_mfcc_lane_tables) -- the variant each name selects, the sparse mel chunks against the dense bank, the two DCT layouts for every
(dct_split, dct_len) -- and the oracle's own float32 noise on the inputs the GPU shape tests use, so that their gate is a statement
about the kernel."""
import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from oracle import oracle as O
from tests import mfcc512_shapes as M
from tests.conftest import RTOL, frame_linf_close


def _tables(name, **more):
    cfg = dsp_amd.default_config(**dict(M.SHAPES[name][0], **more))
    t, rc = M.lane_tables(cfg)
    assert rc == 0, dl.last_error()
    return cfg, t


@pytest.mark.parametrize("name", M.NAMES)
def test_name_selects_its_variant(name):
    cfg, t = _tables(name)
    assert M.variant_of(t) == M.SHAPES[name][1]
    assert (t.n_mels, t.n_mfcc) == (cfg.n_mels, cfg.n_mfcc)
    # the frame length and the log mode choose FLEN and the epilogue, never the tables' shape
    for frame_length in M.FRAME_LENGTHS:
        for log_mode in M.LOG_MODES:
            t2, rc = M.lane_tables(M.config(name, frame_length, log_mode))
            assert rc == 0 and M.variant_of(t2) == M.SHAPES[name][1]


def test_names_cover_every_instantiation():
    variants = [v for _over, v in M.SHAPES.values()]
    for shape in M.KERNEL_SHAPES:
        for conflict_free in (0, 1):
            assert any(v[:3] == shape and v[3] == conflict_free for v in variants), (shape, conflict_free)
    assert any(v[4] > 0 for v in variants), "no name with an empty filter"
    assert len(M.NAMES) <= 14


@pytest.mark.parametrize("name", M.NAMES)
def test_mel_chunks_reproduce_dense_filterbank(name):
    """tests/test_planner_cpu.py's check on every name, against dsp_amd.tables(cfg)'s dense bank"""
    cfg, t = _tables(name)
    k0 = np.array(t.mel_k0[:])
    w = np.array([list(t.mel_w[i]) for i in range(12)])
    src = np.array([list(t.mel_src[g]) for g in range(6)])
    _win, mel, _dct = dsp_amd.tables(cfg)
    assert mel.shape == (cfg.n_mels, 257)
    rec = np.zeros_like(mel)
    used = []
    for m in range(cfg.n_mels):
        for g in range(6):
            lane = src[g][m]
            if lane == 64:      # zero slot
                continue
            assert g < t.mel_gather and 0 <= lane < 64
            used.append(lane)
            assert 0 <= k0[lane] <= 257 - 12       # every read stays inside P[0..256]
            for i in range(12):
                rec[m, k0[lane] + i] += w[i][lane]
    assert len(set(used)) == len(used), "a lane is used twice"
    assert np.array_equal(rec, mel)
    assert int((~mel.any(axis=1)).sum()) == M.SHAPES[name][1][4]
    assert (src[:, cfg.n_mels:] == 64).all()        # lanes past n_mels gather nothing
    assert t.mel_gather in (3, 6) and (t.mel_gather == 6) == bool((src[3:] != 64).any())
    for lane in set(range(64)) - set(used):
        assert not w[:, lane].any()                 # idle lanes carry zero weights
        assert 0 <= k0[lane] <= 257 - 12            # and still read inside P
    # ds_read_b32: lanes 0-31 and 32-63 are served separately over 32 banks
    distinct = all(len(set(half % 32)) == 32 for half in (k0[:32], k0[32:]))
    assert distinct == (t.mel_conflict_free == 1)


@pytest.mark.parametrize("name", M.NAMES)
def test_dct_tables(name):
    """dct_w: the n_mels-long dot product split over dct_split neighbouring lanes; dct_a: the MFMA A operand of the tile epilogue,
    coefficient tile ct, k-step s, lane l -> dct[16 ct + l % 16][4 s + l / 16]"""
    cfg, t = _tables(name)
    split, length = t.dct_split, t.dct_len
    assert split == (4 if cfg.n_mfcc <= 16 else 2) and split * length >= cfg.n_mels
    _win, _mel, d = dsp_amd.tables(cfg)
    assert np.array_equal(d, O.dct_ortho(cfg.n_mfcc, cfg.n_mels))
    w = np.array([list(t.dct_w[i]) for i in range(20)])
    want = np.zeros_like(w)
    for c in range(cfg.n_mfcc):
        for q in range(split):
            for i in range(length):
                m = q * length + i
                if m < cfg.n_mels:
                    want[i, split * c + q] = d[c, m]
    assert np.array_equal(w, want)
    a = np.array([[list(t.dct_a[ct][s]) for s in range(16)] for ct in range(2)])
    want = np.zeros_like(a)
    for ct in range(2):
        for s in range(16):
            for l in range(64):
                c, m = 16 * ct + l % 16, 4 * s + l // 16
                if c < cfg.n_mfcc and m < cfg.n_mels:
                    want[ct, s, l] = d[c, m]
    assert np.array_equal(a, want)
    assert a[0].any() and a[1].any() == (cfg.n_mfcc > 16)


def _reference_noise(name, frame_length, log_mode):
    """the reference-order float32 oracle against the float64-FFT oracle on every input of the GPU tests -> [(what, ok, worst)]"""
    c32 = M.oracle_cfg(name, frame_length, log_mode, fft_mode=O.FFT_REFERENCE_ORDER)
    c64 = M.oracle_cfg(name, frame_length, log_mode)
    out = []
    for n in (1, 17, 67):
        x = M.frames_input(name, frame_length, n)
        out.append((f"frames n{n}",) + frame_linf_close(O.mfcc_frames(x, c32), O.mfcc_frames(x, c64), RTOL))
    for kind, x in zip(M.CLIP_KINDS, M.clips_input(name, frame_length)):
        out.append((f"clip {kind}",) + frame_linf_close(O.compute_mfcc(x, 1000, c32), O.compute_mfcc(x, 1000, c64), RTOL))
    buf, off = M.ragged_input(name, frame_length)
    for c in range(len(off) - 1):
        x = buf[off[c]:off[c + 1]]
        assert np.isfinite(x).all()
        out.append((f"ragged clip {c}",) + frame_linf_close(O.compute_mfcc(x, 1000, c32), O.compute_mfcc(x, 1000, c64), RTOL))
    return out


@pytest.mark.parametrize("name", M.NAMES)
def test_inputs_admit_the_gate(name):
    """On every input of tests/test_gpu_mfcc512_shapes.py the reference's own float32 evaluation is inside the project's pure gate
    of the float64 one: the GPU tests' gate then measures the kernel, not the reference's noise."""
    misses = []
    for frame_length in M.FRAME_LENGTHS:
        for log_mode in M.LOG_MODES:
            for what, ok, worst in _reference_noise(name, frame_length, log_mode):
                if not ok:
                    misses.append((frame_length, log_mode, what, worst))
    assert not misses, misses


def test_inputs_have_the_edges_the_gpu_tests_name():
    for frame_length in M.FRAME_LENGTHS:
        x = M.frames_input("default", frame_length, 67)
        assert x.shape == (67, frame_length) and not x[33].any() and 0 < np.abs(x[5]).max() < 2e-6
        clips = M.clips_input("default", frame_length)
        assert all(c.size == frame_length + 18 * M.HOP for c in clips) and not clips[2][clips[2].size // 2:].any()
        buf, off = M.ragged_input("default", frame_length)
        assert off[0] % 2 == 1 and np.isnan(buf[:off[0]]).all() and np.isnan(buf[off[-1]:]).all()
        frames = [dsp_amd.mfcc.frames_for(M.config("default", frame_length), int(n), 1000) for n in np.diff(off)]
        assert frames == [0, 1, 1, 7, 23]
