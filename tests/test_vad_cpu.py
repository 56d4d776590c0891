"""CPU: voice activity detection (include/dsp_amd.h dsp_vad_*, dsp_rows_*) -- the numpy restatement of tests/vad_ref.py
against independent forms of the same definitions, and the host-only entries and every argument refusal through the built library.
No device is touched here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import vad_ref as V
from tests import vad_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAD_SYMBOLS = ["dsp_vad_default_config", "dsp_vad_ratio_from_db", "dsp_vad_geometry_for", "dsp_vad_workspace_bytes", "dsp_vad_frame_power_ragged_device",
               "dsp_vad_decide_ragged_device", "dsp_vad_run_ragged_device", "dsp_rows_kept_offsets_device", "dsp_rows_select_ragged_device",
               "dsp_vad_trim_spans"]
SEEDS = (0, 1, 2, 3)
LP = dl.LP


def _clip(seed, frame_length):
    return U.signal(seed, 30000 + 2003 * seed + frame_length)


_powers = {}


def _power(name, seed):
    """the restatement's P of the shared clip `seed` under framing `name`, computed once"""
    if (name, seed) not in _powers:
        fl, hop, framing = U.FRAMINGS[name]
        _powers[name, seed] = V.frame_power(_clip(seed, fl), fl, hop, framing)
    return _powers[name, seed]


@pytest.mark.parametrize("name", list(U.FRAMINGS))
def test_frame_power_agrees_with_the_mean_of_squares(name):
    """Both sides add N = frame_length non-negative float64 terms, each sum rounded once: N - 1 roundings of relative size 2^-53 on
    each side, so 2 N 2^-53 relative covers any two orders.  Measured where the issue was written: 7.2e-16."""
    fl, hop, framing = U.FRAMINGS[name]
    worst = 0.0
    for seed in SEEDS:
        x = _clip(seed, fl)
        got, plain = _power(name, seed), V.frame_power_plain(x, fl, hop, framing)
        assert got.shape == plain.shape == (V.frames_for(x.size, fl, hop, framing),) and got.size > 20
        rel = np.abs(got - plain) / plain
        worst = max(worst, float(rel.max()))
    print(f"{name}: worst relative difference {worst:.2e}")
    assert worst <= 2 * fl * 2.0 ** -53


def test_geometry_of_the_four_framings():
    assert V.geometry(400, 160, V.CENTER) == (40, 10, 200, 16)
    assert V.geometry(400, 160, V.COMPLETE) == (80, 5, 0, 32)
    assert V.geometry(512, 160, V.COMPLETE) == (32, 16, 0, 8)
    assert V.geometry(2048, 1024, V.STREAM) == (1024, 2, 1024, 64)
    for fl, hop, framing in U.FRAMINGS.values():
        cfg = U.config(fl, hop, framing, context=5, pad=3)
        geo = U.geometry(cfg)
        g, m, _, _ = V.geometry(fl, hop, framing)
        assert (geo.g, geo.m, geo.rows_per_tile, geo.halo_rows, geo.samples_per_tile) == (g, m, V.TILE, 8, (V.TILE - 1) * hop + fl)


def test_decisions_agree_with_the_db_form():
    """10 log10(P / ref) > db against P > ref 10^(db / 10): the two can differ only for a row within rounding of its threshold, and no
    row of the shared cases lies within 1e-9 relative of one -- asserted, so that nothing is left out of the comparison."""
    rows = 0
    for name in U.FRAMINGS:
        for seed in SEEDS:
            P = _power(name, seed)
            ref = P.max()
            for db in (-20.0, -40.0, -60.0):
                ratio = dl.load().dsp_vad_ratio_from_db(db)
                assert ratio == 10.0 ** (db / 10.0)
                flags, rec, raw, _ = V.decide(P, V.REF_MAX, ratio)
                assert rec["reference"] == ref and rec["threshold"] == ref * ratio
                assert not (np.abs(P - rec["threshold"]) <= 1e-9 * rec["threshold"]).any()
                assert np.array_equal(raw, 10.0 * np.log10(P / ref) > db) and np.array_equal(flags, raw.astype(np.uint8))
            rows += P.size
    assert rows > 1500


@pytest.mark.parametrize("context,pad", [(0, 0), (5, 0), (0, 3), (64, 64), (2, 1)])
@pytest.mark.parametrize("proportion", [0.6, 1.0, 0.01])
def test_smoothing_and_hangover_agree_with_a_loop_per_row(context, pad, proportion):
    rng = np.random.default_rng(context * 100 + pad)
    for T in (1, 2, 7, 130, 300):
        for density in (0.1, 0.5, 0.9):
            P = np.where(rng.random(T) < density, 1.0, 1e-9)
            flags, rec, raw, _ = V.decide(P, V.REF_ABSOLUTE, 1e-3, 0.0, context, proportion, pad)
            assert np.array_equal(raw, P > 1e-3)
            want = V.smooth_loop(raw, context, proportion, pad)
            assert np.array_equal(flags.astype(bool), want)
            assert rec["n_raw"] == raw.sum() and rec["n_kept"] == want.sum()
            where = np.flatnonzero(want)
            assert (rec["first_kept"], rec["last_kept"]) == ((where[0], where[-1]) if where.size else (-1, -1))
    if context == 0:
        assert np.array_equal(V.decide(P, V.REF_ABSOLUTE, 1e-3, pad=0, context=0, proportion=proportion)[0], (P > 1e-3).astype(np.uint8))


def test_reference_levels_and_the_strict_comparison():
    P = np.array([0.0, 4.0, np.nan, 1.0, np.inf, 3.0])
    assert V.reference_level(P, V.REF_ABSOLUTE) == 1.0 and V.reference_level(P, V.REF_MAX) == 4.0 and V.reference_level(P, V.REF_MEAN) == 2.0
    empty = np.array([np.nan, np.inf])
    assert V.reference_level(empty, V.REF_MAX) == 0.0 and V.reference_level(empty, V.REF_MEAN) == 0.0
    flags, rec, _, level = V.decide(np.zeros(5), V.REF_MAX, 1e-6)           # an all-zero clip keeps nothing
    assert not flags.any() and rec["threshold"] == 0.0 and rec["n_kept"] == 0 and np.isnan(level).all()
    flags, rec, _, _ = V.decide(P, V.REF_MAX, 0.5, floor=3.0)                # the floor wins over 4 * 0.5; NaN and inf are never speech
    assert rec["threshold"] == 3.0 and flags.tolist() == [0, 1, 0, 0, 0, 0]
    rng = np.random.default_rng(5)
    big = rng.random(1000)
    assert abs(V.reference_level(big, V.REF_MEAN) - big.mean()) <= 1000 * 2.0 ** -53


def test_the_library_exports_the_entries_and_states_them_in_the_header():
    L = dsp_amd.load()
    header = open(os.path.join(ROOT, "include", "dsp_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", dsp_amd.build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in VAD_SYMBOLS:
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported and re.search(r"\b%s\(" % name, header), name
    assert [n for n in dl.SYMBOLS if n.startswith("dsp_vad") or n.startswith("dsp_rows")] == VAD_SYMBOLS
    assert "capi_vad.cpp" in dsp_amd.build.SOURCES and "vad_kernels.hip" in dsp_amd.build.SOURCES and "vad_kernels.hpp" in dsp_amd.build.HEADERS
    assert C.sizeof(dl.VadConfig) == 56 and C.sizeof(dl.VadGeometry) == 20 and np.dtype(dl.VAD_CLIP_DTYPE).itemsize == 32
    assert np.dtype(dl.VAD_CLIP_DTYPE) == V.CLIP_DTYPE


def test_default_config_and_ratio_from_db():
    L = dsp_amd.load()
    cfg = dl.VadConfig()
    L.dsp_vad_default_config(C.byref(dsp_amd.speaker_config()), C.byref(cfg))
    assert (cfg.frame_length, cfg.hop_length, cfg.framing) == (400, 160, dl.FRAMING_CENTER)
    assert (cfg.reference, cfg.threshold_ratio, cfg.floor_power, cfg.context_frames, cfg.proportion, cfg.pad_frames) == (dl.VAD_REF_MAX, 1e-6, 0.0, 0, 0.6, 0)
    L.dsp_vad_default_config(C.byref(dsp_amd.default_config()), C.byref(cfg))
    assert (cfg.frame_length, cfg.hop_length, cfg.framing) == (400, 160, dl.FRAMING_COMPLETE)
    assert L.dsp_vad_ratio_from_db(-60.0) == 1e-6 and L.dsp_vad_ratio_from_db(0.0) == 1.0 and L.dsp_vad_ratio_from_db(float("-inf")) == 0.0
    assert L.dsp_vad_workspace_bytes(0, 0) > 0 and L.dsp_vad_workspace_bytes(10, 5000) >= 5000 * 8
    assert L.dsp_vad_workspace_bytes(-1, 0) == -1 and "n_clips" in dl.last_error()


BAD_CONFIGS = [
    (dict(hop=0), "hop_length must be >= 1"),
    (dict(frame_length=4097, hop=4097), "frame_length must be 1 .. 4096"),
    (dict(frame_length=0), "frame_length must be 1 .. 4096"),
    (dict(framing=3), "framing must be a DSP_FRAMING_"),
    (dict(frame_length=401, hop=160, framing=V.CENTER), "needs an even frame_length"),
    (dict(frame_length=400, hop=401, framing=V.STREAM), "needs hop_length <= frame_length"),
    (dict(frame_length=400, hop=3), "must be <= 64 sub-blocks per frame, got 400"),
    (dict(frame_length=650, hop=10, framing=V.COMPLETE), "must be <= 64 sub-blocks per frame, got 65"),
    (dict(reference=3), "reference must be"),
    (dict(ratio=-1.0), "threshold_ratio must be finite and >= 0"),
    (dict(ratio=float("inf")), "threshold_ratio must be finite and >= 0"),
    (dict(ratio=float("nan")), "threshold_ratio must be finite and >= 0"),
    (dict(floor=-1.0), "floor_power must be >= 0"),
    (dict(floor=float("nan")), "floor_power must be >= 0"),
    (dict(context=-1), "context_frames must be 0 .. 64"),
    (dict(context=65), "context_frames must be 0 .. 64"),
    (dict(pad=65), "pad_frames must be 0 .. 64"),
    (dict(proportion=0.0), "proportion must lie in (0, 1]"),
    (dict(proportion=1.5), "proportion must lie in (0, 1]"),
    (dict(proportion=float("nan")), "proportion must lie in (0, 1]"),
]


def _cfg(**over):
    base = dict(frame_length=400, hop=160, framing=V.CENTER)
    base.update(over)
    return U.config(**base)


@pytest.mark.parametrize("over,message", BAD_CONFIGS)
def test_a_bad_config_is_refused_by_every_entry_that_takes_one(over, message):
    L = dsp_amd.load()
    cfg = _cfg(**over)
    geo = dl.VadGeometry()
    off, fo, ko = (C.c_long * 2)(0, 1000), (C.c_long * 2)(0, 7), (C.c_long * 2)()
    calls = [lambda: L.dsp_vad_geometry_for(C.byref(cfg), C.byref(geo)),
             lambda: L.dsp_vad_frame_power_ragged_device(0, C.byref(cfg), 256, 1, off, fo, 256, 256, 1 << 20, None),
             lambda: L.dsp_vad_decide_ragged_device(0, C.byref(cfg), 256, 1, fo, 256, None, None, ko, 256, 1 << 20, None),
             lambda: L.dsp_vad_run_ragged_device(0, C.byref(cfg), 256, 1, off, fo, 256, None, None, ko, 256, 1 << 20, None),
             lambda: L.dsp_vad_trim_spans(C.byref(cfg), off, 1, 256, None, None)]
    for call in calls:
        assert call() == -1 and message in dl.last_error(), dl.last_error()
    assert L.dsp_vad_geometry_for(None, C.byref(geo)) == -1 and "dsp_vad_config is NULL" in dl.last_error()
    assert L.dsp_vad_geometry_for(C.byref(_cfg()), None) == -1 and "out is NULL" in dl.last_error()


def test_the_ragged_entries_refuse_their_arguments_before_a_device_is_touched():
    """every pointer below that is not NULL is the bogus address 256: a call that got as far as a launch would not return -1"""
    L = dsp_amd.load()
    cfg, p, big = _cfg(), 256, 1 << 20
    off = (C.c_long * 4)(0, 1000, 1000, 1700)
    fo = (C.c_long * 4)(0, 7, 7, 12)            # 1 + n // 160 rows: 7, 0 (legal: fewer than the 1 its length gives... it has none), 5
    ko = (C.c_long * 4)()

    def refused(rc, message):
        assert rc == -1 and message in dl.last_error(), (rc, dl.last_error())

    run = L.dsp_vad_run_ragged_device
    refused(run(-1, C.byref(cfg), p, 3, off, fo, p, None, None, ko, p, big, None), "device index out of range")
    refused(run(0, C.byref(cfg), p, -1, off, fo, p, None, None, ko, p, big, None), "n_clips < 0")
    refused(run(0, C.byref(cfg), p, 1 << 31, off, fo, p, None, None, ko, p, big, None), "2^31 clips or more")
    refused(run(0, C.byref(cfg), p, 3, off, fo, p, None, None, None, p, big, None), "kept_offsets is NULL")
    refused(run(0, C.byref(cfg), p, 3, None, fo, p, None, None, ko, p, big, None), "offsets is NULL")
    refused(run(0, C.byref(cfg), p, 3, off, None, p, None, None, ko, p, big, None), "frame_offsets is NULL")
    refused(run(0, C.byref(cfg), p, 3, off, (C.c_long * 4)(0, 7, 6, 12), p, None, None, ko, p, big, None), "frame_offsets decrease at clip 1")
    refused(run(0, C.byref(cfg), p, 3, (C.c_long * 4)(0, 1000, 900, 1700), fo, p, None, None, ko, p, big, None), "(clip 1)")
    refused(run(0, C.byref(cfg), p, 3, off, (C.c_long * 4)(0, 7, 7, 13), p, None, None, ko, p, big, None), "clip 2 brings 6 rows, its 700 samples give 5")
    refused(run(0, C.byref(cfg), None, 3, off, fo, p, None, None, ko, p, big, None), "d_signal is NULL")
    refused(run(0, C.byref(cfg), p, 3, off, fo, None, None, None, ko, p, big, None), "d_flags is NULL")
    refused(run(0, C.byref(cfg), p, 3, off, fo, p, None, None, ko, None, big, None), "d_workspace is NULL")
    refused(run(0, C.byref(cfg), p, 3, off, fo, p, None, None, ko, 260, big, None), "d_workspace must be 256-byte aligned")
    refused(run(0, C.byref(cfg), p, 3, off, fo, p, None, None, ko, p, 100, None), "d_workspace holds 100 bytes, the call needs")
    assert run(0, C.byref(cfg), p, 3, off, (C.c_long * 4)(0, 6, 6, 10), p, None, None, ko, p, 100, None) == -1      # fewer rows (a cap) pass the row check
    assert "d_workspace holds" in dl.last_error()
    power, decide = L.dsp_vad_frame_power_ragged_device, L.dsp_vad_decide_ragged_device
    refused(power(0, C.byref(cfg), p, 3, off, fo, None, p, big, None), "d_power is NULL")
    refused(power(0, C.byref(cfg), p, 3, off, (C.c_long * 4)(0, 8, 8, 12), p, p, big, None), "clip 0 brings 8 rows")
    refused(decide(0, C.byref(cfg), None, 3, fo, p, None, None, ko, p, big, None), "d_power is NULL")
    refused(decide(0, C.byref(cfg), p, 3, fo, None, None, None, ko, p, big, None), "d_flags is NULL")
    refused(decide(0, C.byref(cfg), p, 3, fo, p, None, None, None, p, big, None), "kept_offsets is NULL")
    # zero clips and clips without rows: DSP_OK, kept_offsets zeroed, nothing launched
    ko[0] = ko[1] = ko[2] = ko[3] = 77
    assert run(0, C.byref(cfg), None, 0, None, None, None, None, None, ko, None, 0, None) == 0 and ko[0] == 0 and ko[1] == 77
    assert run(0, C.byref(cfg), None, 3, (C.c_long * 4)(0, 0, 0, 0), (C.c_long * 4)(5, 5, 5, 5), None, None, None, ko, None, 0, None) == 0 and list(ko) == [0] * 4
    assert power(0, C.byref(cfg), None, 0, None, None, None, None, 0, None) == 0
    kept, select = L.dsp_rows_kept_offsets_device, L.dsp_rows_select_ragged_device
    refused(kept(-1, p, 3, fo, ko, p, big, None), "device index out of range")
    refused(kept(0, p, 3, fo, None, p, big, None), "kept_offsets is NULL")
    refused(kept(0, p, 3, None, ko, p, big, None), "frame_offsets is NULL")
    refused(kept(0, None, 3, fo, ko, p, big, None), "d_flags is NULL")
    refused(kept(0, p, 3, fo, ko, p, 10, None), "d_workspace holds 10 bytes")
    assert kept(0, None, 0, None, ko, None, 0, None) == 0 and kept(0, None, 2, (C.c_long * 3)(4, 4, 4), ko, None, 0, None) == 0 and list(ko)[:3] == [0] * 3
    good = (C.c_long * 4)(0, 3, 3, 8)
    for d in (0, 65):
        refused(select(0, p, d, p, 3, fo, good, p, None, p, big, None), f"d must be 1 .. 64, got {d}")
    refused(select(0, p, 13, p, 3, fo, None, p, None, p, big, None), "kept_offsets is NULL")
    refused(select(0, p, 13, p, 3, fo, (C.c_long * 4)(1, 3, 3, 8), p, None, p, big, None), "kept_offsets must start at 0")
    refused(select(0, p, 13, p, 3, fo, (C.c_long * 4)(0, 3, 2, 8), p, None, p, big, None), "kept_offsets decrease at clip 1")
    refused(select(0, p, 13, p, 3, fo, (C.c_long * 4)(0, 3, 4, 8), p, None, p, big, None), "kept_offsets give clip 1 more rows than it has")
    refused(select(0, None, 13, p, 3, fo, good, p, None, p, big, None), "d_in is NULL")
    refused(select(0, p, 13, None, 3, fo, good, p, None, p, big, None), "d_flags is NULL")
    refused(select(0, p, 13, p, 3, fo, good, None, None, p, big, None), "d_out is NULL")
    refused(select(0, 4096, 13, p, 3, fo, good, 4096, None, p, big, None), "d_out overlaps the rows of d_in")
    refused(select(0, 4096, 13, p, 3, fo, good, 4096 + 12 * 13 * 4 - 4, None, p, big, None), "d_out overlaps the rows of d_in")
    refused(select(0, 4096, 13, p, 3, fo, good, 4096 + 12 * 13 * 4, None, None, big, None), "d_workspace is NULL")     # (adjacent is no overlap)
    assert select(0, None, 13, None, 0, None, None, None, None, None, 0, None) == 0
    assert select(0, None, 13, None, 3, fo, (C.c_long * 4)(0, 0, 0, 0), None, None, None, 0, None) == 0                # nothing kept: nothing to do


def test_trim_spans_against_the_restatement():
    L = dsp_amd.load()
    cfg = _cfg()
    offsets = np.array([10, 1010, 1010, 5010, 5170], np.int64)
    rec = np.zeros(4, V.CLIP_DTYPE)
    rec["n_kept"], rec["first_kept"], rec["last_kept"] = [3, 0, 26, 1], [2, -1, 0, 1], [5, -1, 25, 1]
    starts, lengths = np.zeros(4, np.int64), np.zeros(4, np.int64)
    n = L.dsp_vad_trim_spans(C.byref(cfg), offsets.ctypes.data_as(LP), 4, rec.ctypes.data, starts.ctypes.data_as(LP), lengths.ctypes.data_as(LP))
    want = V.trim_spans(rec, offsets, 160)
    assert n == want[2] == 3 and np.array_equal(starts, want[0]) and np.array_equal(lengths, want[1])
    assert starts.tolist() == [10 + 320, 1010, 1010, 5010 + 160] and lengths.tolist() == [640, 0, 4000, 0]      # cut at the clip's end; a row past it is empty
    assert L.dsp_vad_trim_spans(C.byref(cfg), offsets.ctypes.data_as(LP), 4, rec.ctypes.data, None, None) == 3
    assert L.dsp_vad_trim_spans(C.byref(cfg), None, 0, None, None, None) == 0
    assert L.dsp_vad_trim_spans(C.byref(cfg), None, 4, rec.ctypes.data, None, None) == -1 and "must not be NULL" in dl.last_error()
    rec["last_kept"][0] = 1
    assert L.dsp_vad_trim_spans(C.byref(cfg), offsets.ctypes.data_as(LP), 4, rec.ctypes.data, None, None) == -1 and "clip 0" in dl.last_error()


def test_the_python_class_checks_its_arguments_without_a_device():
    with dsp_amd.Vad(dsp_amd.speaker_config(), threshold_db=-40.0, floor_db=-90.0, context_frames=5, pad_frames=3) as v:
        assert isinstance(v, dl.Closing) and not isinstance(v, dl.Handle)
        assert v.geometry == {"g": 40, "m": 10, "samples_per_tile": 255 * 160 + 400, "rows_per_tile": 256, "halo_rows": 8}
        assert v.cfg.threshold_ratio == 10.0 ** -4 and v.cfg.floor_power == 10.0 ** -9 and v.cfg.reference == dl.VAD_REF_MAX
        rec = np.zeros(2, V.CLIP_DTYPE)
        rec["n_kept"], rec["first_kept"], rec["last_kept"] = [2, 0], [1, -1], [2, -1]
        starts, lengths, n = v.trim_spans(rec, [0, 1000, 2000])
        assert n == 1 and starts.tolist() == [160, 1000] and lengths.tolist() == [320, 0]
        with pytest.raises(ValueError, match="one entry per clip"):
            v.trim_spans(rec, [0, 1000])
        with pytest.raises(ValueError, match="signal must be a float32 CUDA tensor"):
            v.run(np.zeros(10, np.float32), [0, 10], [0, 1])
    with pytest.raises(dl.DspError, match="the Vad is closed"):
        v.trim_spans(rec, [0, 1000, 2000])
    assert dsp_amd.Vad(dsp_amd.default_config(), reference="mean").cfg.reference == dl.VAD_REF_MEAN
    for bad, message in ((dict(reference="median"), "reference must be"), (dict(context_frames=65), "must be 0 .. 64"), (dict(pad_frames=-1), "must be 0 .. 64"),
                         (dict(proportion=0.0), "proportion"), (dict(threshold_db=float("nan")), "threshold_db"), (dict(device=-1), "device index")):
        with pytest.raises(ValueError, match=message):
            dsp_amd.Vad(dsp_amd.speaker_config(), **bad)
    with pytest.raises(ValueError, match="MfccPlan or an MfccConfig"):
        dsp_amd.Vad(400)
    with pytest.raises(ValueError, match="sub-blocks per frame"):
        dsp_amd.Vad(dsp_amd.default_config(frame_length=400, hop_length=3))


@pytest.mark.skipif(__import__("shutil").which("gcc") is None, reason="no gcc")
def test_c_caller_links_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/main_vad.c, built with gcc against include/dsp_amd.h and libdsp_amd.so as its header comment shows"""
    import torch
    from tests import enroll_util
    dsp_amd.load()
    libdir, exe = os.path.join(ROOT, "dsp_amd"), str(tmp_path / "main_vad")
    cmd = ["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
           os.path.join(ROOT, "examples", "main_vad.c"), f"-L{libdir}", "-ldsp_amd", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    wav = str(tmp_path / "a.wav")
    enroll_util.write_wav(wav, (U.signal(0, 16000) * 32767.0).astype(np.int16))
    enroll_util.write_wav(str(tmp_path / "b.wav"), np.zeros(100, np.int16), rate=8000)
    r = subprocess.run([exe, str(tmp_path / "b.wav")], capture_output=True, text=True)
    assert r.returncode == 1 and "not a 16-bit mono PCM WAV at 16 kHz" in r.stderr
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-t", "-30", wav], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and ("no HIP device" in r.stderr or "hipMalloc" in r.stderr)      # loud, no CPU fallback
