"""GPU: host batches streamed through the host pipeline (dsp_amd/csrc/host_pipe.hpp) -- every *_host entry with the chunk size forced
small through dsp_host_pipeline_set, against the device entry on the same samples, bit for bit: the cuts between chunks, the ring's
depth and the input path (pageable numpy staged, registered or handed over as it is; a pinned tensor) must be invisible in the results and visible in
dsp_host_pipeline_stats.  Shapes are the smallest that hit every boundary: odd clip lengths (the even-stride packing), a short last
chunk, empty clips, clips below / of exactly one frame, a clip longer than a chunk.  Nothing here looks at the clock."""
import ctypes as C

import numpy as np
import pytest

from tests import signals as S

pytestmark = pytest.mark.gpu

MAX_FRAMES = 50
STAGE, REGISTER, DIRECT, WHOLE = 0, 1, 2, 3          # DSP_HOST_PAGEABLE_*: what a call does with a pageable batch larger than a chunk


@pytest.fixture(scope="module")
def dsp():
    import dsp_amd
    return dsp_amd


@pytest.fixture
def pipeline(dsp):
    """host_pipeline(0, ...) for the test, the defaults back when it ends"""
    try:
        yield lambda **kw: dsp.host_pipeline(0, **kw)
    finally:
        dsp.host_pipeline(0)


def _cuda_rows(x, pad_to):
    """host [n][s](...) -> the same rows on the GPU at a row stride of pad_to samples (the device entries want an even stride)"""
    import torch
    buf = torch.zeros((x.shape[0], pad_to) + x.shape[2:], dtype=torch.from_numpy(x).dtype, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf[:, :x.shape[1]]


def _pinned(x):
    import torch
    t = torch.tensor(x).pin_memory()                      # (a copy of its own: the fixtures' arrays are read-only)
    assert t.is_pinned()
    return t


@pytest.fixture(scope="module")
def clips37(dsp):
    """37 clips of 999 samples, T = 4 frames each, and what dsp_mfcc_clips_device makes of them"""
    x = np.stack([S.uniform_pm1(999, 500 + i) * np.float32(0.1 + 0.02 * i) for i in range(37)]).astype(np.float32)
    with dsp.MfccPlan() as plan:
        ref = plan.clips(_cuda_rows(x, 1000), MAX_FRAMES).cpu().numpy()
    assert ref.shape == (37, 4, 13) and np.isfinite(ref).all() and np.abs(ref).max() > 1
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("depth", [1, 3])
def test_mfcc_clips_in_eight_chunks(dsp, pipeline, clips37, depth):
    x, ref = clips37
    with dsp.MfccPlan() as plan:
        dsp.host_pipeline_release(0)                              # a ring that has held nothing larger than this test's chunks
        pipeline(chunk_bytes=5 * 1000 * 4, depth=depth, pageable_mode=STAGE)           # 5 clips at the even stride of 1000 floats: 7 chunks of 5 and one of 2
        for source, path in ((x, "staged"), (_pinned(x), "pinned")):
            got = plan.clips_host(source, MAX_FRAMES)
            assert np.array_equal(got, ref), path
            st = dsp.host_pipeline_stats(0)
            assert (st["n_chunks"], st["depth"], st["input_path"], st["output_path"]) == (8, depth, path, "staged"), st
            assert st["bytes_h2d"] == x.nbytes and st["bytes_d2h"] == ref.nbytes
            # staging is bounded by depth x chunk (input + its slack of 256 bytes, output), not by the batch
            assert 0 < st["peak_staging_bytes"] <= depth * (5 * 1000 * 4 + 256 + 5 * 4 * 13 * 4) < x.nbytes
            assert (st["pinned_ring_bytes"] > 0) and st["pinned_ring_bytes"] <= depth * (5 * 1000 * 4 + 5 * 4 * 13 * 4)
        # the other ways for pageable arrays: page-locked for the call (where the runtime refuses, the input goes the next way and the
        # output through the ring); handed to the runtime's own copy chunk by chunk; and the default: a pageable batch is not cut
        for mode, chunks, paths in ((REGISTER, 8, ("registered", "direct")), (DIRECT, 8, ("direct",)), (WHOLE, 1, ("direct",))):
            pipeline(chunk_bytes=5 * 1000 * 4, depth=depth, pageable_mode=mode)
            assert np.array_equal(plan.clips_host(x.copy(), MAX_FRAMES), ref), mode
            st = dsp.host_pipeline_stats(0)
            assert st["n_chunks"] == chunks and st["input_path"] in paths and st["output_path"] in ("registered", "staged", "direct"), st
        assert np.array_equal(plan.clips_host(_pinned(x), MAX_FRAMES), ref)       # (a pinned batch is cut under every mode)
        assert dsp.host_pipeline_stats(0)["n_chunks"] == 8
        pipeline()
        assert dsp.host_pipeline(0)[2] == WHOLE                   # what the defaults do with pageable arrays


def test_mfcc_clips_in_one_chunk_and_from_pinned_memory_both_ways(dsp, pipeline, clips37):
    x, ref = clips37
    L = dsp.load()
    with dsp.MfccPlan() as plan:
        assert np.array_equal(plan.clips_host(x, MAX_FRAMES), ref)                      # the defaults: one chunk, one pass
        st = dsp.host_pipeline_stats(0)
        assert (st["n_chunks"], st["depth"], st["input_path"], st["output_path"]) == (1, 1, "direct", "direct"), st      # the arrays as they are
        assert np.array_equal(plan.clips_host(_pinned(x), MAX_FRAMES), ref)
        assert dsp.host_pipeline_stats(0)["n_chunks"] == 1
        assert np.array_equal(plan.clips_host(x[0], MAX_FRAMES), ref[:1])               # a single clip
        # dsp_host_alloc: input and output pinned, nothing staged on either side
        p_in, p_out = C.c_void_p(), C.c_void_p()
        assert L.dsp_host_alloc(0, x.nbytes, C.byref(p_in)) == 0 and L.dsp_host_alloc(0, ref.nbytes, C.byref(p_out)) == 0
        try:
            C.memmove(p_in, x.ctypes.data, x.nbytes)
            pipeline(chunk_bytes=5 * 1000 * 4, depth=2, pageable_mode=STAGE)
            assert L.dsp_mfcc_clips_host(plan._h, p_in, 37, 999, 999, p_out, MAX_FRAMES) == 4
            got = np.frombuffer((C.c_char * ref.nbytes).from_address(p_out.value), np.float32).reshape(ref.shape)
            assert np.array_equal(got, ref)
            st = dsp.host_pipeline_stats(0)
            assert (st["n_chunks"], st["depth"], st["input_path"], st["output_path"]) == (8, 2, "pinned", "pinned"), st
        finally:
            L.dsp_host_free(p_in)
            L.dsp_host_free(p_out)


def test_mfcc_frames_in_chunks_of_96(dsp, pipeline):
    import torch
    x = np.stack([S.uniform_pm1(512, 700 + i) for i in range(1000)]).astype(np.float32) * np.float32(0.3)
    with dsp.MfccPlan(dsp.default_config(frame_length=512)) as plan:
        ref = plan.frames(torch.from_numpy(x).cuda()).cpu().numpy()
        pipeline(chunk_bytes=96 * 512 * 4, depth=2, pageable_mode=STAGE)
        for source, path in ((x, "staged"), (_pinned(x), "pinned")):
            assert np.array_equal(plan.frames_host(source), ref), path
            st = dsp.host_pipeline_stats(0)
            assert (st["n_chunks"], st["depth"], st["input_path"]) == (11, 2, path), st      # 10 chunks of 96 frames and one of 40
        pipeline()
        assert np.array_equal(plan.frames_host(x), ref) and dsp.host_pipeline_stats(0)["n_chunks"] == 1


@pytest.mark.parametrize("channels,stereo_mode", [(1, 0), (2, 0), (2, 1)], ids=["mono", "stereo_channel0", "stereo_average"])
def test_mfcc_clips_pcm16_host(dsp, pipeline, channels, stereo_mode):
    rng = np.random.default_rng(31 + channels + stereo_mode)
    pcm = rng.integers(-20000, 20000, (37, 999) + ((2,) if channels == 2 else ()), dtype=np.int16)
    with dsp.MfccPlan() as plan:
        ref = plan.clips_pcm16(_cuda_rows(pcm, 1000), MAX_FRAMES, stereo_mode).cpu().numpy()
        assert ref.shape == (37, 4, 13)
        pipeline(chunk_bytes=5 * 1000 * 2 * channels, depth=3, pageable_mode=STAGE)
        for source, path in ((pcm, "staged"), (_pinned(pcm), "pinned")):
            assert np.array_equal(plan.clips_pcm16_host(source, MAX_FRAMES, stereo_mode), ref), path
            st = dsp.host_pipeline_stats(0)
            assert (st["n_chunks"], st["input_path"], st["bytes_h2d"]) == (8, path, pcm.nbytes), st
        pipeline()
        assert np.array_equal(plan.clips_pcm16_host(pcm, MAX_FRAMES, stereo_mode), ref) and dsp.host_pipeline_stats(0)["n_chunks"] == 1
        if channels == 1:
            with pytest.raises(dsp.DspError, match="channels must be 1 or 2"):
                dsp.lib.check(dsp.load().dsp_mfcc_clips_pcm16_host(plan._h, pcm.ctypes.data, 37, 999, 999, 3, 0, None, MAX_FRAMES), "dsp_mfcc_clips_pcm16_host")


# clip lengths of the ragged batches: none, below one frame, exactly one frame, odd ones, and one clip longer than a chunk of 16 KiB
# (4096 floats, 8192 int16 samples); the batch starts at an odd sample, so that no clip start is aligned by accident
RAGGED_LENGTHS = [1600, 0, 399, 400, 9000, 0, 0, 1234, 2001, 777, 0, 3000, 401, 559, 560, 1, 4096, 0]
RAGGED_OFFSETS = np.concatenate([[3], RAGGED_LENGTHS]).cumsum()


@pytest.mark.parametrize("kind", ["float", "pcm16", "pcm16_stereo_average", "speaker_float"])
def test_mfcc_clips_ragged_host(dsp, pipeline, kind):
    import torch
    total = int(RAGGED_OFFSETS[-1]) + 5
    if kind.startswith("pcm16"):
        shape = (total, 2) if "stereo" in kind else (total,)
        signal = np.random.default_rng(5).integers(-20000, 20000, shape, dtype=np.int16)
    else:
        signal = (S.uniform_pm1(total, 77) * np.float32(0.4)).astype(np.float32)
    stereo_mode = 1 if "stereo" in kind else 0
    cfg = dsp.speaker_config() if kind == "speaker_float" else None        # n_fft 400, DSP_LOG_GLOBAL_REF1 per clip, centred framing
    with dsp.MfccPlan(cfg) as plan:
        ref, fo_ref = plan.clips_ragged(torch.from_numpy(signal).cuda(), RAGGED_OFFSETS, MAX_FRAMES, stereo_mode)
        ref = ref.cpu().numpy()
        rows = np.diff(fo_ref)
        assert rows[RAGGED_LENGTHS.index(9000)] == MAX_FRAMES and (rows[np.array(RAGGED_LENGTHS) == 0] == 0).all() and len(ref) > 100
        if cfg is None:
            assert rows[RAGGED_LENGTHS.index(399)] == 0 and rows[RAGGED_LENGTHS.index(400)] == 1
        item = signal.itemsize * (2 if "stereo" in kind else 1)
        want = len(dsp.plan_host_chunks(len(RAGGED_LENGTHS), item, 16384, RAGGED_OFFSETS)) - 1
        assert want >= 4
        for depth in (1, 3):
            pipeline(chunk_bytes=16384, depth=depth, pageable_mode=STAGE)
            for source, path in ((signal, "staged"), (_pinned(signal), "pinned")):
                got, fo = plan.clips_ragged_host(source, RAGGED_OFFSETS, MAX_FRAMES, stereo_mode)
                assert np.array_equal(fo, fo_ref) and np.array_equal(got, ref), (depth, path)
                st = dsp.host_pipeline_stats(0)
                assert (st["n_chunks"], st["depth"], st["input_path"], st["bytes_d2h"]) == (want, depth, path, ref.nbytes), st
        pipeline()
        got, _ = plan.clips_ragged_host(signal, RAGGED_OFFSETS, MAX_FRAMES, stereo_mode)
        assert np.array_equal(got, ref) and dsp.host_pipeline_stats(0)["n_chunks"] == 1
        empty, fo = plan.clips_ragged_host(signal, [7, 7, 7], MAX_FRAMES, stereo_mode)      # clips without a frame: no rows, no device work
        assert empty.shape == (0, 13) and fo.tolist() == [0, 0, 0]


def classify_clips(n_clips=70, n=8000, seed=900):
    """Half-second clips from the classifier tests' generators (tests/signals.py): a third the call that fires the rule (label 1), a
    third a 2 kHz burst (a midpoint, label 0), a third noise.  The CPU oracle on these seeds: float32 24 labels 1 and 47 clips with a
    midpoint, float64 (45 dB) 24 labels 1 and a midpoint in all 70."""
    fs = 16000.0
    t = np.arange(n, dtype=np.float64) / fs
    gate = ((t >= 0.10) & (t < 0.40)).astype(np.float64)
    out = np.zeros((n_clips, n), np.float64)
    for i in range(n_clips):
        if i % 3 == 0:
            out[i] = gate * (0.4 * np.sin(2 * np.pi * 2000.0 * t) + 0.02 * S.band_noise(n, seed + 3 * i, 5000, 7000)
                             + 0.05 * S.band_noise(n, seed + 3 * i + 1, 500, 2500)) + 1e-3 * S.uniform_pm1(n, seed + 3 * i + 2)
        elif i % 3 == 1:
            out[i] = S.tone_burst(n, fs, [(0.08, 0.38)], [2000.0], [0.4]).astype(np.float64) + 1e-3 * S.uniform_pm1(n, seed + 3 * i)
        else:
            out[i] = 0.05 * S.uniform_pm1(n, seed + 3 * i).astype(np.float64)
    return out.astype(np.float32)


def _same_traces(a, b):
    return len(a) == len(b) and all(np.array_equal(ma, mb) and np.array_equal(sa, sb) for (ma, sa), (mb, sb) in zip(a, b))


def _device_f64_with_trace(dsp, clips):
    """dsp_classify_batch_device_f64 with its trace array: (labels, traces) as the host wrapper returns them"""
    import torch
    import sys
    dc = sys.modules["dsp_amd.classify"]                      # (the package's attribute of that name is the function)
    n_clips, n = clips.shape
    d = torch.from_numpy(clips).cuda()
    labels = torch.empty(n_clips, dtype=torch.int32, device="cuda")
    raw = torch.zeros(n_clips * C.sizeof(dsp.lib.ClassifyTraceF64), dtype=torch.uint8, device="cuda")
    dsp.lib.check(dsp.load().dsp_classify_batch_device_f64(None, d.data_ptr(), n_clips, n, n, labels.data_ptr(), raw.data_ptr(), dsp.lib.current_stream(d)),
                  "dsp_classify_batch_device_f64")
    host = bytearray(raw.cpu().numpy().tobytes())
    tr = (dsp.lib.ClassifyTraceF64 * n_clips).from_buffer(host)
    return labels.cpu().numpy(), dc._traces(tr, n_clips, np.float64)


@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
def test_classify_uniform_host_in_chunks_of_16_clips(dsp, pipeline, f64):
    """Labels against the device entry, traces against the one-chunk host run.  The float64 device entry has a trace array, and the
    one-chunk run is first held to it; the float32 device entry has none, so for float32 the midpoint count of the non-vacuity check and
    the traces come from the one-chunk host run, whose labels are held to the device entry's."""
    import torch
    clips = classify_clips().astype(np.float64 if f64 else np.float32)
    host = dsp.classify_batch_f64 if f64 else dsp.classify_batch
    one_labels, one_trace = host(clips, with_trace=True)                   # the defaults: one chunk, one pass
    assert dsp.host_pipeline_stats(0)["n_chunks"] == 1
    if f64:
        dev_labels, dev_trace = _device_f64_with_trace(dsp, clips)
        assert np.array_equal(one_labels, dev_labels) and _same_traces(one_trace, dev_trace)
    else:                                                                   # (the float32 device entry has no trace array: its labels, and
        dev_labels = dsp.classify_device(torch.from_numpy(clips).cuda()).cpu().numpy()      # the midpoints of the one-chunk run they equal)
        dev_trace = one_trace
        assert np.array_equal(one_labels, dev_labels)
    # not vacuous: the device entry's own result has midpoints in at least a third of the clips and fires the rule
    assert sum(len(m) > 0 for m, _ in dev_trace) * 3 >= len(clips) and (dev_labels == 1).sum() >= 1 and (dev_labels == 0).sum() >= 1
    for depth in (1, 3):
        pipeline(chunk_bytes=16 * clips.shape[1] * clips.itemsize, depth=depth, pageable_mode=STAGE, classify_min_clips=1)
        for source, path in ((clips, "staged"), (_pinned(clips).numpy(), "pinned")):
            labels, trace = host(source, with_trace=True)
            st = dsp.host_pipeline_stats(0)
            assert (st["n_chunks"], st["depth"], st["input_path"]) == (5, depth, path), st      # 4 chunks of 16 clips and one of 6
            assert np.array_equal(labels, dev_labels) and _same_traces(trace, one_trace), (depth, path)
            assert st["bytes_h2d"] == clips.nbytes
        assert np.array_equal(host(clips), dev_labels)                      # without the trace: labels alone travel back
    pcm = np.round(clips * 32767.0).astype(np.int16)                        # the int16 entries take the same road
    pcm_host = dsp.classify_batch_f64_pcm16 if f64 else dsp.classify_batch_pcm16
    pcm_dev = dsp.classify_device_f64_pcm16 if f64 else dsp.classify_device_pcm16
    pipeline(chunk_bytes=16 * clips.shape[1] * 2, depth=2, pageable_mode=STAGE, classify_min_clips=1)
    labels = pcm_host(pcm)
    assert dsp.host_pipeline_stats(0)["n_chunks"] == 5
    assert np.array_equal(labels, pcm_dev(torch.from_numpy(pcm).cuda()).cpu().numpy()) and labels.sum() >= 1


@pytest.mark.parametrize("f64", [False, True], ids=["float32", "float64"])
def test_classify_ragged_host_in_small_chunks(dsp, pipeline, f64):
    import torch
    clips = classify_clips(24).astype(np.float64 if f64 else np.float32)
    # clips cut to other lengths -- none, below one spectrogram segment (256), exactly one, odd ones -- and one of two clips' samples,
    # longer than a chunk of 40 000 bytes in either precision (whole clips of 8000 doubles are longer, too)
    lengths = [8000, 0, 100, 255, 256, 4001, 8000, 6001, 8000, 0, 0, 7999, 16000, 8000, 480, 8000, 5003, 8000, 0, 8000, 3000, 8000, 8000]
    parts, offsets, at = [np.zeros(3, clips.dtype)], [3], 0
    for n in lengths:
        take = np.concatenate([clips[at % 24], clips[(at + 3) % 24]])[:n]
        parts.append(take)
        offsets.append(offsets[-1] + n)
        at += 1
    signal = np.concatenate(parts)
    host = dsp.classify_ragged_f64 if f64 else dsp.classify_ragged
    device = dsp.classify_device_ragged_f64 if f64 else dsp.classify_device_ragged
    dev_labels = device(torch.from_numpy(signal).cuda(), offsets).cpu().numpy()
    one_labels, one_trace = host(signal, offsets, with_trace=True)          # the defaults: one chunk
    assert dsp.host_pipeline_stats(0)["n_chunks"] == 1 and np.array_equal(one_labels, dev_labels)
    assert sum(len(m) > 0 for m, _ in one_trace) * 3 >= len(lengths) and (dev_labels == 1).sum() >= 1 and (dev_labels == 0).sum() >= 1
    want = len(dsp.plan_host_chunks(len(lengths), signal.itemsize, 40000, offsets)) - 1
    assert want >= 8
    for depth in (1, 3):
        pipeline(chunk_bytes=40000, depth=depth, pageable_mode=STAGE, classify_min_clips=1)
        for source, path in ((signal, "staged"), (_pinned(signal).numpy(), "pinned")):
            labels, trace = host(source, offsets, with_trace=True)
            st = dsp.host_pipeline_stats(0)
            assert (st["n_chunks"], st["depth"], st["input_path"]) == (want, depth, path), st
            assert np.array_equal(labels, dev_labels) and _same_traces(trace, one_trace), (depth, path)
    assert np.array_equal(host(signal, offsets), dev_labels)


def test_a_refused_call_leaves_the_pipeline_usable(dsp, pipeline, clips37):
    x, ref = clips37
    L = dsp.load()
    with dsp.MfccPlan() as plan:
        pipeline(chunk_bytes=5 * 1000 * 4, depth=2, pageable_mode=STAGE, classify_min_clips=1)
        assert np.array_equal(plan.clips_host(x, MAX_FRAMES), ref)
        assert L.dsp_mfcc_clips_host(plan._h, x.ctypes.data, 37, 999, 999, None, MAX_FRAMES) == -1 and "NULL buffer" in dsp.lib.last_error()
        assert L.dsp_mfcc_clips_ragged_host(plan._h, x.ctypes.data, 1, np.array([0, 999], np.int64).ctypes.data_as(dsp.lib.LP), MAX_FRAMES, None) == -1
        assert L.dsp_classify_batch_host(x.ctypes.data, 37, 999, 999, None, None) == -1
        assert np.array_equal(plan.clips_host(x, MAX_FRAMES), ref)            # the next call on the same device: correct, in 8 chunks
        assert dsp.host_pipeline_stats(0)["n_chunks"] == 8
        labels = dsp.classify_batch(x)                                        # and another entry through the same pipeline
        assert labels.shape == (37,) and dsp.host_pipeline_stats(0)["n_chunks"] == 8
    dsp.host_pipeline_release(0)                                              # the ring's memory back; the next call makes it again
    with dsp.MfccPlan() as plan:
        assert np.array_equal(plan.clips_host(x, MAX_FRAMES), ref)
