"""CPU: the host side of ragged MFCC matrices -- dsp_mfcc_ragged_frame_offsets (no GPU call) against a prefix sum of
dsp_mfcc_frames_for, and the argument checks the ragged entry points make before any device work."""
import ctypes as C

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from dsp_amd import mfcc as M

LENGTHS = [0, 399, 400, 401, 16000, 16001, 559, 560, 24029, 1023, 1024, 1025, 2047, 2048, 2049, 0, 3, 96001, 160 * 777 + 13]


def _configs():
    sj = dl.MfccConfig()
    dl.load().dsp_mfcc_scrubjay_infer_config(C.byref(sj), 16000)
    return {"reference": dsp_amd.default_config(), "scrubjay_infer": sj}


@pytest.mark.parametrize("cfg_name", ["reference", "scrubjay_infer"])
@pytest.mark.parametrize("max_frames", [0, 7, 500])
def test_frame_offsets_are_the_prefix_sum_of_frames_for(cfg_name, max_frames):
    cfg = _configs()[cfg_name]
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    want = np.concatenate([[0], np.cumsum([dsp_amd.frames_for(cfg, n, max_frames) for n in LENGTHS])]).astype(np.int64)
    got = M.ragged_frame_offsets(cfg, offsets, max_frames)
    assert got.dtype == np.int64 and got.shape == (len(LENGTHS) + 1,)
    np.testing.assert_array_equal(got, want)
    # the C entry point returns the total
    L = dl.load()
    off, n = dl.c_offsets(offsets)
    fo = (C.c_long * (n + 1))()
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, max_frames, fo) == want[-1]
    if max_frames == 500:      # zero-frame clips are legal and add no rows
        assert want[-1] > 0 and np.any(np.diff(want) == 0)


def test_frame_offsets_of_an_empty_batch_and_of_clips_anywhere_in_the_buffer():
    cfg = dsp_amd.default_config()
    assert M.ragged_frame_offsets(cfg, [5], 500).tolist() == [0]
    # clips need not start at 0 or at even positions; only their lengths count
    got = M.ragged_frame_offsets(cfg, [7, 407, 407, 16408], 500)
    assert got.tolist() == [0, 1, 1, 1 + 98]


def test_decreasing_offsets_are_rejected():
    L = dl.load()
    cfg = dsp_amd.default_config()
    off, n = dl.c_offsets([0, 16000, 15999, 32000])
    fo = (C.c_long * (n + 1))()
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, 500, fo) == -1       # DSP_EINVAL
    assert "non-decreasing" in dl.last_error() and "clip 1" in dl.last_error()
    with pytest.raises(dl.DspError):
        M.ragged_frame_offsets(cfg, [0, 16000, 15999, 32000], 500)
    off, n = dl.c_offsets([-4, 16000])
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, 500, fo) == -1
    assert "non-decreasing" in dl.last_error() and "clip 0" in dl.last_error()
    off, n = dl.c_offsets([0, 16000, 16000 + 2**31])           # a clip of 2^31 samples
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, 500, fo) == -1
    assert "non-decreasing" in dl.last_error() and "clip 1" in dl.last_error()


def test_bad_arguments_are_rejected_without_a_gpu():
    L = dl.load()
    cfg = dsp_amd.default_config()
    off, n = dl.c_offsets([0, 16000])
    fo = (C.c_long * 2)()
    assert L.dsp_mfcc_ragged_frame_offsets(None, off, n, 500, fo) == -1
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), None, n, 500, fo) == -1
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, 500, None) == -1
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, -1, 500, fo) == -1
    bad = dsp_amd.default_config(hop_length=0)
    assert L.dsp_mfcc_ragged_frame_offsets(C.byref(bad), off, n, 500, fo) == -1
    # the device entries check their arguments before touching a plan or a device
    assert L.dsp_mfcc_clips_ragged_device(None, None, 1, off, 500, None, None) == -1
    assert L.dsp_mfcc_clips_ragged_pcm16_device(None, None, 1, off, 3, 0, 500, None, None) == -1
    assert L.dsp_mfcc_clips_ragged_pcm16_device(None, None, 1, off, 2, 7, 500, None, None) == -1
    assert L.dsp_speaker_llr_ragged_device(None, None, 1, off, None, None, None, None, None) == -1


def test_ragged_entries_are_exported_and_listed():
    L = dl.load()
    for name in ("dsp_mfcc_ragged_frame_offsets", "dsp_mfcc_clips_ragged_device", "dsp_mfcc_clips_ragged_pcm16_device",
                 "dsp_speaker_llr_ragged_device"):
        assert hasattr(L, name) and name in dl.SYMBOLS
