"""GPU: DSP_FRAMING_CENTER at n_fft 2048 (dsp_mfcc_librosa_config; mfcc2048_kernel.hip, CENTER) on the configurations and clips of
tests/mfcc2048_center_cases.py, which tests/test_mfcc2048_center_cpu.py holds to the gate without the library: a ragged batch of clips of
1 .. 5000 samples lying back to back against the float64 oracle, against one-clip calls and uniform batches bit for bit, with every sample
outside a clip poisoned (padding is zeros, not neighbours, and nothing outside the clip is loaded), a half-silent clip on the clip
floor, and what a centred plan refuses."""
import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl

from tests import mfcc2048_center_cases as K
from tests import mfcc400_ref as R
from tests.conftest import gate

pytestmark = pytest.mark.gpu
NO_CAP = 1 << 20


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _plan(name):
    sr, n_mfcc, over = K.CONFIGS[name]
    return dsp_amd.MfccPlan(dsp_amd.librosa_config(sr, n_mfcc, **over))


def _batch(name):
    """the clips back to back behind a guard region -> (buffer float32 [GUARD + total + GUARD], offsets [n + 1])"""
    clips = K.clips(name)
    off = K.GUARD + np.concatenate([[0], np.cumsum([y.size for y in clips])]).astype(np.int64)
    buf = np.zeros(int(off[-1]) + K.GUARD, np.float32)
    for y, o in zip(clips, off):
        buf[o: o + y.size] = y
    return buf, off


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_ragged_batch_against_float64_and_against_itself(torch, name):
    cfg = K.cfg_of(name)
    buf, off = _batch(name)
    with _plan(name) as plan:
        dev = torch.from_numpy(buf).cuda()
        rows, fo = plan.clips_ragged(dev, off, NO_CAP)
        assert np.diff(fo).tolist() == list(K.FRAMES)
        rows = rows.cpu().numpy()
        for i, (y, ref) in enumerate(zip(K.clips(name), K.oracle(name))):
            mine = rows[fo[i]: fo[i + 1]]
            gate(mine, ref, f"center2048_{name}_{y.size}")
            # padding is zeros, not neighbours: every sample of the allocation outside clip i is NaN, guard regions included
            poisoned = np.full_like(buf, np.nan)
            poisoned[off[i]: off[i + 1]] = y
            alone, fo1 = plan.clips_ragged(torch.from_numpy(poisoned).cuda(), off[i: i + 2], NO_CAP)
            assert fo1.tolist() == [0, K.FRAMES[i]]
            assert alone.cpu().numpy().tobytes() == mine.tobytes(), f"{name}: clip {i} ({y.size} samples) alone among NaN differs from its rows in the batch"
            # a uniform batch of that length (even clip stride, the gap and the neighbours NaN)
            stride = y.size + (y.size & 1) + 2
            uni = np.full((3, stride), np.nan, np.float32)
            uni[1, : y.size] = y
            uni[0, : y.size] = 0.25 * y
            uni[2, : y.size] = 0.0
            got = plan.clips(torch.from_numpy(uni).cuda()[:, : y.size], NO_CAP).cpu().numpy()
            assert got.shape == (3, K.FRAMES[i], cfg.n_mfcc)
            assert got[1].tobytes() == mine.tobytes(), f"{name}: clip {i} ({y.size} samples) in a uniform batch differs from its rows in the ragged one"
            assert np.isfinite(got).all()
        # max_frames caps every clip
        capped, foc = plan.clips_ragged(dev, off, 3)
        assert np.diff(foc).tolist() == [min(t, 3) for t in K.FRAMES]
        if cfg.log_mode == R.LOG_PER_FRAME_MAX:          # (under GLOBAL_REF1 the floor is that of the frames computed)
            capped = capped.cpu().numpy()
            for i in range(len(K.LENGTHS)):
                assert capped[foc[i]: foc[i + 1]].tobytes() == rows[fo[i]: fo[i] + foc[i + 1] - foc[i]].tobytes()


@pytest.mark.parametrize("name", ["keyword_22k_13", "cepstrum_16k_20", "keyword_22k_13_frame_max"])
def test_a_half_silent_clip_sits_on_the_clip_floor(torch, name):
    cfg = K.cfg_of(name)
    y = K.half_silent_clip(name)
    ref = R.features(y, cfg)
    with _plan(name) as plan:
        rows = plan.clips(torch.from_numpy(y).cuda()[None, :], NO_CAP).cpu().numpy()[0]
    gate(rows, ref, f"center2048_{name}_half_silent")
    if cfg.log_mode == R.LOG_GLOBAL_REF1:
        # frames 7 .. 9 lie wholly in the silence: every filter on the clip's floor, max - top_db -> c0 = sqrt(n_mels) floor, the rest 0
        assert rows[7].tobytes() == rows[8].tobytes() == rows[9].tobytes()
        assert np.abs(rows[8, 1:]).max() <= 1e-4 * abs(rows[8, 0]) and rows[8, 0] < rows[0, 0]
        e = R.mel_energies(R.cut(y, cfg), cfg)
        floor = 10.0 * np.log10(np.maximum(e, cfg.amin)).max() - cfg.top_db
        assert abs(rows[8, 0] - np.sqrt(cfg.n_mels) * floor) <= 1e-4 * abs(np.sqrt(cfg.n_mels) * floor)
    else:
        assert rows[8].tobytes() == rows[9].tobytes()      # a silent frame is its own reference: every filter at 0 dB of amin


@pytest.mark.parametrize("name", ["keyword_22k_13", "cepstrum_16k_20_frame_max"])
def test_host_forms_give_the_device_forms_bits(torch, name):
    """dsp_mfcc_clips_host and dsp_mfcc_clips_ragged_host on a centred plan: staged copies of the same clips, the same rows bit for bit
    (odd lengths included: the host form stages equal clips at an even stride)"""
    clips = K.clips(name)
    off = np.concatenate([[0], np.cumsum([y.size for y in clips])]).astype(np.int64)
    flat = np.concatenate(clips)
    with _plan(name) as plan:
        dev, fo = plan.clips_ragged(torch.from_numpy(flat).cuda(), off, NO_CAP)
        host, fo_h = plan.clips_ragged_host(flat, off, NO_CAP)
        assert fo_h.tolist() == fo.tolist() and host.tobytes() == dev.cpu().numpy().tobytes()
        for n in (1, 1025, 3000):
            x = np.stack([K.clip(name, n, K.CONFIGS[name][0]), 0.5 * K.clip(name, n, K.CONFIGS[name][0])[::-1]]).astype(np.float32)
            want = np.stack([plan.clips(torch.from_numpy(x[i:i + 1]).cuda(), NO_CAP).cpu().numpy()[0] for i in range(2)])
            got = plan.clips_host(x, NO_CAP)
            assert got.shape == (2, 1 + n // K.HOP, K.cfg_of(name).n_mfcc) and got.tobytes() == want.tobytes(), f"{name}: clips_host at {n} samples"


def test_independent_frames_run_and_the_rest_is_refused_naming_the_framing(torch):
    cfg = dsp_amd.librosa_config()
    with dsp_amd.MfccPlan(cfg) as plan, dsp_amd.MfccPlan(dsp_amd.librosa_config(framing=dl.FRAMING_COMPLETE)) as whole:
        x = torch.from_numpy(np.stack([K.clip("keyword_22k_13", 2048, 22050), K.clip("keyword_22k_13", 2048 + 1, 22050)[1:]])).cuda()
        assert plan.frames(x).cpu().numpy().tobytes() == whole.frames(x).cpu().numpy().tobytes()      # whole frames: no padding
        pcm = torch.zeros((2, 4096), dtype=torch.int16, device="cuda")
        with pytest.raises(dsp_amd.DspError, match="framing"):
            plan.clips_pcm16(pcm, NO_CAP)
        with pytest.raises(dsp_amd.DspError, match="framing"):
            plan.clips_ragged(pcm.reshape(-1), [0, 4096, 8192], NO_CAP)
        from tests import consumer_ref
        stop = consumer_ref.random_stop_model(np.random.default_rng(1), 13, 20, (4, 2, 2, 1))
        with dsp_amd.StopModel(stop) as sm:
            with pytest.raises(dsp_amd.DspError, match="framing"):
                dsp_amd.Scanner(plan, stop=sm, window_frames=10, hop_frames=5)
            with pytest.raises(dsp_amd.DspError, match="framing"):
                dsp_amd.StreamSession(plan, 2, stop=sm, window_frames=10, hop_frames=5)
            with pytest.raises(dsp_amd.DspError, match="framing"):
                sm.classify_signal_ragged(plan, torch.zeros(8192, device="cuda"), [0, 4096, 8192])
