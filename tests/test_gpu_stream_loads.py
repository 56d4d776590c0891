"""GPU: the shapes at which a change of the frame loads' path (cache policy, helper, instantiation) could show.

frames entry (back-to-back 512-sample frames: the non-temporal loads of csrc/stream_load.hpp) on 1, 16, 17 and 4099 frames -- less
than a tile, exactly one 16-frame tile, one frame more, and more frames than one launch has waves -- against the CPU oracle under
the project's pure gate; the PCM16 entry with one frame per clip (mono, stereo channel 0, stereo average) on the SAME samples, bit
for bit the float entry's rows; one 3-clip call of the overlapping 400 / 160 framing (cacheable loads) against the oracle under
the same gate.  The samples are int16 / 32768, so the float and the int16 entries read the same values.  The oracle runs once per
module (4099 frames), the smaller counts are its first rows: a frame's coefficients do not depend on its place in the batch."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import gate

pytestmark = pytest.mark.gpu

FRAME = 512
COUNTS = (1, 16, 17, 4099)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _pcm():
    """[4099][512] int16 in +-16000 and a second channel offset d with |s +- d| < 32768: left = s + d, right = s - d"""
    rng = np.random.default_rng(512)
    s = rng.integers(-16000, 16001, size=(max(COUNTS), FRAME), dtype=np.int16)
    d = rng.integers(-16000, 16001, size=s.shape, dtype=np.int16)
    s[5] = 0                                    # a silent frame
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


@functools.lru_cache(maxsize=None)
def _frames_f32():
    x = (_pcm()[0].astype(np.float32) / np.float32(32768.0))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle_rows():
    ref = O.mfcc_frames(_frames_f32(), O.default_cfg(frame_length=FRAME, hop_length=FRAME))
    ref.setflags(write=False)
    return ref


def _plan():
    import dsp_amd
    return dsp_amd.MfccPlan(dsp_amd.default_config(frame_length=FRAME, hop_length=FRAME))


def _frames_entry(torch, plan, n):
    out = torch.full((n + 1, plan.cfg.n_mfcc), float("nan"), dtype=torch.float32, device="cuda")
    plan.frames(torch.from_numpy(_frames_f32()[:n].copy()).cuda(), out=out)
    assert bool(torch.isnan(out[n]).all()), "a row past the last frame was written"
    return out[:n]


@pytest.mark.parametrize("n", COUNTS)
def test_frames_against_oracle(torch_cuda, n):
    plan = _plan()
    got = _frames_entry(torch_cuda, plan, n).cpu().numpy()
    if n > 5:
        assert not got[5].any(), "the silent frame"
    gate(got, _oracle_rows()[:n], f"stream loads frames n{n}")
    plan.close()


@pytest.mark.parametrize("n", COUNTS)
def test_pcm16_one_frame_per_clip_is_the_float_entry(torch_cuda, n):
    torch = torch_cuda
    plan = _plan()
    want = _frames_entry(torch, plan, n)
    s, d = (a[:n].astype(np.int32) for a in _pcm())
    left = torch.from_numpy((s + d).astype(np.int16))
    right = torch.from_numpy((s - d).astype(np.int16))
    mono = torch.from_numpy(_pcm()[0][:n].copy()).cuda()
    stereo_left = torch.stack((mono.cpu(), right), dim=2).contiguous().cuda()        # channel 0 = s, channel 1 something else
    stereo_avg = torch.stack((left, right), dim=2).contiguous().cuda()               # (L + R) / 65536 = s / 32768
    for what, pcm, mode in (("mono", mono, 0), ("stereo, channel 0", stereo_left, 0), ("stereo, average", stereo_avg, 1)):
        got = plan.clips_pcm16(pcm, 1, stereo_mode=mode)
        assert tuple(got.shape) == (n, 1, plan.cfg.n_mfcc), what
        assert torch.equal(got[:, 0], want), f"{what}: not the float entry's bits on {n} frames"
    plan.close()


def test_three_overlapping_clips_against_oracle(torch_cuda):
    """400-sample frames every 160 (every sample read 2.5 times: the cacheable loads), three clips of 2000 samples on a stride wider
    than the clip"""
    import dsp_amd
    torch = torch_cuda
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    assert (plan.cfg.frame_length, plan.cfg.hop_length) == (400, 160)
    samples, stride = 2000, 2048
    x = _frames_f32().reshape(-1)[:3 * stride].reshape(3, stride)
    buf = torch.full((3, stride), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :samples] = torch.from_numpy(x[:, :samples].copy()).cuda()
    got = plan.clips(buf[:, :samples], 1000).cpu().numpy()
    t = 1 + (samples - 400) // 160
    assert got.shape == (3, t, plan.cfg.n_mfcc)
    for c in range(3):
        gate(got[c], O.compute_mfcc(x[c, :samples], 1000), f"stream loads clip {c} of 3 (400 / 160)")
    plan.close()
