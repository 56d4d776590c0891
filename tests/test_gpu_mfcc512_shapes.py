"""GPU: every instantiation of the 512-point wave kernel (tests/mfcc512_shapes.py: the six DSP_FOR_SHAPES shapes, both mel placements,
an empty-filter bank, the edges of n_mfcc) at frame lengths 512 / 400 / 320 (FLEN 512, FLEN 400 where compiled in, the run-time
predicate) and both log modes (tile epilogue / per-frame epilogue with the two-pass clip floor), through the frames, clips and ragged
entries.  Every comparison is the project's pure gate (tests/conftest.py gate(), no floor case) against the oracle with its float64
FFT; tests/test_mfcc512_shapes_cpu.py holds the reference's own float32 noise on the same inputs inside that gate.  Ragged rows and
the identities between the entries are bit for bit.  The worst ratio per variant is printed when the module ends."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import mfcc512_shapes as M
from tests.conftest import RTOL, frame_linf_close, gate
from tests.test_gpu_mfcc400 import _run_clips
from tests.test_gpu_ragged_mfcc import _check_against_one_clip_calls, _float_one_clip

pytestmark = pytest.mark.gpu

NO_CAP = 2**31 - 1
CELLS = [(name, fl, lm) for name in M.NAMES for fl in M.FRAME_LENGTHS for lm in M.LOG_MODES]
WORST = {}      # variant -> (worst ratio, case)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for variant in sorted(WORST):
        worst, case = WORST[variant]
        print(f"shape gate {variant}  worst |err| / max(|ref|, L-inf) {worst:.2e} of {RTOL:.0e}  ({case})")


def _plan(name, frame_length, log_mode):
    import dsp_amd
    return dsp_amd.MfccPlan(M.config(name, frame_length, log_mode))


def _gate(got, ref, name, frame_length, log_mode, what):
    """the figure is recorded and printed before gate() asserts it"""
    case = f"mfcc512 shapes {name} flen{frame_length} log{log_mode} {what}"
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    _ok, worst = frame_linf_close(got, ref, RTOL)
    variant = M.SHAPES[name][1]
    if variant not in WORST or worst > WORST[variant][0]:
        WORST[variant] = (worst, case)
    print(f"{case}: {worst:.2e}")
    gate(got, ref, case)


@functools.lru_cache(maxsize=None)
def _clip_refs(name, frame_length, log_mode):
    cfg = M.oracle_cfg(name, frame_length, log_mode)
    return [O.compute_mfcc(x, 1000, cfg) for x in M.clips_input(name, frame_length)]


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_frames_entry(torch_cuda, name, frame_length, log_mode):
    """1 row (less than a half-tile), 17 (one 16-frame tile and one more), 67 (an odd count over several chunks and the block's four
    waves; one row all zeros, one at 1e-6)"""
    torch = torch_cuda
    plan = _plan(name, frame_length, log_mode)
    ocfg = M.oracle_cfg(name, frame_length, log_mode)
    for n in (1, 17, 67):
        x = M.frames_input(name, frame_length, n)
        out = torch.full((n + 1, plan.cfg.n_mfcc), float("nan"), dtype=torch.float32, device="cuda")
        plan.frames(torch.from_numpy(x).cuda(), out=out)
        got = out.cpu().numpy()
        assert np.isnan(got[n]).all(), "a row past the last frame was written"
        _gate(got[:n], O.mfcc_frames(x, ocfg), name, frame_length, log_mode, f"frames n{n}")
        if n == 67 and log_mode == 0:
            assert not got[33].any()
    plan.close()


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_clips_entry(torch_cuda, name, frame_length, log_mode):
    """three clips of 19 frames on an even stride wider than the clip, NaN before the first clip and behind each: a read outside a
    clip shows as a non-finite row"""
    plan = _plan(name, frame_length, log_mode)
    clips = M.clips_input(name, frame_length)
    got = _run_clips(torch_cuda, plan, clips)
    assert got.shape == (3, M.CLIP_FRAMES, plan.cfg.n_mfcc)
    for kind, g, ref in zip(M.CLIP_KINDS, got, _clip_refs(name, frame_length, log_mode)):
        _gate(g, ref, name, frame_length, log_mode, f"clip {kind}")
    if log_mode == 0:
        silent = -(-(clips[2].size // 2) // M.HOP)                 # the first frame wholly inside the silent half
        assert not got[2, silent:].any()
    plan.close()


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_ragged_entry(torch_cuda, name, frame_length, log_mode):
    """five clips from an odd sample offset (no frame, one frame, one frame and a hop less a sample, 7 frames, 23 frames): each clip's
    rows are the one-clip call's bit for bit, and pass the gate"""
    torch = torch_cuda
    plan = _plan(name, frame_length, log_mode)
    ocfg = M.oracle_cfg(name, frame_length, log_mode)
    buf, offsets = M.ragged_input(name, frame_length)
    sig = torch.from_numpy(buf).cuda()
    mf, fo = plan.clips_ragged(sig, offsets, NO_CAP)
    assert fo.tolist() == [0, 0, 1, 2, 9, 32] and mf.shape == (32, plan.cfg.n_mfcc)
    assert bool(torch.isfinite(mf).all()), "a read outside a clip"
    _check_against_one_clip_calls(torch, mf, fo, offsets, _float_one_clip(torch, plan, sig, NO_CAP))
    got = mf.cpu().numpy()
    for c in range(1, 5):
        ref = O.compute_mfcc(buf[offsets[c]:offsets[c + 1]], 1000, ocfg)
        _gate(got[fo[c]:fo[c + 1]], ref, name, frame_length, log_mode, f"ragged clip {c}")
    plan.close()


@pytest.mark.parametrize("frame_length", M.FRAME_LENGTHS)
@pytest.mark.parametrize("name", M.NAMES)
def test_entries_agree_bit_for_bit(torch_cuda, name, frame_length):
    """log_mode 0: frame t of a clip is the frames entry on the same frame_length samples, and another launch geometry (blocks per CU,
    frames per chunk) gives the same bits on all three entries"""
    torch = torch_cuda
    plan = _plan(name, frame_length, 0)
    clips = torch.from_numpy(np.stack(M.clips_input(name, frame_length))).cuda()
    frames = clips.unfold(1, frame_length, M.HOP).reshape(-1, frame_length).contiguous()
    assert frames.shape[0] == 3 * M.CLIP_FRAMES
    buf, offsets = M.ragged_input(name, frame_length)
    sig = torch.from_numpy(buf).cuda()

    def run():
        return plan.clips(clips, 1000), plan.frames(frames), plan.clips_ragged(sig, offsets, NO_CAP)[0]

    by_clip, by_frame, ragged = run()
    assert tuple(by_clip.shape) == (3, M.CLIP_FRAMES, plan.cfg.n_mfcc)
    assert torch.equal(by_frame.reshape(by_clip.shape), by_clip)
    for launch in ((2, 7), (1, 24)):
        plan.set_launch(*launch)
        for a, b, entry in zip(run(), (by_clip, by_frame, ragged), ("clips", "frames", "ragged")):
            assert torch.equal(a, b), f"{entry} entry under set_launch{launch}"
    plan.set_launch(0, 0)
    plan.close()
