"""GPU: every form of the 2048-point kernel (tests/mfcc_wide_shapes.py: the segment path and the CSR walk for each of its two causes, a
filter of exactly 12 pieces, 191 and 192 segments, empty filters, n_mels 63 / 64 / 65 / 127 / 128, n_mfcc 1 and 32, the aubio family
whole and with stream framing alone) at frame lengths 2048 and 1200 and the log modes the family takes, through the frames, clips and
ragged entries, and int16 input on the aubio family.  Every comparison is the project's pure gate (tests/conftest.py gate(), no floor
case) against the oracle with a float64 FFT; tests/test_mfcc_wide_shapes_cpu.py holds the reference's own float32 noise on the same
inputs inside that gate.  Ragged rows, int16 against float input and the launch geometries are bit for bit.  The worst ratio per
variant is printed when the module ends."""
import functools

import numpy as np
import pytest

from tests import mfcc_wide_shapes as M
from tests import signals as S
from tests.conftest import RTOL, frame_linf_close, gate
from tests.test_gpu_mfcc400 import _run_clips
from tests.test_gpu_ragged_mfcc import _check_against_one_clip_calls, _float_one_clip

pytestmark = pytest.mark.gpu

NO_CAP = 2**31 - 1
CELLS = [(name, fl, lm) for name in M.NAMES_2048 for fl in M.frame_lengths(2048, name) for lm in M.log_modes(name)]
AUBIO_NAMES = [name for name in M.NAMES_2048 if M.is_aubio(name)]
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
        print(f"shape gate 2048 {variant}  worst |err| / max(|ref|, L-inf) {worst:.2e} of {RTOL:.0e}  ({case})")
    _plan.cache_clear()


@functools.lru_cache(maxsize=None)
def _plan(name, frame_length, log_mode):
    import dsp_amd
    return dsp_amd.MfccPlan(M.config(2048, name, frame_length, log_mode))


def _gate(got, ref, name, frame_length, log_mode, what):
    """the figure is recorded and printed before gate() asserts it"""
    case = f"mfcc2048 shapes {name} flen{frame_length} log{log_mode} {what}"
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    _ok, worst = frame_linf_close(got, ref, RTOL)
    variant = M.SHAPES_2048[name][1]
    if variant not in WORST or worst > WORST[variant][0]:
        WORST[variant] = (worst, case)
    print(f"{case}: {worst:.2e}")
    gate(got, ref, case)
    return worst


@functools.lru_cache(maxsize=None)
def _frame_refs(name, frame_length, log_mode):
    return M.reference_frames(2048, name, frame_length, log_mode, M.frames_input(2048, name, frame_length))


@functools.lru_cache(maxsize=None)
def _clip_refs(name, frame_length, log_mode):
    return [M.reference_clip(2048, name, frame_length, log_mode, x) for x in M.clips_input(2048, name, frame_length)]


def _run_stream_clips(torch, plan, clips, lead=8, tail=6):
    """_run_clips (tests/test_gpu_mfcc400.py) for DSP_FRAMING_STREAM, whose frame count that helper does not know: one
    dsp_mfcc_clips_device call on clips of one length on an even stride, NaN before the first clip and behind every clip"""
    import dsp_amd
    from dsp_amd import lib as dl
    n = clips[0].size
    stride = n + (n & 1) + tail
    buf = np.full(lead + stride * len(clips), np.nan, np.float32)
    for i, x in enumerate(clips):
        buf[lead + i * stride: lead + i * stride + n] = x
    d = torch.from_numpy(buf).cuda()
    t = dsp_amd.frames_for(plan.cfg, n, NO_CAP)
    out = torch.full((len(clips), t, plan.cfg.n_mfcc), float("nan"), dtype=torch.float32, device="cuda")
    rc = plan._L.dsp_mfcc_clips_device(plan._h, d.data_ptr() + 4 * lead, len(clips), n, stride, out.data_ptr(), NO_CAP, None)
    assert rc == t == -(-n // plan.cfg.hop_length), (rc, t, dl.last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _first_silent_frame(name, frame_length, n):
    """the first frame of an n-sample clip that lies wholly in its silent second half"""
    hop = M.HOPS[frame_length]
    start = n // 2 + (frame_length - hop if M.is_stream(2048, name) else 0)       # stream framing: frame t starts at (t + 1) hop - frame_length
    return -(-start // hop)


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_frames_entry(torch_cuda, name, frame_length, log_mode):
    """1, 3, 4 and 5 rows (around the block's four waves) and 67 (an odd count over several chunks; one row all zeros, one at 1e-6)"""
    torch = torch_cuda
    plan = _plan(name, frame_length, log_mode)
    x = torch.from_numpy(M.frames_input(2048, name, frame_length)).cuda()
    ref = _frame_refs(name, frame_length, log_mode)
    for n in M.FRAME_ROWS[2048]:
        out = torch.full((n + 1, plan.cfg.n_mfcc), float("nan"), dtype=torch.float32, device="cuda")
        plan.frames(x[:n].contiguous(), out=out)
        got = out.cpu().numpy()
        assert np.isnan(got[n]).all(), "a row past the last frame was written"
        _gate(got[:n], ref[:n], name, frame_length, log_mode, f"frames n{n}")
    if log_mode == 0:
        assert not got[M.ZERO_ROW].any()
    else:       # the clip-global reference and aubio's log10 floor leave a silent frame on their floor, not at zero: the oracle's row, gated above
        assert ref[M.ZERO_ROW].any()


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_clips_entry(torch_cuda, name, frame_length, log_mode):
    """three clips on an even stride wider than the clip, NaN before the first clip and behind each: a read outside a clip shows as a
    non-finite row.  Log mode 1 takes the two-pass floor, and the third clip's silent half lies more than top_db below its maximum."""
    plan = _plan(name, frame_length, log_mode)
    clips = M.clips_input(2048, name, frame_length)
    refs = _clip_refs(name, frame_length, log_mode)
    got = (_run_stream_clips if M.is_stream(2048, name) else _run_clips)(torch_cuda, plan, clips)
    assert got.shape == (3,) + refs[0].shape and np.isfinite(got).all()
    for kind, g, ref in zip(M.CLIP_KINDS, got, refs):
        _gate(g, ref, name, frame_length, log_mode, f"clip {kind}")
    silent = _first_silent_frame(name, frame_length, clips[2].size)
    assert silent < got.shape[1] - 2
    if log_mode == 0:
        assert not got[2, silent:].any()
    elif log_mode == 1:     # every filter of the silent frames sits on the clip's floor (above amin: test_mfcc_wide_shapes_cpu.py), so the rows are equal
        assert np.array_equal(got[2, silent:], np.broadcast_to(got[2, silent], got[2, silent:].shape))


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_ragged_entry(torch_cuda, name, frame_length, log_mode):
    """five clips from an odd sample offset (no frame, one frame, one frame and a hop less a sample, 7 frames, 23 frames): each clip's
    rows are the one-clip call's bit for bit, and pass the gate"""
    torch = torch_cuda
    plan = _plan(name, frame_length, log_mode)
    buf, offsets = M.ragged_input(2048, name, frame_length)
    sig = torch.from_numpy(buf).cuda()
    mf, fo = plan.clips_ragged(sig, offsets, NO_CAP)
    assert np.diff(fo).tolist() == [0, 1, 2 if M.is_stream(2048, name) else 1, 7, 23] and mf.shape == (fo[-1], plan.cfg.n_mfcc)
    assert bool(torch.isfinite(mf).all()), "a read outside a clip"
    _check_against_one_clip_calls(torch, mf, fo, offsets, _float_one_clip(torch, plan, sig, NO_CAP))
    got = mf.cpu().numpy()
    for c in range(1, 5):
        ref = M.reference_clip(2048, name, frame_length, log_mode, buf[offsets[c]:offsets[c + 1]])
        _gate(got[fo[c]:fo[c + 1]], ref, name, frame_length, log_mode, f"ragged clip {c}")


@pytest.mark.parametrize("name,frame_length,log_mode", CELLS)
def test_launch_geometry_changes_no_bit(torch_cuda, name, frame_length, log_mode):
    torch = torch_cuda
    plan = _plan(name, frame_length, log_mode)
    x = torch.from_numpy(M.frames_input(2048, name, frame_length)).cuda()
    n = M.clip_samples(2048, name, frame_length)
    clips = torch.zeros((3, n + (n & 1)), device="cuda")
    clips[:, :n] = torch.from_numpy(np.stack(M.clips_input(2048, name, frame_length))).cuda()
    buf, offsets = M.ragged_input(2048, name, frame_length)
    sig = torch.from_numpy(buf).cuda()

    def run():
        return plan.frames(x), plan.clips(clips[:, :n], NO_CAP), plan.clips_ragged(sig, offsets, NO_CAP)[0]

    first = run()
    for launch in ((2, 7), (1, 24)):
        plan.set_launch(*launch)
        for a, b, entry in zip(run(), first, ("frames", "clips", "ragged")):
            assert torch.equal(a, b), f"{entry} entry under set_launch{launch}"
    plan.set_launch(0, 0)


def _to_float(torch, pcm, layout):
    """the reference's conversions (donut-classifier/classifier.c:292-297, main_test.c:205-217), as test_pcm16_ingestion_matches_float_path"""
    if layout == "mono":
        return pcm.float() / 32768.0
    if layout == "stereo_ch0":
        return pcm[..., 0].float() / 32768.0
    return 0.5 * (pcm[..., 0].float() / 32768.0 + pcm[..., 1].float() / 32768.0)


@pytest.mark.parametrize("layout", ["mono", "stereo_ch0", "stereo_avg"])
@pytest.mark.parametrize("name", AUBIO_NAMES)
def test_pcm16_equals_the_float_path(torch_cuda, name, layout):
    """int16 samples converted in the kernel's load give the bits of the float path fed the reference's conversion, on clips whose odd
    length leaves a partial last hop and on a ragged batch, with the extreme samples in both"""
    torch = torch_cuda
    log_mode = M.log_modes(name)[0]
    for frame_length in M.frame_lengths(2048, name):
        plan = _plan(name, frame_length, log_mode)
        n = M.clip_samples(2048, name, frame_length)
        assert n % M.HOPS[frame_length] and n & 1
        shape = (3, n + 1) if layout == "mono" else (3, n + 1, 2)
        gen = torch.Generator(device="cuda").manual_seed(2048 + n)
        pcm = torch.randint(-32768, 32768, shape, dtype=torch.int16, device="cuda", generator=gen)
        pcm[0, :8] = torch.tensor([-32768, 32767, 0, -1, 1, -32768, 32767, 0], dtype=torch.int16)[(...,) + (None,) * (pcm.dim() - 2)]
        pcm[1, n - 2:n] = 32767
        pcm[2, n - 2:n] = -32768
        mode = 1 if layout == "stereo_avg" else 0
        a = plan.clips_pcm16(pcm[:, :n], NO_CAP, stereo_mode=mode)
        b = plan.clips(_to_float(torch, pcm, layout)[:, :n], NO_CAP)
        assert a.shape[1] == -(-n // M.HOPS[frame_length]) and torch.equal(a, b)
        # the same samples as one ragged batch from an odd offset
        lens = M.ragged_lengths(2048, name, frame_length)
        offsets = np.concatenate([[M.RAGGED_START], M.RAGGED_START + np.cumsum(lens)]).astype(np.int64)
        flat = pcm.reshape((-1,) + tuple(pcm.shape[2:]))[: int(offsets[-1]) + 5].contiguous()
        mf, fo = plan.clips_ragged(flat, offsets, NO_CAP, stereo_mode=mode)
        mf_f, fo_f = plan.clips_ragged(_to_float(torch, flat, layout).contiguous(), offsets, NO_CAP)
        assert np.array_equal(fo, fo_f) and fo[-1] == 33 and torch.equal(mf, mf_f)

        def one(lo, hi):
            return None if hi == lo else plan.clips_pcm16(flat[lo:hi].clone()[None], NO_CAP, stereo_mode=mode)[0]
        _check_against_one_clip_calls(torch, mf, fo, offsets, one)


def test_segment_and_csr_paths_of_one_n_mels_pass_the_same_gate(torch_cuda):
    """"librosa128" (190 segments) and "librosa128_22k_csr" (195: the CSR walk) are the same front end at two sample rates; the same
    white-noise frames through both, each under the gate against its own oracle"""
    torch = torch_cuda
    x = S.uniform_pm1(9 * 2048, 77).reshape(9, 2048) * np.float32(0.5)
    worst = {}
    for name in ("librosa128", "librosa128_22k_csr"):
        plan = _plan(name, 2048, 1)
        assert M.SHAPES_2048[name][0]["n_mels"] == 128
        got = plan.frames(torch.from_numpy(x).cuda()).cpu().numpy()
        worst[name] = _gate(got, M.reference_frames(2048, name, 2048, 1, x), name, 2048, 1, "shared noise frames")
    assert M.SHAPES_2048["librosa128"][1][1] == 1 and M.SHAPES_2048["librosa128_22k_csr"][1][1] == 0
