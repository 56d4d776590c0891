"""GPU: every form of the two 1024-point kernels (tests/mfcc_wide_shapes.py: chunk slots 1..3, both mel placements, filters of up to 3, 5
and 6 gather pieces, empty filters, the second filter per lane idle and in use, the edges of n_mfcc) at frame lengths 1024 and 800
(the wave kernel's <FULL, CLIPS> instantiations) through the frames and clips entries, on the wave kernel and on the Stockham kernel
(set_kernel(1)), and the per-frame prefilter on its four paths.  Every comparison is the project's pure gate (tests/conftest.py gate(),
no floor case) against the oracle with its float64 FFT; tests/test_mfcc_wide_shapes_cpu.py holds the reference's own float32 noise on
the same inputs inside that gate.  The identities between the entries and launch geometries are bit for bit.  The worst ratio per
variant is printed when the module ends."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import mfcc_wide_shapes as M
from tests import signals as S
from tests.conftest import RTOL, frame_linf_close, gate
from tests.test_gpu_mfcc400 import _run_clips

pytestmark = pytest.mark.gpu

CELLS = [(name, fl) for name in M.NAMES_1024 for fl in M.FRAME_LENGTHS[1024]]
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
        print(f"shape gate 1024 {variant}  worst |err| / max(|ref|, L-inf) {worst:.2e} of {RTOL:.0e}  ({case})")
    _plan.cache_clear()


@functools.lru_cache(maxsize=None)
def _plan(name, frame_length, prefilter=0):
    import dsp_amd
    return dsp_amd.MfccPlan(M.config(1024, name, frame_length, prefilter=prefilter))


def _kernels(name):
    """(kernel id, what it runs): banks of up to three slots run on both kernels; four slots would leave the Stockham kernel alone"""
    return ((0, "wave"), (1, "stockham")) if M.SHAPES_1024[name][1][0] <= 3 else ((1, "stockham"),)


def _gate(got, ref, name, what):
    """the figure is recorded and printed before gate() asserts it"""
    case = f"mfcc1024 shapes {name} {what}"
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    _ok, worst = frame_linf_close(got, ref, RTOL)
    variant = M.SHAPES_1024[name][1]
    if variant not in WORST or worst > WORST[variant][0]:
        WORST[variant] = (worst, case)
    print(f"{case}: {worst:.2e}")
    gate(got, ref, case)


@functools.lru_cache(maxsize=None)
def _frame_refs(name, frame_length):
    return O.mfcc_frames(M.frames_input(1024, name, frame_length), M.oracle_cfg(1024, name, frame_length))


@functools.lru_cache(maxsize=None)
def _clip_refs(name, frame_length):
    return [M.reference_clip(1024, name, frame_length, 0, x) for x in M.clips_input(1024, name, frame_length)]


def _frames(torch, plan, x):
    """the frames entry into a tensor with one NaN row more, which must stay NaN"""
    n = x.shape[0]
    out = torch.full((n + 1, plan.cfg.n_mfcc), float("nan"), dtype=torch.float32, device="cuda")
    plan.frames(x, out=out)
    assert bool(torch.isnan(out[n]).all()), "a row past the last frame was written"
    return out[:n]


@pytest.mark.parametrize("name,frame_length", CELLS)
def test_frames_entry(torch_cuda, name, frame_length):
    """1, 7, 8, 9, 16, 17 and 67 rows: around the wave kernel's 8-frame granule and its 16-frame tile, and an odd count over several
    chunks and the block's four waves (one row all zeros, one at 1e-6); each kernel against the oracle and the two against each other"""
    torch = torch_cuda
    plan = _plan(name, frame_length)
    x = torch.from_numpy(M.frames_input(1024, name, frame_length)).cuda()
    ref = _frame_refs(name, frame_length)
    outs = {}
    for kern, what in _kernels(name):
        plan.set_kernel(kern)
        for n in M.FRAME_ROWS[1024]:
            got = _frames(torch, plan, x[:n].contiguous()).cpu().numpy()
            _gate(got, ref[:n], name, f"flen{frame_length} {what} frames n{n}")
        assert not got[M.ZERO_ROW].any()
        outs[kern] = got
    if len(outs) == 2:
        assert np.abs(outs[0] - outs[1]).max() <= 2e-3        # two different FFT factorisations of the same chain
    else:
        plan.set_kernel(0)                                    # a bank of four slots: the wave kernel does not hold it, the plan stays on the Stockham kernel
        assert np.array_equal(_frames(torch, plan, x).cpu().numpy(), outs[1])
    plan.set_kernel(0)


@pytest.mark.parametrize("name,frame_length", CELLS)
def test_clips_entry(torch_cuda, name, frame_length):
    """three clips of 19 frames on an even stride wider than the clip, NaN before the first clip and behind each: a read outside a
    clip shows as a non-finite row"""
    plan = _plan(name, frame_length)
    clips = M.clips_input(1024, name, frame_length)
    outs = {}
    for kern, what in _kernels(name):
        plan.set_kernel(kern)
        got = _run_clips(torch_cuda, plan, clips)
        assert got.shape == (3, M.CLIP_FRAMES, plan.cfg.n_mfcc) and np.isfinite(got).all()
        for kind, g, ref in zip(M.CLIP_KINDS, got, _clip_refs(name, frame_length)):
            _gate(g, ref, name, f"flen{frame_length} {what} clip {kind}")
        silent = -(-(clips[2].size // 2) // M.HOPS[frame_length])          # the first frame wholly inside the silent half
        assert not got[2, silent:].any()
        outs[kern] = got
    if len(outs) == 2:
        assert np.abs(outs[0] - outs[1]).max() <= 2e-3
    plan.set_kernel(0)


@pytest.mark.parametrize("name,frame_length", CELLS)
def test_entries_agree_bit_for_bit(torch_cuda, name, frame_length):
    """on either kernel, frame t of a clip is the frames entry on the same frame_length samples, and another launch geometry (blocks per
    CU, frames per chunk) gives the same bits on both entries"""
    torch = torch_cuda
    plan = _plan(name, frame_length)
    clips = torch.from_numpy(np.stack(M.clips_input(1024, name, frame_length))).cuda()
    frames = clips.unfold(1, frame_length, M.HOPS[frame_length]).reshape(-1, frame_length).contiguous()
    assert frames.shape[0] == 3 * M.CLIP_FRAMES
    for kern, what in _kernels(name):
        plan.set_kernel(kern)
        by_clip, by_frame = plan.clips(clips, 1000), plan.frames(frames)
        assert tuple(by_clip.shape) == (3, M.CLIP_FRAMES, plan.cfg.n_mfcc)
        assert torch.equal(by_frame.reshape(by_clip.shape), by_clip), what
        for launch in ((2, 7), (1, 24)):
            plan.set_launch(*launch)
            assert torch.equal(plan.clips(clips, 1000), by_clip), f"{what}: clips entry under set_launch{launch}"
            assert torch.equal(plan.frames(frames), by_frame), f"{what}: frames entry under set_launch{launch}"
        plan.set_launch(0, 0)
    plan.set_kernel(0)


def _prefilter_frames():
    """17 frames of 1024 samples: the stop-band frames of test_config3_prefilter_on_frames_that_live_in_the_stop_band (tests/test_gpu_mfcc.py),
    where a mixed-precision filter would show first, and noise at levels 1 / 0.3 / 0.03 around a silent frame"""
    from scipy import signal as ss
    t = np.arange(1024) / 16000.0

    def filtered_noise(order, wn, seed, scale=1.0, kind="low"):
        bb, aa = ss.butter(order, wn, kind)
        return (scale * ss.lfilter(bb, aa, np.random.default_rng(seed).standard_normal(4096))[-1024:]).astype(np.float32)
    frames = [0.5 * np.sin(2 * np.pi * 500 * t), 0.5 * np.sin(2 * np.pi * 1500 * t), 0.5 * np.sin(2 * np.pi * 7900 * t), S.chirp(1024, 200.0, 7900.0),
              np.eye(1, 1024, 777)[0], np.full(1024, 0.7), np.concatenate([np.zeros(500), np.ones(524)]), filtered_noise(6, 0.1, 0),
              filtered_noise(8, 0.05, 1), filtered_noise(6, 0.2, 2, 5.0), filtered_noise(6, 0.97, 4, kind="high")]
    frames += [S.uniform_pm1(1024, 600 + i) * np.float32((1.0, 0.3, 0.03)[i % 3]) for i in range(6)]
    frames[13] = np.zeros(1024)
    return np.stack([np.asarray(v, np.float32) for v in frames])


PREFILTER_NAMES = ("htk128", "mels40_librosa_g6_fallback_mfcc16")      # the product bank, and a small one: two slots, the fallback placement, six pieces


@pytest.mark.parametrize("prefilter", [2, 1])
@pytest.mark.parametrize("name", PREFILTER_NAMES)
def test_prefilter_paths(torch_cuda, monkeypatch, name, prefilter):
    """both literal band-passes on four paths -- fused into the wave kernel, two passes by DSP_AMD_PREFILTER_TWO_PASS, frame length 800
    (two passes, the frame zero padded) and the Stockham kernel (two passes) -- each against the oracle with the same filter; where the
    plan cannot run the fused kernel the switch must not change a bit"""
    torch = torch_cuda
    x1024 = _prefilter_frames()

    def run(plan, x, two_pass):
        if two_pass:
            monkeypatch.setenv("DSP_AMD_PREFILTER_TWO_PASS", "1")
        else:
            monkeypatch.delenv("DSP_AMD_PREFILTER_TWO_PASS", raising=False)
        out = [_frames(torch, plan, x[:n].contiguous()).cpu().numpy() for n in (1, 8, 9, 17)]
        monkeypatch.delenv("DSP_AMD_PREFILTER_TWO_PASS", raising=False)
        return out

    for frame_length, kern, path in ((1024, 0, "wave"), (800, 0, "flen800"), (1024, 1, "stockham")):
        plan = _plan(name, frame_length, prefilter)
        plan.set_kernel(kern)
        frames = np.ascontiguousarray(x1024[:, :frame_length])
        x = torch.from_numpy(frames).cuda()
        ref = M.reference_frames(1024, name, frame_length, 0, frames, prefilter=prefilter)
        fused, two = run(plan, x, False), run(plan, x, True)
        for n, a, b in zip((1, 8, 9, 17), fused, two):
            if path == "wave":
                _gate(a, ref[:n], name, f"prefilter {prefilter} fused n{n}")
                _gate(b, ref[:n], name, f"prefilter {prefilter} two-pass n{n}")
            else:
                _gate(a, ref[:n], name, f"prefilter {prefilter} {path} n{n}")
                assert np.array_equal(a, b), f"{path}: the two-pass switch changed the result, so one of the runs took the fused kernel"
        assert not fused[3][13].any() and not two[3][13].any()         # the silent frame stays exactly zero through the filter
        if path == "wave":
            assert not np.array_equal(fused[3], two[3]), "the switch changed nothing: both runs took the same path"
        plan.set_kernel(0)


def test_refusals(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    plan = _plan("htk128", 1024)
    sig = torch.zeros(16384, dtype=torch.float32, device="cuda")
    pcm = torch.zeros(16384, dtype=torch.int16, device="cuda")
    with pytest.raises(dsp_amd.DspError, match="ragged MFCC matrices run on the 400-, 512- and 2048-point kernels: n_fft 1024 is not supported"):
        plan.clips_ragged(sig, [0, 8000, 16384], 1000)
    with pytest.raises(dsp_amd.DspError, match="ragged MFCC matrices run on the 400-, 512- and 2048-point kernels: n_fft 1024 is not supported"):
        plan.clips_ragged(pcm, [0, 8000, 16384], 1000)
    with pytest.raises(dsp_amd.DspError, match="PCM16 ingestion runs on the 512-point wave-per-frame kernel"):
        plan.clips_pcm16(pcm[None], 1000)
    pre = _plan("htk128", 1024, 2)
    with pytest.raises(dsp_amd.DspError, match="the per-frame prefilter applies to independent frames only"):
        pre.clips(sig[None], 1000)
    with pytest.raises(dsp_amd.DspError, match="ragged MFCC matrices: prefilter plans are not supported"):
        pre.clips_ragged(sig, [0, 8000, 16384], 1000)
    with pytest.raises(dsp_amd.DspError, match="DSP_LOG_GLOBAL_REF1 is implemented for n_fft = 512 and 2048"):
        dsp_amd.MfccPlan(M.config(1024, "htk128", 1024, 1))
    # the plans still work after every refusal
    x = torch.from_numpy(M.frames_input(1024, "htk128", 1024)[:9]).cuda()
    _gate(_frames(torch, plan, x).cpu().numpy(), _frame_refs("htk128", 1024)[:9], "htk128", "frames n9 after the refusals")
