"""GPU: ragged MFCC matrices (dsp_mfcc_clips_ragged_device / _pcm16_device) and the speaker LLR over them
(dsp_speaker_llr_ragged_device).  Clips of different lengths back to back in one buffer, one launch; clip c's rows must be, bit for
bit, what a one-clip call with the same plan and max_frames returns -- and against the compiled reference's goldens through gate()."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import signals as S
from tests.conftest import LOW_LEVEL_CASES, gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _golden_cases(g):
    c = S.mfcc_cases()
    c["chirp"] = g["input__chirp"]
    bird = g["birdq_pcm"]
    c["birdq_ch0"] = (bird[:, 0] / np.float32(32768.0)).astype(np.float32)
    c["birdq_avg"] = (np.float32(0.5) * (bird[:, 0] / np.float32(32768.0) + bird[:, 1] / np.float32(32768.0))).astype(np.float32)
    c["stop_121417"] = (g["stop_pcm"] / np.float32(32768.0)).astype(np.float32)
    return c


GOLDEN = ["noise0", "noise1", "noise2", "chirp", "silence", "tiny", "dc", "impulse", "half_silent",
          "len399", "len400", "len559", "len560", "long", "birdq_ch0", "birdq_avg", "stop_121417"]


def _lengths(seed, n=40):
    """seeded clip lengths 0 .. 52 000 with the edge cases; odd lengths, so later clips start at odd samples"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 52000, n).tolist()
    lens[:8] = [399, 400, 0, 401, 16001, 559, 1, 160 * 99 + 241]
    rng.shuffle(lens)
    return [int(v) for v in lens]


def _offsets(lens, start=0):
    return np.concatenate([[start], start + np.cumsum(lens)]).astype(np.int64)


def _check_against_one_clip_calls(torch, mf, fo, offsets, one_clip):
    assert mf.shape[0] == fo[-1]
    for c in range(len(offsets) - 1):
        ref = one_clip(int(offsets[c]), int(offsets[c + 1]))
        got = mf[int(fo[c]):int(fo[c + 1])]
        assert got.shape[0] == (0 if ref is None else ref.shape[0]), c
        if ref is not None and ref.shape[0]:
            assert torch.equal(got, ref), f"clip {c}: not bit for bit the one-clip call"


def _float_one_clip(torch, plan, sig, max_frames):
    def run(a, b):
        x = sig[a:b].clone()[None]                        # its own (aligned) buffer
        if plan.cfg.framing == 0 and b - a < plan.cfg.frame_length:
            return None
        return plan.clips(x, max_frames)[0]
    return run


def test_golden_signals_in_one_ragged_call(torch_cuda, golden):
    import dsp_amd
    torch = torch_cuda
    g = golden("mfcc_ref.npz")
    cases = _golden_cases(g)
    sigs = [np.ascontiguousarray(cases[n], np.float32) for n in GOLDEN]
    offsets = _offsets([s.size for s in sigs])
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    mf, fo = plan.clips_ragged(torch.from_numpy(np.concatenate(sigs)).cuda(), offsets, 500)
    got = mf.cpu().numpy()
    for c, name in enumerate(GOLDEN):
        ref = g["mfcc__" + name]
        rows = got[fo[c]:fo[c + 1]]
        assert rows.shape == ref.shape, name
        if name == "len399":
            assert rows.shape[0] == 0
            continue
        gate(rows, ref, f"ragged/golden/{name}", floor_case=name if name in LOW_LEVEL_CASES else None)


@pytest.mark.parametrize("max_frames", [500, 37])
def test_seeded_clips_bitwise_equal_one_clip_calls(torch_cuda, max_frames):
    import dsp_amd
    torch = torch_cuda
    lens = _lengths(11)
    offsets = _offsets(lens)
    sig = torch.from_numpy(S.uniform_pm1(int(offsets[-1]), 5) * np.float32(0.7)).cuda()
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    mf, fo = plan.clips_ragged(sig, offsets, max_frames)
    assert np.array_equal(fo, dsp_amd.mfcc.ragged_frame_offsets(plan.cfg, offsets, max_frames))
    _check_against_one_clip_calls(torch, mf, fo, offsets, _float_one_clip(torch, plan, sig, max_frames))
    # the per-frame epilogue kernel too
    plan.set_kernel(2)
    mf2, _ = plan.clips_ragged(sig, offsets, max_frames)
    _check_against_one_clip_calls(torch, mf2, fo, offsets, _float_one_clip(torch, plan, sig, max_frames))


@pytest.mark.parametrize("layout", ["mono", "stereo_ch0", "stereo_avg"])
@pytest.mark.parametrize("max_frames", [500, 37])
def test_pcm16_clips_bitwise_equal_one_clip_calls(torch_cuda, layout, max_frames):
    import dsp_amd
    torch = torch_cuda
    lens = _lengths(12)
    offsets = _offsets(lens)
    rng = np.random.default_rng(3)
    ch = 1 if layout == "mono" else 2
    pcm = rng.integers(-32768, 32768, (int(offsets[-1]), ch), dtype=np.int16)
    pcm_d = torch.from_numpy(pcm[:, 0].copy() if ch == 1 else pcm).cuda()
    mode = 1 if layout == "stereo_avg" else 0
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    mf, fo = plan.clips_ragged(pcm_d, offsets, max_frames, stereo_mode=mode)

    def one(a, b):
        if b - a < plan.cfg.frame_length:
            return None
        return plan.clips_pcm16(pcm_d[a:b].clone()[None], max_frames, stereo_mode=mode)[0]
    _check_against_one_clip_calls(torch, mf, fo, offsets, one)


def _scrubjay_cfg():
    from dsp_amd.scrubjay import scrubjay_infer_config
    return scrubjay_infer_config(16000)


def _ref1_512():
    import dsp_amd
    from dsp_amd.lib import LOG_GLOBAL_REF1
    return dsp_amd.default_config(frame_length=512, hop_length=160, win_length=400, mel_norm=1, log_mode=LOG_GLOBAL_REF1)


def _ref1_2048():
    import dsp_amd
    from dsp_amd.lib import LOG_GLOBAL_REF1, MELNORM_LIBROSA
    return dsp_amd.default_config(n_fft=2048, frame_length=2048, hop_length=512, n_mels=128, n_mfcc=20, fmin=0.0, fmax=8000.0,
                                  mel_norm=MELNORM_LIBROSA, log_mode=LOG_GLOBAL_REF1)


@pytest.mark.parametrize("which", ["scrubjay_infer", "global_ref1_512", "global_ref1_2048"])
def test_other_plans_bitwise_equal_one_clip_calls(torch_cuda, which):
    import dsp_amd
    torch = torch_cuda
    cfg = {"scrubjay_infer": _scrubjay_cfg, "global_ref1_512": _ref1_512, "global_ref1_2048": _ref1_2048}[which]()
    lens = _lengths(13, 30)
    offsets = _offsets(lens, start=3)          # the batch itself starts at an odd sample
    sig = torch.from_numpy(S.uniform_pm1(int(offsets[-1]) + 5, 6) * np.float32(0.5)).cuda()
    sig[3 + lens[0]: 3 + lens[0] + 2000] *= 1e-3          # clips of different levels: the GLOBAL_REF1 floor is per clip
    plan = dsp_amd.MfccPlan(cfg)
    for max_frames in (500, 37):
        mf, fo = plan.clips_ragged(sig, offsets, max_frames)
        _check_against_one_clip_calls(torch, mf, fo, offsets, _float_one_clip(torch, plan, sig, max_frames))
    if which == "scrubjay_infer":        # int16 PCM on the same front end
        rng = np.random.default_rng(4)
        pcm = torch.from_numpy(rng.integers(-32768, 32768, int(offsets[-1]) + 5, dtype=np.int16)).cuda()
        mf, fo = plan.clips_ragged(pcm, offsets, 500)

        def one(a, b):
            return None if b == a else plan.clips_pcm16(pcm[a:b].clone()[None], 500)[0]
        _check_against_one_clip_calls(torch, mf, fo, offsets, one)


def test_twenty_thousand_clips_of_sixteen_lengths(torch_cuda):
    """Many clips per chunk and many chunks per wave: compared, length group by length group, with one uniform call per group."""
    import dsp_amd
    torch = torch_cuda
    rng = np.random.default_rng(21)
    distinct = rng.integers(8000, 24001, 16)
    lens = np.repeat(distinct, 1250)
    rng.shuffle(lens)
    offsets = _offsets(lens.tolist())
    gen = torch.Generator(device="cuda").manual_seed(9)
    sig = torch.rand(int(offsets[-1]), generator=gen, device="cuda") * 2 - 1
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    mf, fo = plan.clips_ragged(sig, offsets, 500)
    fo_d = torch.from_numpy(fo).cuda()
    off_d = torch.from_numpy(offsets).cuda()
    for L in distinct:
        idx = torch.from_numpy(np.nonzero(lens == L)[0]).cuda()
        cols = off_d[idx][:, None] + torch.arange(int(L), device="cuda")[None]
        grp = torch.zeros((idx.numel(), int(L) + int(L) % 2), device="cuda")    # the uniform entry takes an even clip stride
        grp[:, :int(L)] = sig[cols]
        ref = plan.clips(grp[:, :int(L)], 500)                               # [n_group][T][13]
        t = ref.shape[1]
        rows = fo_d[idx][:, None] + torch.arange(t, device="cuda")[None]
        assert torch.equal(fo_d[idx + 1] - fo_d[idx], torch.full_like(idx, t))
        assert torch.equal(mf[rows], ref), f"length {int(L)}"


def _gmms(golden):
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return t, u


def test_speaker_llr_over_a_ragged_matrix(torch_cuda, golden):
    import dsp_amd
    torch = torch_cuda
    t, u = _gmms(golden)
    spk = dsp_amd.SpeakerModel(t, u)
    lens = _lengths(11)
    offsets = _offsets(lens)
    sig = torch.from_numpy(S.uniform_pm1(int(offsets[-1]), 5) * np.float32(0.7)).cuda()
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    mf, fo = plan.clips_ragged(sig, offsets, 500)
    keep = np.nonzero(np.diff(fo) > 0)[0]
    fo_k = np.concatenate([[0], fo[keep + 1]])           # clips with >= 1 frame: their rows are back to back already
    mean, label, lt, lu = spk.llr_ragged(mf, fo_k, per_frame=True)
    mf_h = mf.cpu().numpy()
    for j, c in enumerate(keep):
        rows = mf[int(fo[c]):int(fo[c + 1])]
        m1, l1, t1, u1 = spk.llr(rows[None].contiguous(), per_frame=True)
        assert int(mean[j]) == int(m1[0]) and int(label[j]) == int(l1[0]), c
        assert torch.equal(lt[int(fo[c]):int(fo[c + 1])], t1[0]) and torch.equal(lu[int(fo[c]):int(fo[c + 1])], u1[0]), c
        if j < 4:                                          # and against the CPU oracle
            x = mf_h[fo[c]:fo[c + 1]]
            assert int(mean[j]) == O.speaker_llr_mean(t, u, x) and int(label[j]) == O.classify_speaker(t, u, x)
    # without the per-frame outputs
    mean2, label2 = spk.llr_ragged(mf, fo_k)
    assert torch.equal(mean2, mean) and torch.equal(label2, label)
    # a clip without frames has no mean: refused, and the message names it
    with pytest.raises(dsp_amd.DspError, match="clip 1"):
        spk.llr_ragged(mf, [0, 5, 5, 9])


def test_rejections(torch_cuda):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    L = dl.load()
    sig = torch.zeros(64000, dtype=torch.float32, device="cuda")
    out = torch.empty((1000, 20), dtype=torch.float32, device="cuda")
    off, n = dl.c_offsets([0, 16000, 32000])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cfg, word in ((dsp_amd.default_config(n_fft=1024, frame_length=1024, hop_length=1024, n_mels=128), "1024"),
                      (dsp_amd.default_config(n_fft=1024, frame_length=1024, hop_length=1024, n_mels=128, prefilter=1), "prefilter")):
        plan = dsp_amd.MfccPlan(cfg)
        assert L.dsp_mfcc_clips_ragged_device(plan._h, sig.data_ptr(), n, off, 500, out.data_ptr(), stream) == -1
        assert word in dl.last_error()
        with pytest.raises(dsp_amd.DspError):
            plan.clips_ragged(sig, [0, 16000, 32000], 500)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    assert L.dsp_mfcc_clips_ragged_device(plan._h, sig.data_ptr() + 4, n, off, 500, out.data_ptr(), stream) == -1     # misaligned
    assert "aligned" in dl.last_error()
    pcm = torch.zeros(64000, dtype=torch.int16, device="cuda")
    assert L.dsp_mfcc_clips_ragged_pcm16_device(plan._h, pcm.data_ptr() + 2, n, off, 1, 0, 500, out.data_ptr(), stream) == -1
    assert "aligned" in dl.last_error()
    assert L.dsp_mfcc_clips_ragged_device(plan._h, None, n, off, 500, out.data_ptr(), stream) == -1
    assert "NULL" in dl.last_error()
    off_bad, n_bad = dl.c_offsets([0, 16000, 15000])
    assert L.dsp_mfcc_clips_ragged_device(plan._h, sig.data_ptr(), n_bad, off_bad, 500, out.data_ptr(), stream) == -1
    assert "non-decreasing" in dl.last_error()
    torch.cuda.synchronize()
