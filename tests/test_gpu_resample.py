"""GPU: the polyphase FIR resampler (dsp_resample_*, dsp_amd.Resampler) against the float64 restatement of its definition
(tests/resample_ref.py), under the rounding bound of a float32 dot product:

    |got[k] - ref[k]| <= (L_k + 2) 2^-24 sum_i |h x|       L_k = the terms of output k

(taps rounded once to float32, L_k products and sums in float32: it holds for any summation order, with or without FMA; the sequential
float32 model of resample_ref stays within 0.34 of it; the bound grows with the branch length, so the long branches -- and every
kernel form and tile geometry these seven ratios do not reach -- are held to the tighter rms gate of tests/resample_shapes.py in
tests/test_gpu_resample_shapes.py).  Then what must hold bit for bit: a recording's output does not depend on the
batch around it or on the entry it came through, int16 input is the float entry on the decoded samples, 16000 -> 16000 is the input.
The resampler exposes no launch geometry (its tiling is a function of the ratio alone), so there is none to vary.  Last, composition
with what follows it: MFCC rows of a resampled clip, and a Scanner run on the resampler's own (out, out_offsets)."""
import ctypes as C

import numpy as np
import pytest

from tests import resample_ref as R
from tests.conftest import gate
from tests.test_resample_cpu import COMPOSITION_CLIPS, composition_clip

pytestmark = pytest.mark.gpu
GPU_PAIRS = [(8000, 16000), (9000, 16000), (10000, 16000), (11025, 16000), (44100, 16000), (48000, 16000), (96000, 16000)]
LONG = 200003
FORMS = ("float", "mono", "stereo_ch0", "stereo_avg")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _signal(rng, n, form):
    """a recording in the caller's format and the float32 samples the kernels decode from it"""
    env = np.repeat(rng.uniform(0.01, 1.0, n // 500 + 1), 500)[:n]
    if form == "float":
        x = (rng.uniform(-1, 1, n) * env).astype(np.float32)
        return x, x
    shape = (n,) if form == "mono" else (n, 2)
    pcm = np.clip(np.rint(rng.uniform(-32768, 32767, shape) * (env if form == "mono" else env[:, None])), -32768, 32767).astype(np.int16)
    return pcm, R.decode_pcm16(pcm, 1 if form == "stereo_avg" else 0)


def _ragged(torch, sigs, form, lead=3):
    """the recordings back to back behind `lead` sample frames of filler (so that recordings start at every alignment) -> (tensor, offsets)"""
    filler = np.full((lead,) + sigs[0].shape[1:], 77, sigs[0].dtype)
    offs = np.concatenate([[lead], lead + np.cumsum([s.shape[0] for s in sigs])]).astype(np.int64)
    return torch.from_numpy(np.concatenate([filler] + list(sigs))).cuda(), offs


def _mode(form):
    return 1 if form == "stereo_avg" else 0


def _run_ragged(torch, rs, signal, offs, form):
    """through Resampler.ragged into a buffer with a NaN fence behind it"""
    total = int(R.offsets(rs.rate_in, rs.rate_out, offs)[-1])
    buf = torch.full((total + 8,), float("nan"), dtype=torch.float32, device="cuda")
    out, oo = rs.ragged(signal, offs, stereo_mode=_mode(form), out=buf)
    torch.cuda.synchronize()
    assert oo.tolist() == R.offsets(rs.rate_in, rs.rate_out, offs).tolist()
    assert bool(torch.isnan(buf[total:]).all()), "wrote past the last recording"
    return buf[:total], oo


@pytest.mark.parametrize("rate_in,rate_out", GPU_PAIRS)
def test_parity_with_the_float64_definition(torch_cuda, rate_in, rate_out):
    import dsp_amd
    torch = torch_cuda
    rs = dsp_amd.Resampler(rate_in, rate_out)
    up, down, half = R.ratio(rate_in, rate_out)
    assert (rs.up, rs.down, rs.half) == (up, down, half)
    lens = [0, 1, 7, half // up + 3, 997, LONG]
    worst = 0.0
    for f, form in enumerate(FORMS):
        rng = np.random.default_rng(1000 * f + rate_in)
        pairs = [_signal(rng, n, form) for n in lens]
        signal, offs = _ragged(torch, [p[0] for p in pairs], form)
        out, oo = _run_ragged(torch, rs, signal, offs, form)
        got_all = out.cpu().numpy()
        for c, (raw, x) in enumerate(pairs):
            ref, mag, terms = R.resample(x, rate_in, rate_out, with_bound=True)
            bound = (terms + 2) * 2.0 ** -24 * mag
            got = got_all[oo[c]:oo[c + 1]].astype(np.float64)
            assert got.shape == ref.shape == (R.out_len(lens[c], up, down),)
            clip = rs.clips(torch.from_numpy(raw[None]).cuda(), stereo_mode=_mode(form))
            assert clip.shape == (1, ref.size)
            got_clip = clip[0].cpu().numpy().astype(np.float64)
            for what, g in (("ragged", got), ("clips", got_clip)):
                err = np.abs(g - ref)
                assert np.all(np.isfinite(g)) and np.all(err <= bound), (rate_in, form, lens[c], what, float((err / np.where(bound > 0, bound, 1)).max()))
                if ref.size:
                    worst = max(worst, float((err / np.where(bound > 0, bound, np.inf)).max()))
    print(f"\nresample parity {rate_in} -> {rate_out}: worst |err| / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("rate_in", [10000, 44100, 48000])
@pytest.mark.parametrize("form", ["float", "stereo_avg"])
def test_a_recording_does_not_see_its_batch(torch_cuda, rate_in, form):
    """>= 40 recordings of mixed lengths in one launch == each resampled alone; the clips entry == the ragged entry"""
    import dsp_amd
    torch = torch_cuda
    rs = dsp_amd.Resampler(rate_in, 16000)
    rng = np.random.default_rng(rate_in + len(form))
    lens = [0, 1, 0, 5000, 2, 31, 0] + rng.integers(1, 30000, 36).tolist() + [0]
    assert len(lens) >= 40
    pairs = [_signal(rng, n, form) for n in lens]
    signal, offs = _ragged(torch, [p[0] for p in pairs], form)
    out, oo = _run_ragged(torch, rs, signal, offs, form)
    for c, (raw, _) in enumerate(pairs):
        one_sig, one_off = _ragged(torch, [raw], form, lead=c % 5)
        one, _ = _run_ragged(torch, rs, one_sig, one_off, form)
        assert torch.equal(one, out[oo[c]:oo[c + 1]]), (c, lens[c])
    # equal clips, a stride wider than the clips, an output stride wider than the outputs
    n, k = 4001, 6
    raws = [_signal(rng, n, form)[0] for _ in range(k)]
    wide = torch.zeros((k, n + 6) + raws[0].shape[1:], dtype=torch.from_numpy(raws[0]).dtype, device="cuda")
    wide[:, :n] = torch.from_numpy(np.stack(raws)).cuda()
    n_out = rs.out_samples(n)
    wide_out = torch.full((k, n_out + 3), float("nan"), dtype=torch.float32, device="cuda")
    got = rs.clips(wide[:, :n], stereo_mode=_mode(form), out=wide_out[:, :n_out])
    rag_sig, rag_off = _ragged(torch, raws, form, lead=1)
    rag, roo = _run_ragged(torch, rs, rag_sig, rag_off, form)
    assert bool(torch.isnan(wide_out[:, n_out:]).all())
    for c in range(k):
        assert torch.equal(got[c], rag[roo[c]:roo[c + 1]]), c


@pytest.mark.parametrize("rate_in", [9000, 11025, 48000, 96000, 16000])
def test_int16_forms_are_the_float_entry_on_the_decoded_samples(torch_cuda, rate_in):
    import dsp_amd
    torch = torch_cuda
    rs = dsp_amd.Resampler(rate_in, 16000)
    for f, form in enumerate(FORMS[1:]):
        rng = np.random.default_rng(7 * rate_in + f)
        pairs = [_signal(rng, n, form) for n in (0, 1, 9, 1234, 40001)]
        sig_i, off_i = _ragged(torch, [p[0] for p in pairs], form, lead=f + 1)
        sig_f, off_f = _ragged(torch, [p[1] for p in pairs], "float", lead=2 * f)
        out_i, _ = _run_ragged(torch, rs, sig_i, off_i, form)
        out_f, _ = _run_ragged(torch, rs, sig_f, off_f, "float")
        assert torch.equal(out_i, out_f), form
        clips_i = rs.clips(torch.from_numpy(np.stack([pairs[3][0], pairs[3][0][::-1].copy()])).cuda(), stereo_mode=_mode(form))
        clips_f = rs.clips(torch.from_numpy(np.stack([pairs[3][1], pairs[3][1][::-1].copy()])).cuda())
        assert torch.equal(clips_i, clips_f), form


def test_equal_rates_return_the_input_bit_for_bit(torch_cuda):
    import dsp_amd
    torch = torch_cuda
    rs = dsp_amd.Resampler(16000, 16000)
    assert (rs.up, rs.down) == (1, 1)
    x = np.random.default_rng(11).uniform(-1, 1, 70001).astype(np.float32)
    x[:4] = [-0.0, np.float32(1e-42), np.inf, np.nan]                   # a copy keeps what no filter would
    offs = [0, 0, 5, 4100, 70001]
    out, oo = rs.ragged(torch.from_numpy(x).cuda(), offs)
    assert oo.tolist() == offs
    assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32))
    clips = rs.clips(torch.from_numpy(x[:70000].reshape(7, 10000)).cuda())
    assert np.array_equal(clips.cpu().numpy().view(np.uint32), x[:70000].reshape(7, 10000).view(np.uint32))


def test_host_entry_and_zero_recordings(torch_cuda):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    L = dl.load()
    x = np.random.default_rng(12).uniform(-1, 1, 12345).astype(np.float32)
    rs = dsp_amd.Resampler(44100, 16000)
    want, _ = rs.ragged(torch.from_numpy(x).cuda(), [0, x.size])
    got = np.full(rs.out_samples(x.size), np.nan, np.float32)
    assert L.dsp_resample_host(44100, 16000, x.ctypes.data, x.size, got.ctypes.data) == 0, dl.last_error()
    assert np.array_equal(got, want.cpu().numpy())
    # zero recordings and recordings without samples: DSP_OK, nothing written
    out, oo = rs.ragged(torch.zeros(0, device="cuda"), [0])
    assert out.numel() == 0 and oo.tolist() == [0]
    fence = torch.full((4,), float("nan"), device="cuda")
    off = (C.c_long * 3)(2, 2, 2)
    assert L.dsp_resample_ragged_device(rs._h, fence.data_ptr(), 2, off, fence.data_ptr(), None) == 0
    assert L.dsp_resample_ragged_device(rs._h, None, 0, None, None, None) == 0
    assert L.dsp_resample_clips_device(rs._h, None, 0, 100, 100, None, 37, None) == rs.out_samples(100)
    torch.cuda.synchronize()
    assert bool(torch.isnan(fence).all())
    assert rs.clips(torch.zeros((3, 0), device="cuda")).shape == (3, 0)


@pytest.mark.parametrize("name", COMPOSITION_CLIPS)
def test_mfcc_of_a_resampled_clip(torch_cuda, golden, name):
    """a golden 16 kHz clip upsampled x 3 in float64 here, 48 kHz -> 16 kHz on the GPU, then MfccPlan.clips: against MfccPlan.clips of the
    float64 resampling, under the 1e-4-of-frame-L-inf gate (tests/test_resample_cpu.py holds the float32 model to it on these clips)"""
    import dsp_amd
    torch = torch_cuda
    x48 = R.resample(composition_clip(golden, name), 16000, 48000).astype(np.float32)
    want16 = R.resample(x48, 48000, 16000).astype(np.float32)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    got16 = dsp_amd.Resampler(48000, 16000).clips(torch.from_numpy(x48[None]).cuda())
    assert got16.shape == (1, 16000)
    got = plan.clips(got16, 98).cpu().numpy()
    want = plan.clips(torch.from_numpy(want16[None]).cuda(), 98).cpu().numpy()
    gate(got, want, f"resample_then_mfcc_{name}")


def test_scanner_takes_the_resamplers_output_and_offsets(torch_cuda, golden):
    """the offsets contract, not a numeric claim: Scanner.run(out, out_offsets) == Scanner.run on a copy of the same samples with the
    offsets counted here"""
    import dsp_amd
    torch = torch_cuda
    s = golden("speaker_gmm_ref.npz")
    spk = dsp_amd.SpeakerModel({k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}, {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")})
    net = dsp_amd.StopModel(dict(golden("stop_model.npz")))
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    sc = dsp_amd.Scanner(plan, stop=net, speaker=spk, window_frames=98, hop_frames=10)
    rng = np.random.default_rng(13)
    lens = [48000 * 3 + 1, 1200, 48000 * 2, 48000 + 17]                  # (every recording keeps at least one MFCC frame: 400 samples at 16 kHz)
    pcm = [_signal(rng, n, "mono")[0] for n in lens]
    signal, offs = _ragged(torch, pcm, "mono", lead=5)
    out, oo = dsp_amd.Resampler(48000, 16000).ragged(signal, offs)
    assert np.diff(oo).tolist() == [-(-n // 3) for n in lens]
    a = sc.run(out, oo)
    direct = torch.from_numpy(out.cpu().numpy().copy()).cuda()
    b = sc.run(direct, np.concatenate([[0], np.cumsum([-(-n // 3) for n in lens])]))
    assert a[0].tolist() == b[0].tolist() and a[0][-1] > 0
    for u, v in zip(a[1:], b[1:]):
        assert torch.equal(u, v)
