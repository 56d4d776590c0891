"""GPU: the 400-point MFCC front end (mfcc400_kernel.hip; dsp_mfcc_speaker_config, DSP_FRAMING_CENTER) against the float64
restatement tests/mfcc400_ref.py under the project's pure gate -- independent frames, clips under both framings, ragged batches bit
for bit against one-clip calls, the entries that refuse a 400-point plan, and the chain from recorded speech to the float GMMs' LLR."""
import ctypes as C

import numpy as np
import pytest

from tests import enroll_ref as E
from tests import mfcc400_ref as R
from tests import signals as S
from tests import verify_ref as V
from tests.conftest import gate

pytestmark = pytest.mark.gpu

NO_CAP = 2**31 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _cfg(name, log_mode=None):
    import dsp_amd
    from dsp_amd import lib as dl
    over = {"speaker": {}, "mel40_20": dict(n_mels=40, n_mfcc=20), "htk128": dict(mel_norm=dl.MELNORM_NONE), "one_coef": dict(n_mfcc=1),
            "sr8000": dict(sample_rate=8000, fmax=4000.0)}[name]
    if log_mode is not None:
        over = dict(over, log_mode=log_mode)
    return dsp_amd.speaker_config(**over)


def _frames(n):
    """n seeded frames of 400 samples, the input classes in turn; from 3 frames on the middle one is all zeros"""
    rng = np.random.default_rng(4000 + n)
    k = np.arange(400)
    kinds = [lambda: rng.uniform(-1, 1, 400), lambda: 1e-4 * rng.uniform(-1, 1, 400), lambda: (k == 0).astype(float), lambda: np.ones(400),
             lambda: np.where(k % 2 == 0, 1.0, -1.0), lambda: (k == 399).astype(float), lambda: 0.5 * rng.uniform(-1, 1, 400)]
    x = np.stack([kinds[i % len(kinds)]() for i in range(n)]).astype(np.float32)
    if n >= 3:
        x[n // 2] = 0.0
    return x


@pytest.mark.parametrize("log_mode", [0, 1])
@pytest.mark.parametrize("name", ["speaker", "mel40_20", "htk128", "one_coef", "sr8000"])
def test_independent_frames(torch_cuda, name, log_mode):
    import dsp_amd
    torch = torch_cuda
    cfg = _cfg(name, log_mode)
    plan = dsp_amd.MfccPlan(cfg)
    for n in (1, 3, 5, 37):          # fewer than a block's four waves, one more than a block, an odd count across chunks
        x = _frames(n)
        got = plan.frames(torch.from_numpy(x).cuda()).cpu().numpy()
        want = R.frames_features(x, cfg)
        assert got.shape == want.shape == (n, cfg.n_mfcc)
        gate(got, want, f"mfcc400 frames {name} log{log_mode} n{n}")
        if n >= 3:                   # the silent frame: exact
            if log_mode == 0:
                assert not got[n // 2].any()
            else:
                assert abs(got[n // 2, 0] + 100.0 * np.sqrt(cfg.n_mels)) <= 1e-4 * 100.0 * np.sqrt(cfg.n_mels)
        if n == 5:
            host = plan.frames_host(x)
            assert np.array_equal(host, got)
    plan.close()


LENGTHS = [1, 159, 160, 161, 199, 200, 201, 399, 400, 401, 559, 560, 6129]
KINDS = ["noise", "chirp", "burst", "silent"]


def _clip(kind, n, seed):
    if kind == "noise":
        return S.uniform_pm1(n, seed).astype(np.float32)
    if kind == "chirp":
        return S.chirp(n, 100.0, 7000.0).astype(np.float32)
    x = np.zeros(n, np.float32)
    if kind == "burst":              # a burst between silences: the clip-wide top_db floor bites on the silent frames
        a, b = (n // 3, max(n // 3 + 1, 2 * n // 3))
        x[a:b] = np.float32(0.5) * S.uniform_pm1(b - a, seed + 1).astype(np.float32)
    return x


def _clips(n):
    return [_clip(kind, n, 100 * n + i) for i, kind in enumerate(KINDS)]


def _run_clips(torch, plan, clips, max_frames=NO_CAP, lead=8, tail=6):
    """one dsp_mfcc_clips_device call on clips of one length laid out with an even stride; NaN before the first clip and behind every clip
    inside its stride, so that any read outside a clip shows as a non-finite row -> numpy [n_clips][T][n_mfcc]"""
    from dsp_amd import lib as dl
    n = clips[0].size
    stride = n + (n & 1) + tail
    buf = np.full(lead + stride * len(clips), np.nan, np.float32)
    for i, x in enumerate(clips):
        buf[lead + i * stride: lead + i * stride + n] = x
    d = torch.from_numpy(buf).cuda()
    t = R.frames_for(plan.cfg, n, max_frames)
    out = torch.full((len(clips), max(t, 1), plan.cfg.n_mfcc), float("nan"), dtype=torch.float32, device="cuda")
    rc = plan._L.dsp_mfcc_clips_device(plan._h, d.data_ptr() + 4 * lead, len(clips), n, stride, out.data_ptr(), int(max_frames), None)
    assert rc == t, (rc, t, dl.last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()[:, :t]


@pytest.mark.parametrize("log_mode", [1, 0])
def test_clips_center_framing(torch_cuda, log_mode):
    """every length that puts the left padding, the right padding or both into the first and last frames"""
    import dsp_amd
    cfg = _cfg("speaker", log_mode)
    plan = dsp_amd.MfccPlan(cfg)
    for n in LENGTHS:
        clips = _clips(n)
        got = _run_clips(torch_cuda, plan, clips)
        assert got.shape == (len(clips), 1 + n // 160, 13)
        for kind, x, g in zip(KINDS, clips, got):
            gate(g, R.features(x, cfg), f"mfcc400 center log{log_mode} {kind} n{n}")
    # the cap and the host form
    clips = _clips(6129)
    got = _run_clips(torch_cuda, plan, clips, max_frames=5)
    assert got.shape[1] == 5
    for x, g in zip(clips, got):
        gate(g, R.features(x, cfg, 5), f"mfcc400 center log{log_mode} cap5")
    host = plan.clips_host(np.stack(_clips(561)), NO_CAP)
    assert np.array_equal(host, _run_clips(torch_cuda, plan, _clips(561)))
    plan.close()


def test_clips_complete_framing(torch_cuda):
    import dsp_amd
    from dsp_amd import lib as dl
    cfg = dsp_amd.speaker_config(framing=dl.FRAMING_COMPLETE)
    plan = dsp_amd.MfccPlan(cfg)
    for n, t in ((399, 0), (400, 1), (401, 1), (720, 3)):
        clips = _clips(n)
        got = _run_clips(torch_cuda, plan, clips)
        assert got.shape[1] == t
        for kind, x, g in zip(KINDS, clips, got):
            gate(g, R.features(x, cfg), f"mfcc400 complete {kind} n{n}")
    plan.close()


def _ragged_batch():
    clips = [x for n in LENGTHS for x in _clips(n)]
    clips.insert(7, np.zeros(0, np.float32))
    clips.insert(30, np.zeros(0, np.float32))
    clips.append(np.float32([0.25]))
    return clips


@pytest.mark.parametrize("which", ["speaker", "per_frame_max", "complete"])
def test_ragged_rows_are_the_one_clip_rows_bit_for_bit(torch_cuda, which):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    cfg = {"speaker": lambda: _cfg("speaker"), "per_frame_max": lambda: _cfg("speaker", 0),
           "complete": lambda: dsp_amd.speaker_config(framing=dl.FRAMING_COMPLETE)}[which]()
    plan = dsp_amd.MfccPlan(cfg)
    clips = _ragged_batch()
    start = 3                                                   # the batch starts at an odd sample; odd lengths: offsets of both parities
    offsets = np.concatenate([[start], start + np.cumsum([x.size for x in clips])]).astype(np.int64)
    assert (offsets % 2 == 0).any() and (offsets % 2 == 1).any()
    buf = np.full(int(offsets[-1]) + 5, np.nan, np.float32)
    for x, a in zip(clips, offsets):
        buf[a:a + x.size] = x
    sig = torch.from_numpy(buf).cuda()

    def alone(max_frames):
        rows = [plan.clips(torch.from_numpy(x[None]).cuda(), max_frames)[0] if R.frames_for(cfg, x.size, max_frames) else None for x in clips]
        return rows

    for max_frames in (NO_CAP, 2):
        want = alone(max_frames)
        for launch in ((0, 0), (1, 1), (2, 24)):
            plan.set_launch(*launch)
            mf, fo = plan.clips_ragged(sig, offsets, max_frames)
            assert fo.tolist() == np.concatenate([[0], np.cumsum([R.frames_for(cfg, x.size, max_frames) for x in clips])]).tolist()
            assert mf.shape == (fo[-1], 13) and bool(torch.isfinite(mf).all())
            for c, ref in enumerate(want):
                rows = mf[int(fo[c]):int(fo[c + 1])]
                assert rows.shape[0] == (0 if ref is None else ref.shape[0])
                if ref is not None:
                    assert torch.equal(rows, ref), f"{which} clip {c} (n = {clips[c].size}) launch {launch} max_frames {max_frames}"
        plan.set_launch(0, 0)
        if max_frames == 2:
            assert int(np.diff(fo).max()) == 2
    # and against the definition, once
    mf, fo = plan.clips_ragged(sig, offsets, NO_CAP)
    got = mf.cpu().numpy()
    for c in (0, 9, 25, len(clips) - 2, len(clips) - 1):
        if fo[c + 1] > fo[c]:
            gate(got[fo[c]:fo[c + 1]], R.features(clips[c], cfg), f"mfcc400 ragged {which} clip {c}")
    plan.close()


def _random_svm(rng, n_sv, n_features):
    return {"offset": rng.normal(0, 1, n_features), "scale": rng.uniform(0.5, 2, n_features), "sv": rng.normal(0, 1, (n_sv, n_features)),
            "coef": rng.normal(0, 1, n_sv), "kernel_params": [0.05], "rho": [0.1], "prob_a": [-1.0], "prob_b": [0.0]}


def test_entries_that_refuse_a_400_point_plan(torch_cuda, golden):
    import dsp_amd
    from dsp_amd import lib as dl
    from dsp_amd import scrubjay
    torch = torch_cuda
    plan = dsp_amd.MfccPlan(dsp_amd.speaker_config(log_mode=dl.LOG_PER_FRAME_MAX, framing=dl.FRAMING_COMPLETE))
    L = plan._L

    def refused(call):
        with pytest.raises(dsp_amd.DspError):
            call()
        assert "400" in dl.last_error(), dl.last_error()

    pcm = torch.zeros((2, 1600), dtype=torch.int16, device="cuda")
    sig = torch.zeros((2, 1600), dtype=torch.float32, device="cuda")
    refused(lambda: plan.clips_pcm16(pcm, 500))
    refused(lambda: plan.clips_ragged(pcm.reshape(-1), [0, 1600, 3200], 500))
    sj = scrubjay.ScrubJay(_random_svm(np.random.default_rng(1), 5, 26), config=plan.cfg)
    refused(lambda: sj(sig))
    refused(lambda: sj.pcm16(pcm))
    refused(lambda: sj.ragged(sig.reshape(-1), [0, 1600, 3200]))
    refused(lambda: scrubjay.ScrubJayScanner(sj))
    stop = dsp_amd.StopModel(dict(golden("stop_model.npz")))
    refused(lambda: stop.classify_signal_batch(plan, sig))
    refused(lambda: stop.classify_signal_ragged(plan, sig.reshape(-1), [0, 1600, 3200]))
    s = golden("speaker_gmm_ref.npz")
    spk = dsp_amd.SpeakerModel({k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")},
                               {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")})
    refused(lambda: dsp_amd.Scanner(plan, stop, spk))
    refused(lambda: dsp_amd.StreamSession(plan, 2, stop, spk))
    refused(lambda: dsp_amd.StreamSession(plan, 2))
    refused(lambda: plan.set_kernel(1))           # DSP_KERNEL_ROW
    refused(lambda: plan.set_kernel(2))
    plan.set_kernel(0)                            # the default stays accepted
    assert L.dsp_mfcc_lane_tables(C.byref(plan.cfg), None, 0) == -1 and "400" in dl.last_error()
    # the plan still works after every refusal
    x = _frames(5)
    gate(plan.frames(torch.from_numpy(x).cuda()).cpu().numpy(), R.frames_features(x, plan.cfg), "mfcc400 after refusals")


def test_speaker_front_end_refuses_short_clips_by_name(torch_cuda):
    import dsp_amd
    with dsp_amd.SpeakerFrontEnd() as fe:
        sig = torch_cuda.zeros(2000, dtype=torch_cuda.float32, device="cuda")
        with pytest.raises(ValueError, match="clip 1 has 399 samples"):
            fe.features(sig, [0, 800, 1199, 2000])
    assert fe.plan is None and fe.cmvn is None


def test_whole_chain_on_recorded_speech(torch_cuda, golden):
    """Four recorded clips -> SpeakerFrontEnd.features -> SpeakerVerifier.verify with the reference's target means as the one speaker.
    The MFCC rows against mfcc400_ref under gate(); the CMVN rows against enroll_ref's CMVN of the GPU's own MFCC rows under that file's
    gate (8 x its float32 model); the LLR and the UBM's log-likelihood against the float64 chain end to end under verify_ref.gates()'s
    rule with the float32 numpy model of the whole chain (there the floor 8 * 2^-23 * max |value| governs the log-likelihoods)."""
    import dsp_amd
    torch = torch_cuda
    z, g = golden("speaker_frontend_ref.npz"), golden("speaker_enroll_ref.npz")
    off = z["offsets"]
    assert off.tolist() == [0, 9471, 18328, 27943, 32710] and z["pcm"].dtype == np.int16
    x = (z["pcm"] / np.float32(32768.0)).astype(np.float32)
    ubm = {k: g[f"ubm_{k}_d"] for k in ("log_consts", "means", "inv_covs")}
    means = g["target_means_d"][None]
    fe = dsp_amd.SpeakerFrontEnd()
    cfg = fe.plan.cfg
    sig = torch.from_numpy(x).cuda()
    feats, fo = fe.features(sig, off)
    assert fo.tolist() == np.concatenate([[0], np.cumsum(1 + np.diff(off) // 160)]).tolist() and feats.shape == (fo[-1], 13)
    # 1. the MFCC rows
    mfcc, fo2 = fe.plan.clips_ragged(sig, off, NO_CAP)
    assert np.array_equal(fo, fo2)
    mfcc = mfcc.cpu().numpy()
    want_rows = [R.features(x[off[c]:off[c + 1]], cfg) for c in range(4)]
    for c in range(4):
        gate(mfcc[fo[c]:fo[c + 1]], want_rows[c], f"mfcc400 speech {str(z['names'][c])}")
    # 2. the CMVN of the GPU's own rows
    want = E.cmvn_ragged(mfcc, fo, 300)
    model = E.cmvn_ragged(mfcc, fo, 300, np.float32)
    cm_gate = E.GATE_FACTOR * float(np.abs(model - want).max())
    cm_err = float(np.abs(feats.cpu().numpy() - want).max())
    print(f"\nspeech chain: cmvn gate {cm_gate:.3e}, GPU vs float64 {cm_err:.3e}")
    assert cm_err <= cm_gate
    # 3. end to end
    def chain(dtype):
        rows = [E.cmvn(R.features(x[off[c]:off[c + 1]], cfg, dtype=dtype), 300, dtype) for c in range(4)]
        return V.verify(np.concatenate(rows), fo, ubm, means, dtype)
    w64, m32 = chain(np.float64), chain(np.float32)
    gates = V.gates(w64, m32)
    got = dsp_amd.SpeakerVerifier(ubm).verify(feats, fo, torch.from_numpy(means.astype(np.float32)).cuda(), want=("llr", "ll_ubm", "ll_target", "best"))
    for key in ("llr", "ll_ubm", "ll_target"):
        err = float(np.abs(got[key].cpu().numpy().astype(np.float64) - w64[key]).max())
        print(f"speech chain: {key} float64 {np.ravel(w64[key]).round(6).tolist()}, gate {gates[key]:.3e}, GPU vs float64 {err:.3e}")
    for key in ("llr", "ll_ubm", "ll_target"):
        assert float(np.abs(got[key].cpu().numpy().astype(np.float64) - w64[key]).max()) <= gates[key], key
    assert np.allclose(w64["llr"].ravel(), [-0.155063, 0.107779, -0.688120, 0.078314], atol=5e-7)
    assert not got["best"].cpu().numpy().any()
    fe.close()
