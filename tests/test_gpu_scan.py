"""GPU: scanning long recordings (dsp_scanner_*, dsp_stop_scan_device, dsp_speaker_scan_device).  Window w of a recording is rows
[w hop, w hop + window_frames) of its MFCC matrix, i.e. the clip of samples [w hop 160, + 400 + (window_frames - 1) 160) (the whole
recording when it has fewer rows than a window).  Every window's result must be the per-clip entry's on that cut-out clip: P("stop")
within 1e-6 of classify_signal's two-kernel path (MFCC matrix -> stop_tail_kernel, the same per-input arithmetic; the uniform batch entry,
since the ragged one runs on the fused kernel only), the speaker LLR exactly as dsp_speaker_llr_ragged_device, and a sample of both
against the oracle.  Every buffer is sized from the planner's window count."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
HOP, FRAME = 160, 400
NO_CAP = 2**31 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _gmms(golden):
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return s, t, u


def _windows(n_rows, wf, hop):
    """plain restatement of the window rule: [(first row, rows)] of one recording"""
    if n_rows < wf:
        return [(0, n_rows)]
    return [(w * hop, wf) for w in range(1 + (n_rows - wf) // hop)]


def _recordings(seed):
    """seeded lengths: the edge cases, a few of 1-30 s, one of 10 min; float32 noise with quiet and loud stretches"""
    rng = np.random.default_rng(seed)
    lens = [0, 399, 400, 15999, 16000] + rng.integers(16000, 30 * 16000, 4).tolist() + [10 * 60 * 16000]
    sigs = []
    for n in lens:
        x = rng.uniform(-1, 1, n).astype(np.float32)
        env = np.repeat(rng.uniform(0.001, 1.0, n // 4000 + 1).astype(np.float32), 4000)[:n]
        sigs.append((x * env).astype(np.float32))
    return lens, sigs


def _cut(sig, n_rows, w, wf, hop):
    """window w of a recording as its own clip (samples)"""
    if n_rows < wf:
        return sig
    a = w * hop * HOP
    return sig[a:a + FRAME + (wf - 1) * HOP]


def _check_rule(wo, fo, wf, hop):
    want = [0]
    for r in range(len(fo) - 1):
        want.append(want[-1] + len(_windows(int(fo[r + 1] - fo[r]), wf, hop)))
    assert wo.tolist() == want


def _picked(n_rows, wf, hop, rng):
    """every window of recordings up to 30 s; ~512 seeded windows plus the first and last of longer ones"""
    W = len(_windows(n_rows, wf, hop))
    if n_rows <= 30 * 100:
        return list(range(W))
    return sorted({0, W - 1} | set(rng.choice(W, size=min(512, W), replace=False).tolist()))


def _two_kernel_probs(torch, net, plan, clips, monkeypatch):
    """classify_signal per clip through the uniform batch entry's two-kernel path, clips grouped by length"""
    out = np.empty(len(clips), np.float32)
    by_len = {}
    for i, c in enumerate(clips):
        by_len.setdefault(c.size, []).append(i)
    monkeypatch.setenv("DSP_AMD_STOP_TWO_KERNELS", "1")
    try:
        for n, idx in by_len.items():
            n_eff = max(n, 1)            # a clip without samples has no rows, like any clip shorter than a frame
            for k in range(0, len(idx), 1024):
                part = idx[k:k + 1024]
                batch = np.zeros((len(part), n_eff + (n_eff & 1)), np.float32)
                for j, i in enumerate(part):
                    batch[j, :n] = clips[i]
                t = torch.from_numpy(batch).cuda()[:, :n_eff]
                out[part] = net.classify_signal_batch(plan, t).cpu().numpy()
    finally:
        monkeypatch.delenv("DSP_AMD_STOP_TWO_KERNELS")
    return out


def test_window_rows_are_the_cut_clips_rows(torch_cuda):
    """the premise: a window cut out as a clip has, bit for bit, the recording's rows"""
    import dsp_amd
    torch = torch_cuda
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    rng = np.random.default_rng(5)
    sig = rng.uniform(-1, 1, 7 * 16000 + 123).astype(np.float32)
    mf, fo = plan.clips_ragged(torch.from_numpy(sig).cuda(), [0, sig.size], NO_CAP)
    n_rows = int(fo[1])
    for wf, hop in ((98, 10), (98, 1), (300, 37)):
        for w in (0, 1, 5, len(_windows(n_rows, wf, hop)) - 1):
            clip = _cut(sig, n_rows, w, wf, hop)
            one = plan.clips(torch.from_numpy(np.ascontiguousarray(clip)).cuda()[None], NO_CAP)[0]
            assert torch.equal(one, mf[w * hop:w * hop + wf]), (wf, hop, w)


def test_reference_clips_reproduced(torch_cuda, golden):
    import dsp_amd
    torch = torch_cuda
    g = golden("stop_ref.npz")
    net = dsp_amd.StopModel(dict(golden("stop_model.npz")))
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    # the 7 reference clips are 16 000 samples = 100 hops: back to back, windows of 98 rows every 100 rows are the clips themselves
    rec = np.concatenate([(g[f"clip{i}__pcm"] / np.float32(32768.0)).astype(np.float32) for i in range(7)])
    want = np.array([g[f"clip{i}__prob"] for i in range(7)], np.float32)
    wo, prob, mean, label = dsp_amd.Scanner(plan, stop=net, window_frames=98, hop_frames=100).run(torch.from_numpy(rec).cuda(), [0, rec.size])
    assert wo.tolist() == [0, 7] and mean is None and label is None
    assert np.abs(prob.cpu().numpy() - want).max() <= 5e-5
    # the reference's own MFCC matrices, back to back, windows of 98 rows every 98: bit-exact LLR means and labels
    s, t, u = _gmms(golden)
    spk = dsp_amd.SpeakerModel(t, u)
    mf = np.concatenate([s[f"clip{i}__mfcc"] for i in range(4)])
    wo, m, lab = spk.scan(torch.from_numpy(mf).cuda(), [0, mf.shape[0]], 98, 98)
    assert wo.tolist() == [0, 4]
    assert m.cpu().numpy().tolist() == [int(s[f"clip{i}__llr_mean"]) for i in range(4)]
    assert lab.cpu().numpy().tolist() == [int(s[f"clip{i}__label"]) for i in range(4)]


@pytest.mark.parametrize("wf,hop", [(98, 1), (98, 7), (98, 98), (600, 7)])
def test_random_recordings_against_cut_clips(torch_cuda, golden, monkeypatch, wf, hop):
    import dsp_amd
    torch = torch_cuda
    m = dict(golden("stop_model.npz"))
    net = dsp_amd.StopModel(m)
    s, t, u = _gmms(golden)
    spk = dsp_amd.SpeakerModel(t, u)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    lens, sigs = _recordings(11)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    signal = torch.from_numpy(np.concatenate(sigs)).cuda()
    fo = dsp_amd.mfcc.ragged_frame_offsets(plan.cfg, offsets, NO_CAP)
    rows = np.diff(fo)
    wo, prob, mean, label = dsp_amd.Scanner(plan, stop=net, window_frames=wf, hop_frames=hop).run(signal, offsets)
    _check_rule(wo, fo, wf, hop)
    assert wo.tolist() == dsp_amd.scan_window_offsets(fo, wf, hop).tolist()
    assert prob.shape == (int(wo[-1]),) and mean is None and label is None
    prob = prob.cpu().numpy()
    # the speaker scan refuses recordings without rows: it runs on the others (speaker-only scanner)
    keep = [r for r in range(len(lens)) if rows[r] > 0]
    sub_off = np.concatenate([[0], np.cumsum([lens[r] for r in keep])]).astype(np.int64)
    sub = torch.from_numpy(np.concatenate([sigs[r] for r in keep])).cuda()
    swo, sprob, smean, slabel = dsp_amd.Scanner(plan, speaker=spk, window_frames=wf, hop_frames=hop).run(sub, sub_off)
    assert sprob is None and smean.shape == (int(swo[-1]),)
    smean, slabel = smean.cpu().numpy(), slabel.cpu().numpy()
    # both models in one scanner: the same numbers
    bwo, bprob, bmean, blabel = dsp_amd.Scanner(plan, stop=net, speaker=spk, window_frames=wf, hop_frames=hop).run(sub, sub_off)
    assert np.array_equal(bwo, swo) and np.array_equal(bmean.cpu().numpy(), smean) and np.array_equal(blabel.cpu().numpy(), slabel)
    sub_w = {r: int(swo[k]) for k, r in enumerate(keep)}
    bprob = bprob.cpu().numpy()
    rng = np.random.default_rng(wf * 1000 + hop)
    clips, where, spk_where = [], [], []
    for r in range(len(lens)):
        for w in _picked(int(rows[r]), wf, hop, rng):
            clips.append(_cut(sigs[r], int(rows[r]), w, wf, hop))
            where.append(int(wo[r]) + w)
            spk_where.append(sub_w[r] + w if r in sub_w else -1)
            if r in sub_w:
                assert bprob[sub_w[r] + w] == prob[int(wo[r]) + w]
    want = _two_kernel_probs(torch, net, plan, clips, monkeypatch)
    got = prob[where]
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    for i in rng.choice(len(clips), size=6, replace=False).tolist() + [0, len(clips) - 1]:
        assert abs(got[i] - O.classify_signal(m, clips[i])) <= 5e-5, i
    # speaker: the cut-out clips in one ragged MFCC call and the ragged LLR over them, exactly
    sk = [i for i in range(len(clips)) if spk_where[i] >= 0]
    cl = [clips[i] for i in sk]
    c_off = np.concatenate([[0], np.cumsum([c.size for c in cl])]).astype(np.int64)
    for k in range(0, len(cl), 2048):
        part = slice(k, min(k + 2048, len(cl)))
        buf = torch.from_numpy(np.concatenate(cl[part])).cuda()
        mf, cfo = plan.clips_ragged(buf, c_off[part.start:part.stop + 1] - c_off[part.start], NO_CAP)
        ref_mean, ref_label = spk.llr_ragged(mf, cfo)
        idx = [spk_where[i] for i in sk[part]]
        assert np.array_equal(ref_mean.cpu().numpy(), smean[idx]), (wf, hop, k)
        assert np.array_equal(ref_label.cpu().numpy(), slabel[idx]), (wf, hop, k)
        if k == 0:
            mfn = mf.cpu().numpy()
            for j in (0, len(idx) // 2, len(idx) - 1):
                assert O.speaker_llr_mean(t, u, mfn[int(cfo[j]):int(cfo[j + 1])]) == smean[idx[j]]


def test_pcm16_matches_float_path(torch_cuda, golden):
    import dsp_amd
    torch = torch_cuda
    net = dsp_amd.StopModel(dict(golden("stop_model.npz")))
    _s, t, u = _gmms(golden)
    spk = dsp_amd.SpeakerModel(t, u)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    sc = dsp_amd.Scanner(plan, stop=net, speaker=spk, window_frames=98, hop_frames=10)
    rng = np.random.default_rng(3)
    lens = [16000, 40001, 401, 123457]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pcm = rng.integers(-32768, 32768, (int(offsets[-1]), 2)).astype(np.int16)
    pcm[: 20000] //= 64
    mono = np.ascontiguousarray(pcm[:, 0])
    decoded = {
        "mono": (torch.from_numpy(mono).cuda(), 0, (mono / np.float32(32768.0)).astype(np.float32)),
        "ch0": (torch.from_numpy(pcm).cuda(), 0, (pcm[:, 0] / np.float32(32768.0)).astype(np.float32)),
        "avg": (torch.from_numpy(pcm).cuda(), 1, (np.float32(0.5) * (pcm[:, 0] / np.float32(32768.0) + pcm[:, 1] / np.float32(32768.0))).astype(np.float32)),
    }
    for name, (x, mode, f) in decoded.items():
        a = sc.run(x, offsets, stereo_mode=mode)
        b = sc.run(torch.from_numpy(f).cuda(), offsets)
        assert np.array_equal(a[0], b[0]), name
        for p, q in zip(a[1:], b[1:]):
            assert torch.equal(p, q), name


def test_empty_inputs_and_refusals(torch_cuda, golden):
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    net = dsp_amd.StopModel(dict(golden("stop_model.npz")))
    _s, t, u = _gmms(golden)
    spk = dsp_amd.SpeakerModel(t, u)
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    sc = dsp_amd.Scanner(plan, stop=net, speaker=spk)
    wo, prob, mean, label = sc.run(torch.zeros(8, device="cuda"), [0])
    assert wo.tolist() == [0] and prob.numel() == mean.numel() == label.numel() == 0
    lib = L.load()
    cfg = L.ScanConfig(98, 10)
    assert lib.dsp_scanner_run_device(sc._h, None, 0, None, None, None, None, None) == 0
    assert lib.dsp_stop_scan_device(net._h, None, 0, None, C.byref(cfg), None, None) == 0
    assert lib.dsp_speaker_scan_device(spk._h, None, 0, None, C.byref(cfg), None, None, None) == 0
    # a recording without rows: the speaker scan names it, nothing is launched
    x = torch.rand(40000, device="cuda")
    with pytest.raises(L.DspError, match="recording 1"):
        sc.run(x, [0, 20000, 20300, 40000])
    mf = torch.zeros((200, 13), device="cuda")
    with pytest.raises(L.DspError, match="recording 1"):
        spk.scan(mf, [0, 100, 100, 200], 98, 10)
    # plans whose rows depend on more than their own samples are refused
    sj = L.MfccConfig()
    lib.dsp_mfcc_scrubjay_infer_config(C.byref(sj), 16000)
    sj.n_mfcc = 13
    bad_cfgs = [dsp_amd.default_config(log_mode=L.LOG_GLOBAL_REF1), sj,
                dsp_amd.default_config(prefilter=L.PREFILTER_BUTTER_1000_3000)]
    for cfg_bad in bad_cfgs:
        bad = dsp_amd.MfccPlan(cfg_bad)
        with pytest.raises(L.DspError, match="rows do not depend on the window"):
            dsp_amd.Scanner(bad, stop=net)
    with pytest.raises(L.DspError):
        dsp_amd.Scanner(dsp_amd.MfccPlan(dsp_amd.default_config(n_mfcc=20)), speaker=spk)
    with pytest.raises(ValueError):
        dsp_amd.Scanner(plan)
