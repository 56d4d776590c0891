"""GPU: scrub-jay scans of long recordings (dsp_scrubjay_scanner_*, dsp_svm_scan_device).  Window w of a recording is the clip
dsp_scan_window_spans gives; every window's label, decision value, P(label 1) and pooled features must equal, bit for bit,
dsp_scrubjay_fused_ragged_device (ScrubJay.ragged) on that clip cut out -- for the three front ends the scanner accepts: the
reference's 512-point framing with 20 coefficients (BASELINE config 5), scrubjay_infer.c's own aubio front end (stream framing: each
window's head row computed from the window's own samples) and its 2048 / 1024 numbers on complete frames.  The matrix-level scan
equals mean | std -> SVM on the rows gathered per window, on random SVMs of several shapes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NO_CAP = 2**31 - 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _attrs(golden):
    m = golden("scrubjay_svm.npz")
    return {k: m[k] for k in m.files}


def _config(name, sr=16000):
    import dsp_amd
    from dsp_amd import scrubjay
    if name == "512":
        return dsp_amd.default_config(n_mfcc=20)
    return scrubjay.scrubjay_infer_config(sr, aubio=name == "aubio")


def _recordings(cfg, wf, hf, seed):
    """seeded lengths: one frame, one window, one window + one hop, a few of 1-20 s, one of 60 s; noise with quiet and loud stretches"""
    rng = np.random.default_rng(seed)
    hop, frame = cfg.hop_length, cfg.frame_length
    one = wf * hop if cfg.framing == 1 else frame + (wf - 1) * hop
    lens = [frame, one, one + hf * hop, 1] + rng.integers(16000, 20 * 16000, 3).tolist() + [60 * 16000]
    lens = [n for n in lens if n >= (1 if cfg.framing == 1 else frame)]
    sigs = []
    for n in lens:
        x = rng.uniform(-1, 1, n).astype(np.float32)
        env = np.repeat(rng.uniform(0.001, 1.0, n // 4000 + 1).astype(np.float32), 4000)[:n]
        sigs.append((x * env).astype(np.float32))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(sigs)


def _cut_out(torch, x, starts, lengths):
    """the windows as their own clips, back to back: (buffer, offsets)"""
    idx = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, lengths)])
    return x[torch.from_numpy(idx).to(x.device)].contiguous(), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _equal(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch_equal(a, b), (what, ["labels", "decision", "prob1", "feat"][i])


def torch_equal(a, b):
    import torch
    return torch.equal(a, b)


@pytest.mark.parametrize("name", ["512", "aubio", "2048"])
@pytest.mark.parametrize("wf,hf", [(16, 4), (16, 1), (98, 10), (100000, 3)])
def test_scanner_equals_the_cut_out_windows(torch_cuda, golden, name, wf, hf):
    torch = torch_cuda
    from dsp_amd import scrubjay
    cfg = _config(name)
    sj = scrubjay.ScrubJay(_attrs(golden), config=cfg)
    sc = scrubjay.ScrubJayScanner(sj, wf, hf)
    offsets, x = _recordings(cfg, wf, hf, 11 * wf + hf)
    xd = torch.from_numpy(x).cuda()
    wo, *got = sc.run(xd, offsets)
    starts, lengths = scrubjay.scan_window_spans(cfg, offsets, wf, hf)
    assert wo[-1] == starts.size == got[0].shape[0] and got[3].shape == (starts.size, 40)
    cut, coff = _cut_out(torch, xd, starts, lengths)
    _equal(got, sj.ragged(cut, coff), (name, wf, hf))
    # the same scanner again (grown workspace kept) and a recording alone give the same windows
    _equal(sc.run(xd, offsets)[1:], got, "rerun")
    r = len(offsets) - 2
    alone = sc.run(xd[int(offsets[r]):int(offsets[r + 1])].clone(), [0, int(offsets[r + 1] - offsets[r])])
    _equal(alone[1:], [t[int(wo[r]):int(wo[r + 1])] for t in got], "alone")


@pytest.mark.parametrize("name", ["512", "aubio"])
def test_pcm16_equals_the_float_scanner(torch_cuda, golden, name):
    """int16 mono, stereo channel 0 and stereo average against the float scanner on the converted samples.  The ragged MFCC matrix takes
    int16 on the aubio front end and on the 512-point framing's 13-coefficient shape: there with a random SVM of 26 features."""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(5)
    if name == "512":
        sj = scrubjay.ScrubJay(_random_svm(rng, 40, 13), n_mfcc=13)
    else:
        sj = scrubjay.ScrubJay(_attrs(golden), config=_config(name))
    sc = scrubjay.ScrubJayScanner(sj, 16, 4)
    lens = [16000, 40001, 2048, 123457]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pcm = rng.integers(-32768, 32768, (int(offsets[-1]), 2)).astype(np.int16)
    pcm[:20000] //= 64
    mono = np.ascontiguousarray(pcm[:, 0])
    decoded = {
        "mono": (torch.from_numpy(mono).cuda(), 0, (mono / np.float32(32768.0)).astype(np.float32)),
        "ch0": (torch.from_numpy(pcm).cuda(), dsp_amd.STEREO_CHANNEL0, (pcm[:, 0] / np.float32(32768.0)).astype(np.float32)),
        "avg": (torch.from_numpy(pcm).cuda(), dsp_amd.STEREO_AVERAGE,
                ((pcm[:, 0].astype(np.float32) + pcm[:, 1].astype(np.float32)) / np.float32(65536.0)).astype(np.float32)),
    }
    for mode_name, (x, mode, f) in decoded.items():
        a = sc.run(x, offsets, stereo_mode=mode)
        b = sc.run(torch.from_numpy(f).cuda(), offsets)
        assert np.array_equal(a[0], b[0])
        _equal(a[1:], b[1:], (name, mode_name))
    if name == "512":                      # config 5's 20 coefficients: int16 is refused before any launch
        from dsp_amd import lib as dl
        c5 = scrubjay.ScrubJayScanner(scrubjay.ScrubJay(_attrs(golden), config=_config("512")), 16, 4)
        with pytest.raises(dl.DspError, match="int16 input"):
            c5.run(decoded["mono"][0], offsets)


def _random_svm(rng, n_sv, n_coef):
    nf = 2 * n_coef
    return {"offset": rng.normal(0, 3, nf).astype(np.float32), "scale": rng.uniform(0.05, 0.5, nf).astype(np.float32),
            "sv": rng.normal(0, 1, (n_sv, nf)).astype(np.float32), "coef": rng.normal(0, 1, n_sv).astype(np.float32),
            "kernel_params": np.array([1.0 / nf, 0.0, 3.0], np.float32), "rho": np.array([rng.normal(0, 0.5)], np.float32),
            "prob_a": np.array([-rng.uniform(0.5, 3)], np.float32), "prob_b": np.array([rng.normal(0, 0.3)], np.float32)}


@pytest.mark.parametrize("n_coef", [13, 20, 32])
@pytest.mark.parametrize("n_sv", [1, 55, 64, 65, 300])
def test_matrix_scan_equals_stats_then_predict(torch_cuda, n_sv, n_coef):
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    rng = np.random.default_rng(1000 * n_sv + n_coef)
    svm = scrubjay.SvmModel(_random_svm(rng, n_sv, n_coef))
    rows = [1, 5, 16, 20, 98, 108, 300, 1300, 2]
    fo = np.concatenate([[7], 7 + np.cumsum(rows)]).astype(np.int64)
    mfcc = torch.from_numpy((rng.normal(0, 8, (int(fo[-1]) + 3, n_coef))).astype(np.float32)).cuda()
    # (600, 50): one window per block with rows read from memory when n_coef = 32
    for wf, hf in ((16, 4), (98, 10), (7, 3), (5000, 1), (600, 50), (1, 1)):
        wo, *got = svm.scan(mfcc, fo, wf, hf)
        assert np.array_equal(wo, dsp_amd.scan_window_offsets(fo, wf, hf))
        want = [torch.empty_like(t) for t in got]
        groups = {}
        for r in range(len(rows)):
            n = min(rows[r], wf)
            for w in range(int(wo[r + 1] - wo[r])):
                groups.setdefault(n, []).append((int(wo[r]) + w, int(fo[r]) + w * hf))
        for n, items in groups.items():
            g = torch.tensor([i for i, _ in items], device="cuda")
            idx = torch.tensor([[a + t for t in range(n)] for _, a in items], device="cuda")
            feat = scrubjay.mfcc_stats(mfcc[idx])
            for dst, src in zip(want, svm.predict(feat) + (feat,)):
                dst[g] = src
        _equal(got, want, (n_sv, n_coef, wf, hf))


def test_reference_recordings(torch_cuda, golden):
    """The two labelled recordings of the reference (tests/golden/labelled_audio.npz, 96 kHz stereo int16) through the aubio front end,
    channels averaged: one window over the whole file is the file's own result; sliding windows equal their cut-outs."""
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import scrubjay
    g = golden("labelled_audio.npz")
    for name in ("sj_short", "not_sj"):
        pcm, sr = g[f"{name}__pcm"], int(g[f"{name}__sr"])
        cfg = _config("aubio", sr)
        sj = scrubjay.ScrubJay(_attrs(golden), config=cfg)
        x = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
        off = [0, pcm.shape[0]]
        whole = scrubjay.ScrubJayScanner(sj, 1 << 20, 1).run(x, off, stereo_mode=dsp_amd.STEREO_AVERAGE)
        assert whole[0].tolist() == [0, 1]
        _equal(whole[1:], sj.ragged(x, off, stereo_mode=dsp_amd.STEREO_AVERAGE), (name, "whole"))
        for wf, hf in ((16, 4), (32, 2)):
            wo, *got = scrubjay.ScrubJayScanner(sj, wf, hf).run(x, off, stereo_mode=dsp_amd.STEREO_AVERAGE)
            starts, lengths = scrubjay.scan_window_spans(cfg, off, wf, hf)
            cut, coff = _cut_out(torch, x, starts, lengths)
            assert wo[-1] == starts.size > 1
            _equal(got, sj.ragged(cut, coff, stereo_mode=dsp_amd.STEREO_AVERAGE), (name, wf, hf))


def test_refusals_and_optional_outputs(torch_cuda, golden):
    torch = torch_cuda
    import dsp_amd
    from dsp_amd import lib as dl
    from dsp_amd import scrubjay
    attrs = _attrs(golden)
    with pytest.raises(dl.DspError, match="GLOBAL_REF1"):
        scrubjay.ScrubJayScanner(scrubjay.ScrubJay(attrs, config=dsp_amd.default_config(n_mfcc=20, log_mode=dl.LOG_GLOBAL_REF1)))
    with pytest.raises(dl.DspError, match="n_features"):
        scrubjay.ScrubJayScanner(scrubjay.ScrubJay(attrs, config=dsp_amd.default_config(n_mfcc=13)))
    with pytest.raises(ValueError):
        scrubjay.ScrubJayScanner(scrubjay.ScrubJay(attrs), 0, 4)
    sj = scrubjay.ScrubJay(attrs)
    sc = scrubjay.ScrubJayScanner(sj, 98, 10)
    x = torch.from_numpy(np.random.default_rng(9).uniform(-1, 1, 50000).astype(np.float32)).cuda()
    with pytest.raises(dl.DspError, match="recording 1 "):
        sc.run(x, [0, 20000, 20399, 50000])                                      # 399 samples: no row
    with pytest.raises(dl.DspError, match="recording 0 "):
        sj.svm.scan(torch.zeros((10, 20), device="cuda"), [0, 0, 10], 4, 1)
    wo, *empty = sc.run(x, [0])                                                   # zero recordings: DSP_OK, nothing launched
    assert wo.tolist() == [0] and all(t.shape[0] == 0 for t in empty)
    # d_decision, d_prob1 and d_feat may be NULL; d_labels may not
    ref = sc.run(x, [0, 20000, 50000])
    labels = torch.full_like(ref[1], -1)
    off, n = dl.c_offsets([0, 20000, 50000])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = dl.load()
    dl.check(L.dsp_scrubjay_scanner_run_device(sc._h, x.data_ptr(), n, off, labels.data_ptr(), None, None, None, st), "run")
    assert torch.equal(labels, ref[1])
    assert L.dsp_scrubjay_scanner_run_device(sc._h, x.data_ptr(), n, off, None, None, None, None, st) < 0
    assert L.dsp_scrubjay_scanner_run_device(sc._h, x.data_ptr(), 0, off, None, None, None, None, st) == 0
