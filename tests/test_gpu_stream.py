"""GPU: stream sessions (dsp_stream_session_*, dsp_stream_push_device).  A stream's outputs, concatenated over its pushes, must be bit
for bit what the whole-recording entries give on the samples it has received: the rows of MfccPlan.clips_ragged (no frame cap) and,
for every stream that holds at least window_frames rows, Scanner.run's P("stop"), Q8 LLR mean and label (a stream with fewer rows has
no window at all: the one deliberate difference from the scanner).  Every comparison is exact: both sides run the same kernels on the
same values.  Floats are compared by their bit patterns."""
import ctypes as C

import numpy as np
import pytest

from tests import stream_ref as R

pytestmark = pytest.mark.gpu
NO_CAP = 2**31 - 1
FL, H = 400, 160


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def models(torch_cuda, golden):
    import dsp_amd
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return dsp_amd.MfccPlan(dsp_amd.default_config()), dsp_amd.StopModel(dict(golden("stop_model.npz"))), dsp_amd.SpeakerModel(t, u)


def _noise(rng, n):
    """float32 noise with quiet and loud stretches (as test_gpu_scan._recordings)"""
    x = rng.uniform(-1, 1, n).astype(np.float32)
    env = np.repeat(rng.uniform(0.001, 1.0, n // 4000 + 1).astype(np.float32), 4000)[:n]
    return (x * env).astype(np.float32)


def _recordings(seed):
    """seeded lengths: the edge cases, a few of 1-30 s, one of 10 min -> (lengths, signals, a chunking per recording)"""
    rng = np.random.default_rng(seed)
    lens = [0, 399, 400, 401, 15999, 16000] + rng.integers(16000, 30 * 16000, 4).tolist() + [10 * 60 * 16000]
    sigs = [_noise(rng, n) for n in lens]
    cuts = [R.chunking(n, rng, [16000, 50001, 160000] if n > 30 * 16000 else R.CHUNKS) for n in lens]
    return lens, sigs, cuts


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _drive(torch, sess, sigs, cuts, want_rows=True, sync_every_push=True):
    """Push every stream's chunks (cuts[s]; a stream that has none left pushes a zero-length chunk) until all are consumed.
    -> per stream [rows, prob, llr_mean, label] as numpy arrays (None where the session has none)."""
    import dsp_amd
    n = len(sigs)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in sigs]
    at = [0] * n
    pushes = []
    wf_hf = (sess.cfg.window_frames, sess.cfg.hop_frames) if sess.cfg is not None else ()
    for p in range(max(len(c) for c in cuts)):
        lens = [cuts[s][p] if p < len(cuts[s]) else 0 for s in range(n)]
        pad = int(p % 3)                                     # the chunks need not start at the buffer's first sample
        parts = [dev[0][:0].new_zeros((pad,) + tuple(dev[0].shape[1:]))] + [dev[s][at[s]:at[s] + lens[s]] for s in range(n)]
        co = np.concatenate([[pad], lens]).cumsum()
        want_ro, want_wo = dsp_amd.stream_push_plan(sess.plan.cfg, sess.counts()[0], co, *wf_hf)
        out = sess.push(torch.cat(parts), co, want_rows=want_rows)
        assert np.array_equal(out[0], want_ro) and (want_wo is None or np.array_equal(out[2], want_wo)), p
        if want_wo is None:
            assert not out[2].any()
        pushes.append(out)
        at = [a + ln for a, ln in zip(at, lens)]
        if sync_every_push:
            torch.cuda.synchronize()
    assert at == [len(x) for x in sigs]
    torch.cuda.synchronize()
    host = [[None if t is None else t.cpu().numpy() for t in (o[1], o[3], o[4], o[5])] for o in pushes]
    per = []
    for s in range(n):
        got = []
        for k, off in ((0, 0), (1, 2), (2, 2), (3, 2)):
            if host[0][k] is None:
                got.append(None)
            else:
                got.append(np.concatenate([h[k][int(o[off][s]):int(o[off][s + 1])] for h, o in zip(host, pushes)]))
        per.append(got)
    return per


def _whole_rows(torch, plan, sigs):
    off = np.concatenate([[0], np.cumsum([len(x) for x in sigs])]).astype(np.int64)
    mf, fo = plan.clips_ragged(torch.from_numpy(np.concatenate(sigs)).cuda(), off, NO_CAP)
    mf = mf.cpu().numpy()
    return [mf[int(fo[r]):int(fo[r + 1])] for r in range(len(sigs))]


def _whole_windows(torch, plan, stop, spk, sigs, wf, hf):
    """Scanner.run on the recordings that hold at least wf rows -> {recording: [prob, llr_mean, label]}"""
    import dsp_amd
    keep = [r for r, x in enumerate(sigs) if R.rows_after(len(x), FL, H) >= wf]
    if not keep:
        return {}
    off = np.concatenate([[0], np.cumsum([len(sigs[r]) for r in keep])]).astype(np.int64)
    sc = dsp_amd.Scanner(plan, stop=stop, speaker=spk, window_frames=wf, hop_frames=hf)
    wo, prob, mean, label = sc.run(torch.from_numpy(np.concatenate([sigs[r] for r in keep])).cuda(), off)
    outs = [None if t is None else t.cpu().numpy() for t in (prob, mean, label)]
    sc.close()
    return {r: [None if o is None else o[int(wo[k]):int(wo[k + 1])] for o in outs] for k, r in enumerate(keep)}


def _check_windows(per, whole, n, wf, hf, sigs):
    for r in range(n):
        rows = R.rows_after(len(sigs[r]), FL, H)
        for k in range(3):
            got = per[r][1 + k]
            if got is None:
                assert r not in whole or whole[r][k] is None
                continue
            if r in whole:
                assert got.size == R.windows_after(rows, wf, hf) and _same(got, whole[r][k]), (r, k, wf, hf)
            else:
                assert got.size == 0, (r, k)


def test_rows_equal_the_whole_recordings(torch_cuda, models):
    import dsp_amd
    torch = torch_cuda
    plan, _stop, _spk = models
    lens, sigs, cuts = _recordings(21)
    sess = dsp_amd.StreamSession(plan, len(lens))
    per = _drive(torch, sess, sigs, cuts)
    want = _whole_rows(torch, plan, sigs)
    for r in range(len(lens)):
        assert _same(per[r][0], want[r]), (r, lens[r])
        assert per[r][1] is None and per[r][2] is None and per[r][3] is None
    samples, rows, windows = sess.counts()
    assert samples.tolist() == lens and rows.tolist() == [w.shape[0] for w in want] and not windows.any()
    sess.close()


@pytest.mark.parametrize("which", ["stop", "speaker", "both"])
@pytest.mark.parametrize("wf,hf", [(98, 10), (98, 1), (98, 98), (30, 7)])
def test_windows_equal_the_scanner(torch_cuda, models, wf, hf, which):
    import dsp_amd
    torch = torch_cuda
    plan, stop, spk = models
    stop, spk = (stop if which != "speaker" else None), (spk if which != "stop" else None)
    lens, sigs, cuts = _recordings(1000 * wf + hf)
    whole = _whole_windows(torch, plan, stop, spk, sigs, wf, hf)
    assert len(whole) >= 6                                   # a condition on the inputs: the short recordings cannot hide a failure
    sess = dsp_amd.StreamSession(plan, len(lens), stop=stop, speaker=spk, window_frames=wf, hop_frames=hf)
    per = _drive(torch, sess, sigs, cuts, want_rows=(which == "both"))
    _check_windows(per, whole, len(lens), wf, hf, sigs)
    if which == "both":
        want = _whole_rows(torch, plan, sigs)
        assert all(_same(per[r][0], want[r]) for r in range(len(lens)))
    assert sess.counts()[2].tolist() == [R.windows_after(R.rows_after(n, FL, H), wf, hf) for n in lens]
    sess.close()


def test_chunking_does_not_show(torch_cuda, models):
    import dsp_amd
    torch = torch_cuda
    plan, stop, spk = models
    rng = np.random.default_rng(33)
    lens = [401, 16000, 47111] + rng.integers(16000, 30 * 16000, 3).tolist()
    sigs = [_noise(rng, n) for n in lens]
    runs = []
    for cuts in ([R.chunking(n, rng) for n in lens], [R.chunking(n, rng) for n in lens], [[n] for n in lens]):
        sess = dsp_amd.StreamSession(plan, len(lens), stop=stop, speaker=spk)
        runs.append(_drive(torch, sess, sigs, cuts))
        sess.close()
    for other in runs[1:]:
        for r in range(len(lens)):
            for k in range(4):
                assert _same(runs[0][r][k], other[r][k]), (r, k)
    whole = _whole_windows(torch, plan, stop, spk, sigs, 98, 10)
    _check_windows(runs[2], whole, len(lens), 98, 10, sigs)


def test_short_pushes(torch_cuda, models):
    """a chunk shorter than what is carried (the new tail comes out of the old one), next to a stream fed a second per push; then
    2 000 pushes enqueued back to back with no host synchronisation, compared once at the end"""
    import dsp_amd
    torch = torch_cuda
    plan, stop, spk = models
    rng = np.random.default_rng(44)
    sigs = [_noise(rng, 1000), _noise(rng, 1000 * 16000)]
    sess = dsp_amd.StreamSession(plan, 2, stop=stop, speaker=spk)
    per = _drive(torch, sess, sigs, [[1] * 1000, [16000] * 1000], sync_every_push=False)
    want = _whole_rows(torch, plan, sigs)
    assert _same(per[0][0], want[0]) and want[0].shape[0] == 4 and _same(per[1][0], want[1])
    _check_windows(per, _whole_windows(torch, plan, stop, spk, sigs, 98, 10), 2, 98, 10, sigs)
    sess.close()
    # hop-sized pushes, three streams out of phase with each other
    first = [0, 77, 399]
    sigs = [_noise(rng, f + 1999 * 160) for f in first]
    sess = dsp_amd.StreamSession(plan, 3, stop=stop, speaker=spk)
    per = _drive(torch, sess, sigs, [[f] + [160] * 1999 for f in first], sync_every_push=False)
    want = _whole_rows(torch, plan, sigs)
    assert all(_same(per[r][0], want[r]) for r in range(3))
    whole = _whole_windows(torch, plan, stop, spk, sigs, 98, 10)
    assert len(whole) == 3
    _check_windows(per, whole, 3, 98, 10, sigs)
    sess.close()


def test_pcm16_matches_the_float_session(torch_cuda, models):
    import dsp_amd
    torch = torch_cuda
    plan, stop, spk = models
    rng = np.random.default_rng(3)
    lens = [16000, 40001, 401, 123457]
    pcms = [rng.integers(-32768, 32768, (n, 2)).astype(np.int16) for n in lens]
    pcms[1][:20000] //= 64
    cuts = [R.chunking(n, rng) for n in lens]
    one = np.float32(32768.0)
    kinds = {
        "mono": ([np.ascontiguousarray(p[:, 0]) for p in pcms], dict(), [(p[:, 0] / one).astype(np.float32) for p in pcms]),
        "ch0": (pcms, dict(channels=2, stereo_mode=0), [(p[:, 0] / one).astype(np.float32) for p in pcms]),
        "avg": (pcms, dict(channels=2, stereo_mode=1), [(np.float32(0.5) * (p[:, 0] / one + p[:, 1] / one)).astype(np.float32) for p in pcms]),
    }
    for name, (raw, kw, decoded) in kinds.items():
        a = dsp_amd.StreamSession(plan, len(lens), stop=stop, speaker=spk, dtype=torch.int16, **kw)
        b = dsp_amd.StreamSession(plan, len(lens), stop=stop, speaker=spk)
        pa, pb = _drive(torch, a, raw, cuts), _drive(torch, b, decoded, cuts)
        for r in range(len(lens)):
            for k in range(4):
                assert _same(pa[r][k], pb[r][k]), (name, r, k)
        assert sum(p[1].size for p in pa) > 0
        a.close()
        b.close()


def test_reset_and_refused_pushes(torch_cuda, models):
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    plan, stop, spk = models
    rng = np.random.default_rng(66)
    first = [_noise(rng, n) for n in (30000, 20123, 16000, 50001)]
    rest = [_noise(rng, n) for n in (40000, 33333, 999, 70001)]          # streams 0 and 2 go on; 1 and 3 are new feeds after the reset
    sess = dsp_amd.StreamSession(plan, 4, stop=stop, speaker=spk)
    per1 = _drive(torch, sess, first, [R.chunking(len(x), rng) for x in first])
    before = [c.copy() for c in sess.counts()]
    # refused pushes: stream 0's chunk is fine, stream 1's runs backwards -- nothing may have been committed for stream 0 either
    lib = L.load()
    lp = C.POINTER(C.c_long)
    x = torch.zeros(4000, device="cuda")
    bad = np.array([0, 500, 400, 900, 1000], np.int64)
    assert lib.dsp_stream_push_device(sess._h, x.data_ptr(), bad.ctypes.data_as(lp), None, None, None, None, None, None, None) == -1
    ok = np.array([0, 500, 600, 900, 1000], np.int64)
    assert lib.dsp_stream_push_device(sess._h, None, ok.ctypes.data_as(lp), None, None, None, None, None, None, None) == -1      # no chunks
    with pytest.raises(ValueError):
        sess.push(x, bad)
    with pytest.raises(ValueError):
        sess.push(x, [0, 500, 600, 900, 5000])
    with pytest.raises(ValueError):
        sess.reset([4])
    assert all(np.array_equal(a, b) for a, b in zip(before, sess.counts()))
    sess.reset([1, 3])
    after = sess.counts()
    for c, b in zip(after, before):
        assert c[[1, 3]].tolist() == [0, 0] and c[[0, 2]].tolist() == b[[0, 2]].tolist()
    per2 = _drive(torch, sess, rest, [R.chunking(len(x), rng) for x in rest])
    whole_sigs = [np.concatenate([first[0], rest[0]]), rest[1], np.concatenate([first[2], rest[2]]), rest[3]]
    got = [[np.concatenate([per1[r][k], per2[r][k]]) if r in (0, 2) else per2[r][k] for k in range(4)] for r in range(4)]
    want = _whole_rows(torch, plan, whole_sigs)
    assert all(_same(got[r][0], want[r]) for r in range(4))
    whole = _whole_windows(torch, plan, stop, spk, whole_sigs, 98, 10)
    assert len(whole) == 4
    _check_windows(got, whole, 4, 98, 10, whole_sigs)
    # what the streams emitted before the reset was their own first recording's
    w1 = _whole_rows(torch, plan, first)
    assert all(_same(per1[r][0], w1[r]) for r in range(4))
    sess.reset()
    assert not any(c.any() for c in sess.counts())
    sess.close()


def test_many_streams(torch_cuda, models):
    import dsp_amd
    torch = torch_cuda
    plan, stop, spk = models
    n, pushes = 4096, 15
    rng = np.random.default_rng(77)
    lens = 1600 + rng.integers(0, 201, (pushes, n))
    total = lens.sum(0)
    off = np.concatenate([[0], np.cumsum(total)]).astype(np.int64)
    signal = _noise(rng, int(off[-1]))
    dev = torch.from_numpy(signal).cuda()
    sess = dsp_amd.StreamSession(plan, n, stop=stop, speaker=spk)
    at = off[:-1].copy()
    outs = []
    for p in range(pushes):
        # stream s's chunk is the next lens[p][s] samples of its recording: gathered on the GPU into one buffer, back to back
        co = np.concatenate([[0], np.cumsum(lens[p])]).astype(np.int64)
        src = np.repeat(at - co[:-1], lens[p]) + np.arange(int(co[-1]))
        outs.append(sess.push(dev[torch.from_numpy(src).cuda()], co))
        at += lens[p]
    torch.cuda.synchronize()
    mf, fo = plan.clips_ragged(dev, off, NO_CAP)
    sc = dsp_amd.Scanner(plan, stop=stop, speaker=spk)
    wo, prob, mean, label = sc.run(dev, off)
    want = [t.cpu().numpy() for t in (mf, prob, mean, label)]
    host = [[t.cpu().numpy() for t in (o[1], o[3], o[4], o[5])] for o in outs]
    assert np.diff(fo).min() >= 98
    for s in range(n):
        for k, (whole_off, idx) in enumerate(((fo, 0), (wo, 2), (wo, 2), (wo, 2))):
            got = np.concatenate([h[k][int(o[idx][s]):int(o[idx][s + 1])] for h, o in zip(host, outs)])
            assert _same(got, want[k][int(whole_off[s]):int(whole_off[s + 1])]), (s, k)
    sc.close()
    sess.close()


def test_refusals(torch_cuda, models):
    import dsp_amd
    from dsp_amd import lib as L
    torch = torch_cuda
    plan, stop, spk = models
    lib = L.load()
    sj = L.MfccConfig()
    lib.dsp_mfcc_scrubjay_infer_config(C.byref(sj), 16000)
    sj.n_mfcc = 13
    for cfg_bad in (dsp_amd.default_config(log_mode=L.LOG_GLOBAL_REF1), sj, dsp_amd.default_config(prefilter=L.PREFILTER_BUTTER_1000_3000)):
        bad = dsp_amd.MfccPlan(cfg_bad)
        with pytest.raises(L.DspError, match="rows do not depend on the window"):
            dsp_amd.StreamSession(bad, 4, stop=stop)
        with pytest.raises(L.DspError, match="rows do not depend on the window"):
            dsp_amd.StreamSession(bad, 4)
    with pytest.raises(L.DspError, match="n_mfcc"):
        dsp_amd.StreamSession(dsp_amd.MfccPlan(dsp_amd.default_config(n_mfcc=20)), 4, speaker=spk)
    with pytest.raises(L.DspError, match="n_mfcc"):
        dsp_amd.StreamSession(dsp_amd.MfccPlan(dsp_amd.default_config(n_mfcc=20)), 4, stop=stop)
    with pytest.raises(L.DspError, match="hop_length > frame_length"):
        dsp_amd.StreamSession(dsp_amd.MfccPlan(dsp_amd.default_config(hop_length=480)), 4)
    with pytest.raises(ValueError):
        dsp_amd.StreamSession(plan, 4, stop=stop, window_frames=10, hop_frames=25)
    h = C.c_void_p()
    cfg = L.ScanConfig(10, 25)
    assert lib.dsp_stream_session_create(plan._h, stop._h, None, C.byref(cfg), 4, 1, 0, 0, C.byref(h)) == -1 and "hop_frames > window_frames" in L.last_error()
    assert lib.dsp_stream_session_create(plan._h, stop._h, None, None, 4, 1, 0, 0, C.byref(h)) == -1
    assert lib.dsp_stream_session_create(plan._h, None, None, None, 4, 2, 0, 0, C.byref(h)) == -1              # float samples are mono
    assert lib.dsp_stream_session_create(plan._h, None, None, None, 4, 3, 0, 1, C.byref(h)) == -1
    assert lib.dsp_stream_session_create(plan._h, None, None, None, 4, 2, 7, 1, C.byref(h)) == -1
    # the session's input format is fixed when it is created
    f32 = dsp_amd.StreamSession(plan, 2)
    i16 = dsp_amd.StreamSession(plan, 2, dtype=torch.int16)
    with pytest.raises(ValueError, match="float32"):
        f32.push(torch.zeros(800, dtype=torch.int16, device="cuda"), [0, 400, 800])
    with pytest.raises(ValueError, match="int16"):
        i16.push(torch.zeros(800, device="cuda"), [0, 400, 800])
    with pytest.raises(ValueError):
        i16.push(torch.zeros((800, 2), dtype=torch.int16, device="cuda"), [0, 400, 800])
    with pytest.raises(ValueError):
        f32.push(torch.zeros(800), [0, 400, 800])
    assert not f32.counts()[0].any() and not i16.counts()[0].any()
    # zero streams, and a push that completes nothing: DSP_OK
    empty = dsp_amd.StreamSession(plan, 0, stop=stop)
    ro, rows, wo, prob, mean, label = empty.push(torch.zeros(8, device="cuda"), [0])
    assert ro.tolist() == [0] and wo.tolist() == [0] and rows.shape == (0, 13) and prob.numel() == 0 and mean is None
    ro, rows, _wo, _p, _m, _l = f32.push(torch.zeros(800, device="cuda"), [0, 399, 399])
    assert ro.tolist() == [0, 0, 0] and f32.counts()[0].tolist() == [399, 0]
    for s in (f32, i16, empty):
        s.close()
