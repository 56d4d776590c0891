"""GPU: the streaming resampler (dsp_stream_resample*, dsp_stream_session_attach_resampler).  The oracle is always the existing
one-shot entry (Resampler.ragged) on the concatenated feed, and every comparison is of bit patterns: a stream's pushes give the first
K(N) outputs of the whole feed, finish() the rest, whatever the chunk lengths, the other streams or the batch.  Sizes are the
smallest that cross every branch: chunks of 0, 1, T - 2, T - 1, T and random <= 700 frames, one push per stream of two tiles plus a
ragged third, 1 / 3 / 257 streams, chunks at odd int16 and non-16-byte positions."""
import ctypes as C

import numpy as np
import pytest

from tests import resample_ref as R
from tests import stream_resample_ref as S

pytestmark = pytest.mark.gpu
RATES = [10000, 9000, 44100, 48000, 16000]          # up 8 / down 5, 16 / 9, 160 / 441, 1 / 3 (UP1), the copy
FORMATS = ["float", "mono", "stereo0", "stereo_avg"]
LP = C.POINTER(C.c_long)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _fmt(torch, fmt):
    """-> kwargs of StreamResampler / StreamSession, stereo_mode"""
    if fmt == "float":
        return dict(dtype=torch.float32), 0
    if fmt == "mono":
        return dict(dtype=torch.int16), 0
    mode = 0 if fmt == "stereo0" else 1
    return dict(dtype=torch.int16, channels=2, stereo_mode=mode), mode


def _feeds(rng, fmt, lengths):
    """seeded feeds in the caller's format: float32 [n], int16 [n] or int16 [n][2]"""
    if fmt == "float":
        return [rng.uniform(-1, 1, n).astype(np.float32) for n in lengths]
    shape = (lambda n: (n,)) if fmt == "mono" else (lambda n: (n, 2))
    return [rng.integers(-32768, 32768, shape(n)).astype(np.int16) for n in lengths]


def _tile(rate_in):
    """outputs per block at this ratio (a function of the ratio), T"""
    up, down, half = R.ratio(rate_in, 16000)
    return {10000: 4096, 9000: 4096, 44100: 1920, 48000: 2048, 16000: 4096}[rate_in], S.taps_per_branch(up, half)


def _cuts(rng, rate_in, n_streams, pushes=7):
    """per stream a list of chunk lengths: the lengths around the carry's, and one chunk of two tiles of outputs plus a ragged third"""
    up, down, _half = R.ratio(rate_in, 16000)
    tile, T = _tile(rate_in)
    long_chunk = (2 * tile + 37) * down // up + 11
    cuts = []
    for s in range(n_streams):
        c = [int(rng.choice([0, 1, T - 2, T - 1, T, int(rng.integers(1, 701))])) for _ in range(pushes)]
        c.insert(int(rng.integers(0, pushes + 1)), long_chunk + int(rng.integers(0, 50)))
        cuts.append(c)
    return cuts


def _upload(torch, buf, fmt, odd):
    """a host buffer -> the CUDA tensor a push takes; odd: interleaved stereo whose first int16 lies at an odd int16 of its allocation"""
    if fmt.startswith("stereo") and odd:
        flat = torch.zeros(1 + buf.size, dtype=torch.int16, device="cuda")
        flat[1:] = torch.from_numpy(buf.reshape(-1)).cuda()
        t = flat[1:].view(-1, 2)
        assert t.data_ptr() % 4 == 2 and t.is_contiguous()
        return t
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def _drive(torch, rs, feeds, cuts, fmt, odd=False, at=None):
    """Push every stream's chunks (a stream that has none left pushes a zero-length chunk).  Push p's chunks start 1 + p % 5 sample
    frames into the buffer: odd int16 and non-16-byte positions.  -> per stream the concatenated outputs (numpy float32)."""
    import dsp_amd
    n = len(feeds)
    at = [0] * n if at is None else at
    got = [[] for _ in range(n)]
    outs = []
    for p in range(max(len(c) for c in cuts)):
        lens = [cuts[s][p] if p < len(cuts[s]) else 0 for s in range(n)]
        pad = 1 + p % 5
        parts = [np.zeros((pad,) + feeds[0].shape[1:], feeds[0].dtype)] + [feeds[s][at[s]:at[s] + lens[s]] for s in range(n)]
        co = np.concatenate([[pad], lens]).cumsum()
        want = dsp_amd.stream_resample_plan(rs.rate_in, rs.rate_out, rs.counts()[0], co)
        out, oo = rs.push(_upload(torch, np.concatenate(parts), fmt, odd), co)
        assert np.array_equal(oo, want), p
        outs.append((out, oo))
        for s in range(n):
            at[s] += lens[s]
    torch.cuda.synchronize()
    for out, oo in outs:
        h = out.cpu().numpy()
        for s in range(n):
            got[s].append(h[int(oo[s]):int(oo[s + 1])])
    return [np.concatenate(g) for g in got]


def _whole(torch, rate_in, feeds, fmt, mode, lengths=None):
    """the one-shot entry on the feeds (their first lengths[s] frames) -> per stream numpy float32"""
    import dsp_amd
    lengths = [len(x) for x in feeds] if lengths is None else lengths
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    r = dsp_amd.Resampler(rate_in, 16000)
    sig = np.concatenate([x[:ln] for x, ln in zip(feeds, lengths)])
    out, oo = r.ragged(torch.from_numpy(np.ascontiguousarray(sig)).cuda(), off, stereo_mode=mode)
    out = out.cpu().numpy()
    r.close()
    return [out[int(oo[s]):int(oo[s + 1])] for s in range(len(feeds))]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _k(rate_in, n):
    return S.emitted(n, *R.ratio(rate_in, 16000))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n_streams", [1, 3, 257])
@pytest.mark.parametrize("rate_in", RATES)
def test_pushes_then_finish_equal_the_whole_feed(torch_cuda, rate_in, n_streams, fmt):
    import dsp_amd
    torch = torch_cuda
    rng = np.random.default_rng(rate_in + 7 * n_streams + len(fmt))
    cuts = _cuts(rng, rate_in, n_streams)
    feeds = _feeds(rng, fmt, [sum(c) for c in cuts])
    kw, mode = _fmt(torch, fmt)
    rs = dsp_amd.StreamResampler(rate_in, 16000, n_streams, **kw)
    got = _drive(torch, rs, feeds, cuts, fmt, odd=n_streams == 3)
    want = _whole(torch, rate_in, feeds, fmt, mode)
    n_in, n_out = rs.counts()
    for s in range(n_streams):
        k = _k(rate_in, len(feeds[s]))
        assert n_in[s] == len(feeds[s]) and n_out[s] == k == got[s].size
        assert _same(got[s], want[s][:k]), (s, k)
    rest, ro = rs.finish()
    rest = rest.cpu().numpy()
    for s in range(n_streams):
        assert _same(np.concatenate([got[s], rest[int(ro[s]):int(ro[s + 1])]]), want[s]), s
    assert not rs.counts()[0].any() and not rs.counts()[1].any()
    rs.close()


@pytest.mark.parametrize("fmt", ["mono", "stereo0", "stereo_avg"])
@pytest.mark.parametrize("rate_in", [10000, 48000])
def test_int16_equals_the_float_stream_on_the_decoded_samples(torch_cuda, rate_in, fmt):
    import dsp_amd
    torch = torch_cuda
    rng = np.random.default_rng(rate_in + len(fmt))
    cuts = _cuts(rng, rate_in, 3)
    feeds = _feeds(rng, fmt, [sum(c) for c in cuts])
    kw, mode = _fmt(torch, fmt)
    a = dsp_amd.StreamResampler(rate_in, 16000, 3, **kw)
    b = dsp_amd.StreamResampler(rate_in, 16000, 3)
    got = _drive(torch, a, feeds, cuts, fmt, odd=True)
    ref = _drive(torch, b, [R.decode_pcm16(x, mode) for x in feeds], cuts, "float")
    for s in range(3):
        assert got[s].size == _k(rate_in, len(feeds[s])) and _same(got[s], ref[s]), s
    a.close()
    b.close()


@pytest.mark.parametrize("rate_in", [10000, 44100, 48000])
def test_chunking_and_neighbours_show_in_no_bit(torch_cuda, rate_in):
    """two chunkings of the same feeds give the same bits; a stream's bits do not change with the other streams' data and chunks"""
    import dsp_amd
    torch = torch_cuda
    rng = np.random.default_rng(rate_in)
    cuts = _cuts(rng, rate_in, 3)
    feeds = _feeds(rng, "float", [sum(c) for c in cuts])
    rs = dsp_amd.StreamResampler(rate_in, 16000, 3)
    first = _drive(torch, rs, feeds, cuts, "float")
    rs.reset()
    other = [S.chunking(len(x), rng, [19, 20, 21, 5000]) for x in feeds]
    second = _drive(torch, rs, feeds, other, "float")
    for s in range(3):
        assert first[s].size == _k(rate_in, len(feeds[s])) and _same(first[s], second[s]), s
    rs.reset()
    cuts2 = _cuts(rng, rate_in, 3, pushes=5)
    cuts2[1] = cuts[1]
    feeds2 = _feeds(rng, "float", [sum(c) for c in cuts2])
    feeds2[1] = feeds[1]
    third = _drive(torch, rs, feeds2, cuts2, "float")
    assert _same(third[1], first[1])
    rs.close()


@pytest.mark.parametrize("fmt", ["float", "mono"])
@pytest.mark.parametrize("rate_in", [10000, 48000, 16000])
def test_finish_completes_short_and_empty_streams(torch_cuda, rate_in, fmt):
    import dsp_amd
    torch = torch_cuda
    _tile_, T = _tile(rate_in)
    lengths = [0, 1, T - 1, 3000, 5]
    rng = np.random.default_rng(5 + rate_in)
    feeds = _feeds(rng, fmt, lengths)
    cuts = [[n] if n < 100 else [1000, 0, 1999, 1] for n in lengths]
    kw, mode = _fmt(torch, fmt)
    rs = dsp_amd.StreamResampler(rate_in, 16000, len(lengths), **kw)
    got = _drive(torch, rs, feeds, cuts, fmt)
    want = _whole(torch, rate_in, feeds, fmt, mode)
    # finish some streams, in an order of the caller's; the others go on
    order = [3, 0, 2]
    rest, ro = rs.finish(order)
    rest = rest.cpu().numpy()
    for i, s in enumerate(order):
        assert _same(np.concatenate([got[s], rest[int(ro[i]):int(ro[i + 1])]]), want[s]), s
    n_in, n_out = rs.counts()
    assert n_in.tolist() == [0, 1, 0, 0, 5] and n_out.tolist() == [0, _k(rate_in, 1), 0, 0, _k(rate_in, 5)]
    rest, ro = rs.finish([4, 1])
    rest = rest.cpu().numpy()
    for i, s in enumerate([4, 1]):
        assert _same(np.concatenate([got[s], rest[int(ro[i]):int(ro[i + 1])]]), want[s]), s
    # a finished slot takes a new feed
    again = _drive(torch, rs, feeds, cuts, fmt)
    for s in range(len(lengths)):
        assert _same(again[s], got[s]), s
    rs.close()


def test_reset_gives_a_slot_a_fresh_feed_and_a_refused_push_changes_nothing(torch_cuda):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    rate_in = 10000
    rng = np.random.default_rng(77)
    cuts = _cuts(rng, rate_in, 3)
    feeds = _feeds(rng, "float", [sum(c) for c in cuts])
    rs = dsp_amd.StreamResampler(rate_in, 16000, 3)
    half = [c[:4] for c in cuts]
    at = [0, 0, 0]
    first = _drive(torch, rs, feeds, half, "float", at=at)
    before = [a.copy() for a in rs.counts()]
    # refused at the C ABI: chunks of 8 frames each and no buffer; decreasing offsets; the counters stay
    co = np.array([0, 8, 16, 24], np.int64)
    assert rs._L.dsp_stream_resample_push_device(rs._h, None, co.ctypes.data_as(LP), None, None, None) == -1 and "d_chunks" in dl.last_error()
    bad = np.array([0, 8, 4, 24], np.int64)
    assert rs._L.dsp_stream_resample_push_device(rs._h, 16, bad.ctypes.data_as(LP), None, None, None) == -1 and "stream 1" in dl.last_error()
    idx = np.array([0, 3], np.int64)
    assert rs._L.dsp_stream_resample_finish_device(rs._h, idx.ctypes.data_as(LP), 2, None, None, None) == -1
    idx = np.array([1, 1], np.int64)
    assert rs._L.dsp_stream_resample_finish_device(rs._h, idx.ctypes.data_as(LP), 2, None, None, None) == -1 and "twice" in dl.last_error()
    for a, b in zip(before, rs.counts()):
        assert np.array_equal(a, b)
    # stream 1 starts a new feed; 0 and 2 go on with theirs
    rs.reset([1])
    assert rs.counts()[0][1] == 0 and rs.counts()[1][1] == 0
    new = _feeds(rng, "float", [2345])[0]
    feeds2 = [feeds[0], new, feeds[2]]
    at[1] = 0
    rest_cuts = [cuts[0][4:], [700, 20, 1, 1624], cuts[2][4:]]
    second = _drive(torch, rs, feeds2, rest_cuts, "float", at=at)
    want = _whole(torch, rate_in, feeds2, "float", 0)
    for s in (0, 2):
        assert _same(np.concatenate([first[s], second[s]]), want[s][:_k(rate_in, len(feeds[s]))]), s
    assert _same(second[1], want[1][:_k(rate_in, 2345)])
    rs.close()


@pytest.fixture(scope="module")
def models(torch_cuda, golden):
    import dsp_amd
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    return dsp_amd.MfccPlan(dsp_amd.default_config()), dsp_amd.StopModel(dict(golden("stop_model.npz"))), dsp_amd.SpeakerModel(t, u)


def test_attach_refusals(torch_cuda, models):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    plan, _stop, _spk = models
    L = dl.load()
    attach = L.dsp_stream_session_attach_resampler

    def refused(sess, rs, word):
        assert attach(sess._h, rs._h) == -1 and word in dl.last_error(), dl.last_error()

    good = dsp_amd.StreamResampler(10000, 16000, 3)
    sess = dsp_amd.StreamSession(plan, 3)
    assert attach(sess._h, None) == -1 and attach(None, good._h) == -1
    refused(sess, dsp_amd.StreamResampler(10000, 16000, 4), "streams")
    refused(sess, dsp_amd.StreamResampler(10000, 8000, 3), "Hz")
    pcm = dsp_amd.StreamSession(plan, 3, dtype=torch.int16)
    refused(pcm, good, "float mono")
    if torch.cuda.device_count() > 1:
        refused(sess, dsp_amd.StreamResampler(10000, 16000, 3, device=1), "devices")
    sess.push(torch.zeros(30, device="cuda"), [0, 10, 20, 30])
    refused(sess, good, "first push")
    fresh = dsp_amd.StreamSession(plan, 3)
    assert attach(fresh._h, good._h) == 0
    refused(fresh, good, "already")
    for o in (fresh, sess, pcm, good):
        o.close()


@pytest.mark.parametrize("fmt", ["float", "mono"])
@pytest.mark.parametrize("wf,hf", [(98, 10), (30, 7)])
def test_session_with_a_resampler_equals_resampling_first(torch_cuda, models, wf, hf, fmt):
    """3 feeds of about 2 s at 10 kHz in 100 ms chunks through StreamSession(rate_in=10000) against: Resampler on the whole feed,
    pushed as one chunk into a plain session"""
    import dsp_amd
    torch = torch_cuda
    plan, stop, spk = models
    rng = np.random.default_rng(wf + len(fmt))
    lengths = [20000, 19037, 21111]
    feeds = _feeds(rng, fmt, lengths)
    kw, mode = _fmt(torch, fmt)
    sess = dsp_amd.StreamSession(plan, 3, stop=stop, speaker=spk, window_frames=wf, hop_frames=hf, rate_in=10000, **kw)
    outs, at = [], [0, 0, 0]
    while any(a < n for a, n in zip(at, lengths)):
        lens = [min(1000, n - a) for a, n in zip(at, lengths)]
        co = np.concatenate([[0], lens]).cumsum()
        chunk = np.concatenate([feeds[s][at[s]:at[s] + lens[s]] for s in range(3)])
        outs.append(sess.push(torch.from_numpy(chunk).cuda(), co))
        at = [a + ln for a, ln in zip(at, lens)]
    torch.cuda.synchronize()
    # the other side
    whole = _whole(torch, 10000, feeds, fmt, mode)
    at_rate = [w[:_k(10000, n)] for w, n in zip(whole, lengths)]           # what a stream has emitted without a finish
    plain = dsp_amd.StreamSession(plan, 3, stop=stop, speaker=spk, window_frames=wf, hop_frames=hf)
    co = np.concatenate([[0], [len(x) for x in at_rate]]).cumsum()
    ref = plain.push(torch.from_numpy(np.concatenate(at_rate)).cuda(), co)
    torch.cuda.synchronize()
    for a, b in zip(sess.counts(), plain.counts()):
        assert np.array_equal(a, b)
    assert sess.counts()[0].tolist() == [len(x) for x in at_rate]
    for k, off in ((1, 0), (3, 2), (4, 2), (5, 2)):              # rows by row_offsets; prob, llr_mean, label by window_offsets
        want = ref[k].cpu().numpy()
        for s in range(3):
            got = np.concatenate([o[k].cpu().numpy()[int(o[off][s]):int(o[off][s + 1])] for o in outs])
            w = want[int(ref[off][s]):int(ref[off][s + 1])]
            assert got.shape == w.shape and got.size > 0 and np.array_equal(got.view(np.uint8), w.view(np.uint8)), (k, s)
    # a reset reaches the resampler
    sess.reset([1])
    assert sess.counts()[0].tolist()[1] == 0 and sess.resampler.counts()[0].tolist() == [lengths[0], 0, lengths[2]]
    sess.close()
    plain.close()
