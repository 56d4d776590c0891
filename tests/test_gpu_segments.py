"""GPU: segments from window scores (dsp_segments_device; dsp_amd.Segmenter).

Against tests/segments_ref.py every integer field and `peak` must be equal, `mean` within 2^-23 |ref| + n_active 2^-53 max |x| (one
float32 rounding plus the any-order float64 summation bound; the reference sums with math.fsum).  Every field stays the same bits whatever
the batch, a recording's position in it, the other columns (independent mode), the stream, max_segments, the outputs asked for and what
the workspace held.  Every output buffer is filled with a sentinel and has spare entries behind it, which are checked.  That the shared
cases exercise merges, drops, word and chunk crossings and inherited states is checked on the reference alone, without a GPU, by
tests/test_segments_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import segments_ref as R
from tests import segments_util as U

pytestmark = pytest.mark.gpu
LP = C.POINTER(C.c_long)
SPARE = 3
SENTINEL = -7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def seg(torch_cuda):
    import dsp_amd
    s = dsp_amd.Segmenter()
    yield s
    s.close()


def _raw(torch, seg, scores, wo, m, g, mode, on=U.ON, off=U.OFF, room=None, want_segments=True, want_counts=True, stream=None):
    """dsp_segments_device into sentinel-filled buffers with SPARE entries behind each -> (segments written, counts or None, total[2]), the
    spare and everything behind the written segments checked.  room: max_segments (default: the capacity)."""
    import dsp_amd
    x = scores if isinstance(scores, torch.Tensor) else torch.tensor(np.ascontiguousarray(scores, np.float32), device="cuda")
    wo = np.ascontiguousarray(wo, np.int64)
    n, S = wo.size - 1, (x.shape[1] if x.dim() == 2 else 1)
    if x.numel() == 0:                                      # (an empty tensor has no address, and a NULL d_scores is refused)
        x = torch.zeros(1, dtype=torch.float32, device="cuda")
    cfg = dsp_amd.lib.SegmentConfig(float(on), float(off), m, g, mode)
    if room is None:
        room = R.capacity(wo, S, m, g)
    segs = torch.full((room + SPARE, 8), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.full((n * S + SPARE,), SENTINEL, dtype=torch.int32, device="cuda")
    total = torch.full((2 + SPARE,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    rc = seg._L.dsp_segments_device(seg._h, x.data_ptr(), n, wo.ctypes.data_as(LP), S, C.byref(cfg), segs.data_ptr() if want_segments else None, room,
                                    counts.data_ptr() if want_counts else None, total.data_ptr(), st)
    assert rc == 0, dsp_amd.lib.last_error()
    torch.cuda.synchronize()
    total = total.cpu().numpy()
    assert (total[2:] == SENTINEL).all(), "wrote behind d_total"
    found, written = int(total[0]), int(total[1])
    assert written == (min(found, room) if want_segments else 0)
    segs = segs.cpu().numpy()
    assert (segs[written:] == SENTINEL).all(), "wrote behind the segments"
    counts = counts.cpu().numpy()
    assert (counts[n * S:] == SENTINEL).all(), "wrote behind d_track_counts"
    if not want_counts:
        assert (counts == SENTINEL).all()
    return segs[:written].copy().view(R.DTYPE).reshape(-1), (counts[:n * S].reshape(n, S) if want_counts else None), total[:2]


def _bits(segs):
    return np.ascontiguousarray(segs).view(np.int32).reshape(-1, 8)


def _check(got, counts, total, ref, ref_counts, scores):
    assert int(total[0]) == ref.size
    assert np.array_equal(counts, ref_counts)
    assert got.size == ref.size
    for key in ("recording", "column", "first_window", "n_windows", "n_active", "peak_window"):
        assert np.array_equal(got[key], ref[key]), key
    assert np.array_equal(got["peak"], ref["peak"])
    finite = np.abs(np.where(np.isfinite(scores), scores, 0)).max() if scores.size else 0.0
    for a, b in zip(got, ref):
        if np.isfinite(b["mean"]):
            assert abs(float(a["mean"]) - float(b["mean"])) <= R.mean_bound(b["mean"], b["n_active"], finite), (a, b)
        else:
            assert a["mean"] == b["mean"] or (np.isnan(a["mean"]) and np.isnan(b["mean"])), (a, b)


@pytest.mark.parametrize("m,g", U.MG)
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("S", U.S_LIST)
def test_parity_with_the_reference_at_every_width(torch_cuda, seg, S, mode, m, g):
    for W in U.W_LIST:
        x = U.case_scores(W, S)
        ref, ref_counts = U.case_ref(W, S, mode, m, g)
        got, counts, total = _raw(torch_cuda, seg, x, [0, W], m, g, mode)
        _check(got, counts, total, ref, ref_counts, x)


@pytest.mark.parametrize("m,g", U.MG)
@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("S", U.RAGGED_S)
@pytest.mark.parametrize("name", sorted(U.RAGGED))
def test_parity_on_ragged_batches_with_empty_recordings(torch_cuda, seg, name, S, mode, m, g):
    x, wo = U.ragged_case(name, S)
    ref, ref_counts = R.segments(x, wo, U.ON, U.OFF, m, g, mode)          # (what these yield: tests/test_segments_cpu.py, on the reference alone)
    got, counts, total = _raw(torch_cuda, seg, x, wo, m, g, mode)
    _check(got, counts, total, ref, ref_counts, x)


def test_all_empty_recordings_and_window_offsets_that_start_late(torch_cuda, seg):
    got, counts, total = _raw(torch_cuda, seg, np.zeros((0, 3), np.float32), [0, 0, 0], 1, 0, R.INDEPENDENT)
    assert got.size == 0 and not counts.any() and list(total) == [0, 0]
    # the recordings own windows [wo[0], wo[n]) of the scores: rows in front of wo[0] belong to nobody
    x = U.case_scores(257, 3)
    ref, ref_counts = R.segments(x[40:], [0, 100, 217], U.ON, U.OFF, 3, 2)
    got, counts, total = _raw(torch_cuda, seg, x, [40, 140, 257], 3, 2, R.INDEPENDENT)
    _check(got, counts, total, ref, ref_counts, x)


@pytest.mark.parametrize("S,mode", [(1, R.INDEPENDENT), (3, R.INDEPENDENT), (65, R.INDEPENDENT), (65, R.EXCLUSIVE)])
def test_bit_identity_whatever_the_call(torch_cuda, seg, S, mode):
    torch = torch_cuda
    m, g = 3, 2
    x, wo = U.ragged_case("chunks", S)
    base, base_counts, _ = _raw(torch, seg, x, wo, m, g, mode)
    assert base.size
    n = wo.size - 1
    # alone: every recording as a call of its own
    for r in range(n):
        alone, _, _ = _raw(torch, seg, x[wo[r]:wo[r + 1]], [0, wo[r + 1] - wo[r]], m, g, mode)
        mine = base[base["recording"] == r].copy()
        mine["recording"] = 0
        assert np.array_equal(_bits(alone), _bits(mine)), r
    # a permuted batch
    perm = np.random.default_rng(5).permutation(n)
    px = np.concatenate([x[wo[r]:wo[r + 1]] for r in perm], axis=0)
    pwo = np.concatenate(([0], np.cumsum([wo[r + 1] - wo[r] for r in perm])))
    permuted, _, _ = _raw(torch, seg, px, pwo, m, g, mode)
    for at, r in enumerate(perm):
        mine = base[base["recording"] == r].copy()
        mine["recording"] = at
        assert np.array_equal(_bits(permuted[permuted["recording"] == at]), _bits(mine)), r
    # a stream of its own, the workspace dirtied by a larger call with other thresholds in front, counts not asked for
    big, bwo = U.ragged_case("long", 65)
    _raw(torch, seg, big, bwo, 1, 0, R.EXCLUSIVE, on=0.9, off=0.1)
    side = torch.cuda.Stream()
    again, none, _ = _raw(torch, seg, x, wo, m, g, mode, want_counts=False, stream=side)
    assert none is None and np.array_equal(_bits(again), _bits(base))
    if mode == R.INDEPENDENT and S > 1:
        # other columns changed: column 1 keeps its bits
        y = np.array(x)
        y[:, [s for s in range(S) if s != 1]] = np.random.default_rng(6).uniform(0, 1, (x.shape[0], S - 1)).astype(np.float32)
        other, _, _ = _raw(torch, seg, y, wo, m, g, mode)
        assert np.array_equal(_bits(other[other["column"] == 1]), _bits(base[base["column"] == 1]))
        # and alone as a single column
        one, _, _ = _raw(torch, seg, np.ascontiguousarray(x[:, 1]), wo, m, g, mode)
        mine = base[base["column"] == 1].copy()
        mine["column"] = 0
        assert np.array_equal(_bits(one), _bits(mine))


@pytest.mark.parametrize("S,mode", [(1, R.INDEPENDENT), (65, R.EXCLUSIVE)])
def test_overflow_writes_a_prefix_and_the_true_count(torch_cuda, seg, S, mode):
    torch = torch_cuda
    m, g = 3, 2
    x, wo = U.ragged_case("small", S)
    ref, ref_counts = R.segments(x, wo, U.ON, U.OFF, m, g, mode)
    full, counts, total = _raw(torch, seg, x, wo, m, g, mode)
    n_found = int(total[0])
    assert n_found == ref.size > 2 and np.array_equal(counts, ref_counts) and counts.sum() == n_found
    for room in (n_found - 1, 1, 0):
        part, counts, total = _raw(torch, seg, x, wo, m, g, mode, room=room)
        assert list(total) == [n_found, min(n_found, room)]
        assert np.array_equal(_bits(part), _bits(full[:room]))
        assert np.array_equal(counts, ref_counts)
    none, counts, total = _raw(torch, seg, x, wo, m, g, mode, want_segments=False)
    assert none.size == 0 and list(total) == [n_found, 0] and np.array_equal(counts, ref_counts)


def test_python_segmenter_retries_when_its_cap_is_too_small(torch_cuda, seg, monkeypatch):
    import dsp_amd
    torch = torch_cuda
    x, wo = U.ragged_case("small", 3)
    ref, _ = R.segments(x, wo, U.ON, U.OFF, 1, 0)
    t = torch.tensor(np.array(x), device="cuda")
    got = seg.segments(t, wo, U.ON, U.OFF)
    assert np.array_equal(_bits(got)[:, :7], _bits(ref)[:, :7])
    monkeypatch.setattr(dsp_amd.Segmenter, "CAP", 2)
    again = seg.segments(t, wo, U.ON, U.OFF)
    assert np.array_equal(_bits(again), _bits(got))
    dev = seg.segments(t, wo, U.ON, U.OFF, as_tensor=True)
    assert dev.is_cuda and dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), _bits(got))
    one = seg.segments(t[:, 0], wo, U.ON)           # off defaults to on, [Wt] is one column
    ref1, _ = R.segments(np.array(x[:, 0]), wo, U.ON, U.ON, 1, 0)
    assert np.array_equal(_bits(one)[:, :7], _bits(ref1)[:, :7])
    assert seg.segments(t[:0], [0], 0.5).size == 0 and seg.segments(t[:0], [0, 0, 0], 0.5).size == 0


def _check_end_to_end(got, ref, x):
    assert ref.size and got.size == ref.size
    for key in ("recording", "column", "first_window", "n_windows", "n_active", "peak_window", "peak"):
        assert np.array_equal(got[key], ref[key]), key
    for a, b in zip(got, ref):
        assert abs(float(a["mean"]) - float(b["mean"])) <= R.mean_bound(b["mean"], b["n_active"], np.abs(x).max())


def test_end_to_end_speakers_who_speaks_when(torch_cuda, seg):
    """2 recordings, 3 speakers: SpeakerFrontEnd -> SpeakerVerifier.scan -> Segmenter.segments(exclusive=True) equals the reference applied
    to the scan's own device output (the scan is not under test here), and the sample spans match the reference's.  The thresholds
    are taken from the scan's output: `on` the median of the windows' best LLR, `off` a quarter of the LLRs' deviation below."""
    import dsp_amd
    from tests import enroll_ref as E
    torch = torch_cuda
    rng = np.random.default_rng(11)
    lengths = (16000 * 6, 16000 * 4 + 77)
    offsets = np.concatenate(([0], np.cumsum(lengths)))
    signal = torch.tensor((0.1 * rng.standard_normal(offsets[-1])).astype(np.float32), device="cuda")
    ubm = E.random_ubm(rng, 5, 13)
    window, hop = 50, 5
    with dsp_amd.SpeakerFrontEnd() as front:
        feats, fo = front.features(signal, offsets)
        ver = dsp_amd.SpeakerVerifier(ubm)
        means = torch.tensor((np.asarray(ubm["means"], np.float32)[None] + 0.3 * rng.standard_normal((3, 5, 13))).astype(np.float32), device="cuda")
        llr = ver.scan(feats, fo, means, window, hop, want=("llr",))["llr"]
        ver.close()
        cfg = front.plan.cfg
    wo = dsp_amd.scan_window_offsets(fo, window, hop)
    x = llr.cpu().numpy()
    assert np.isfinite(x).all()
    on = float(np.median(x.max(axis=1)))
    off = on - 0.25 * float(x.std())
    got = seg.segments(llr, wo, on, off, min_windows=2, max_gap=1, exclusive=True)
    ref, _ = R.segments(x, wo, on, off, 2, 1, R.EXCLUSIVE)
    _check_end_to_end(got, ref, x)
    starts, spans = dsp_amd.segment_sample_spans(cfg, offsets, got, window, hop)
    ref_starts, ref_spans = R.sample_spans(cfg, window, hop, offsets, ref)
    assert np.array_equal(starts, ref_starts) and np.array_equal(spans, ref_spans)
    assert (starts >= offsets[got["recording"]]).all() and (starts + spans <= offsets[got["recording"] + 1]).all()


def test_end_to_end_stop_word_scanner(torch_cuda, seg, golden):
    """one recording (the reference's seven one-second clips back to back, three of them the stop word) through the 2fa scanner -> P(stop)
    per window -> segments(on = 0.5, off = 0.3) equals the reference on the scanner's own output; the sample spans are
    dsp_scan_window_spans' from the first window's start to the last window's end"""
    import dsp_amd
    torch = torch_cuda
    g = golden("stop_ref.npz")
    rec = np.concatenate([(g[f"clip{i}__pcm"] / np.float32(32768.0)).astype(np.float32) for i in range(7)])
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    stop = dsp_amd.StopModel(dict(golden("stop_model.npz")))
    scanner = dsp_amd.Scanner(plan, stop=stop, window_frames=98, hop_frames=10)
    wo, prob, _, _ = scanner.run(torch.from_numpy(rec).cuda(), [0, rec.size])
    x = prob.cpu().numpy()
    got = seg.segments(prob, wo, on=0.5, off=0.3)
    ref, _ = R.segments(x, wo, 0.5, 0.3, 1, 0)
    _check_end_to_end(got, ref, x)
    starts, spans = dsp_amd.segment_sample_spans(plan.cfg, [0, rec.size], got, 98, 10)
    ref_starts, ref_spans = R.sample_spans(plan.cfg, 98, 10, [0, rec.size], ref)
    assert np.array_equal(starts, ref_starts) and np.array_equal(spans, ref_spans)
    # against dsp_scan_window_spans itself
    n_win = int(wo[-1])
    ws, wl = np.zeros(n_win, np.int64), np.zeros(n_win, np.int64)
    off = (C.c_long * 2)(0, rec.size)
    assert seg._L.dsp_scan_window_spans(C.byref(plan.cfg), C.byref(dsp_amd.lib.ScanConfig(98, 10)), off, 1, ws.ctypes.data_as(LP), wl.ctypes.data_as(LP)) == n_win
    last = got["first_window"] + got["n_windows"] - 1
    assert np.array_equal(starts, ws[got["first_window"]]) and np.array_equal(starts + spans, ws[last] + wl[last])
    scanner.close()
    stop.close()
    plan.close()


def test_example_main_segments_prints_the_python_chains_segments(torch_cuda, seg, golden, tmp_path):
    """examples/main_segments.c on two WAV files against the same chain through the Python wrappers: the same entry points, so the same
    segments, printed"""
    import subprocess
    import dsp_amd
    from tests.enroll_util import write_wav
    torch = torch_cuda
    g = golden("stop_ref.npz")
    pcm = [np.concatenate([g[f"clip{i}__pcm"] for i in order]).astype(np.int16) for order in ((4, 0, 1, 5, 6, 2), (3, 2, 4))]
    paths = []
    for i, p in enumerate(pcm):
        paths.append(str(tmp_path / f"rec{i}.wav"))
        write_wav(paths[-1], p)
    params = dict(golden("stop_model.npz"))
    model = str(tmp_path / "stop.txt")
    U.write_stop_model(model, params)
    exe = U.build_main_segments(str(tmp_path / "main_segments"))
    r = subprocess.run([exe, "-min", "2", "-gap", "1", model] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    stop = dsp_amd.StopModel(params)
    scanner = dsp_amd.Scanner(plan, stop=stop, window_frames=98, hop_frames=10)
    rec = np.concatenate(pcm).astype(np.float32) / np.float32(32768.0)
    offsets = [0, pcm[0].size, pcm[0].size + pcm[1].size]
    wo, prob, _, _ = scanner.run(torch.from_numpy(rec).cuda(), offsets)
    got = seg.segments(prob, wo, 0.5, 0.3, min_windows=2, max_gap=1)
    assert got.size
    lines = r.stdout.strip().split("\n")
    assert lines[0] == f"{int(wo[-1])} windows, {got.size} segments" and len(lines) == 1 + got.size
    for line, s in zip(lines[1:], got):
        assert line.startswith(paths[s["recording"]]) and f"windows {s['first_window']}..{s['first_window'] + s['n_windows'] - 1} " in line
        assert f"active {s['n_active']} " in line and f"at window {s['peak_window']} " in line
    scanner.close()
    stop.close()
    plan.close()
