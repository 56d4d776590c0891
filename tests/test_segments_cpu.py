"""CPU: segments from window scores (include/dsp_amd.h dsp_segment*) -- the numpy restatement against hand-written
answers, the host-only entries of the library (capacity, sample spans, refusals: no device is touched), and that the seeded cases of
tests/segments_util.py exercise what tests/test_gpu_segments.py relies on.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import segments_ref as R
from tests import segments_util as U

LP = C.POINTER(C.c_long)
NAN, INF = float("nan"), float("inf")


def _seg(x, on, off, m=1, g=0, mode=R.INDEPENDENT):
    x = np.asarray(x, np.float32)
    segs, counts = R.segments(x, [0, x.shape[0]], on, off, m, g, mode)
    assert counts.sum() == segs.size
    return [tuple(int(s[k]) for k in ("column", "first_window", "n_windows", "n_active", "peak_window")) + (float(s["peak"]), float(s["mean"])) for s in segs]


# on = 0.5, off = 0.25 everywhere: all values are exact in float32
HAND = [
    # x == on sets, x == off keeps, just below off resets
    ([0.5, 0.25, 0.25, 0.125, 0.25], 1, 0, [(0, 0, 3, 3, 0, 0.5, (0.5 + 0.25 + 0.25) / 3)]),
    # the band alone never switches on; state[-1] = 0
    ([0.25, 0.375, 0.5, 0.375], 1, 0, [(0, 2, 2, 2, 2, 0.5, 0.4375)]),
    # NaN resets, and is never active; +inf sets and is the peak; -inf resets
    ([1.0, NAN, 0.375, INF, 0.375, -INF, 0.375], 1, 0, [(0, 0, 1, 1, 0, 1.0, 1.0), (0, 3, 2, 2, 3, INF, INF)]),
    # a gap of exactly max_gap joins (the gap windows belong to the segment but are not active), max_gap + 1 does not
    ([1, 0, 0, 2, 0, 0, 0, 1], 1, 2, [(0, 0, 4, 2, 3, 2.0, 1.5), (0, 7, 1, 1, 7, 1.0, 1.0)]),
    # a span of exactly min_windows survives, min_windows - 1 is dropped
    ([1, 1, 1, 0, 1, 1, 0], 3, 0, [(0, 0, 3, 3, 0, 1.0, 1.0)]),
    # merging comes first: two runs of 1 with a gap of 1 span 3 = min_windows
    ([1, 0, 1, 0, 0, 1], 3, 1, [(0, 0, 3, 2, 0, 1.0, 1.0)]),
    # a dropped run between two survivors: whatever is dropped lies more than max_gap from both neighbours, so they stay apart (the rule
    # "not joined again" fixes the order merge, then drop; no input can tell it from drop, then merge)
    ([1, 1, 1, 0, 0, 1, 0, 0, 1, 1, 1], 2, 1, [(0, 0, 3, 3, 0, 1.0, 1.0), (0, 8, 3, 3, 8, 1.0, 1.0)]),
    # the first of equal peaks
    ([0.75, 1.5, 0.375, 1.5], 1, 0, [(0, 0, 4, 4, 1, 1.5, (0.75 + 1.5 + 0.375 + 1.5) / 4)]),
    # a track that ends switched on, one window, nothing
    ([0, 1], 1, 0, [(0, 1, 1, 1, 1, 1.0, 1.0)]),
    ([1], 1, 0, [(0, 0, 1, 1, 0, 1.0, 1.0)]),
    ([0.375], 1, 0, []),
    ([], 1, 0, []),
]


@pytest.mark.parametrize("x,m,g,want", HAND)
def test_reference_against_hand_written_tracks(x, m, g, want):
    got = _seg(np.asarray(x, np.float32).reshape(-1, 1), 0.5, 0.25, m, g)
    assert got == [tuple(w[:6]) + (float(np.float32(w[6])),) for w in want]          # (mean is rounded once to float32)


def test_reference_exclusive_ties_and_rows_of_nan():
    x = np.array([[1.0, 1.0, 0.0],         # a tie: the smallest column
                  [0.375, 2.0, 2.0],       # column 1
                  [NAN, NAN, NAN],         # no best column: every track is reset
                  [NAN, 0.375, 1.0],       # NaN is not a candidate
                  [0.375, 0.375, 0.3125],  # a tie inside the band: column 0 keeps -- but it is off
                  [-INF, NAN, -INF]], np.float32)
    assert R.best_columns(x).tolist() == [0, 1, -1, 2, 0, 0] == R.best_columns_fast(x).tolist()
    assert _seg(x, 0.5, 0.25, mode=R.EXCLUSIVE) == [(0, 0, 1, 1, 0, 1.0, 1.0), (1, 1, 1, 1, 1, 2.0, 2.0), (2, 3, 1, 1, 3, 1.0, 1.0)]
    # independent: every column on its own
    assert [s[:3] for s in _seg(x, 0.5, 0.25)] == [(0, 0, 2), (1, 0, 2), (2, 1, 1), (2, 3, 2)]
    # exclusive, the band inherits only in the best column: column 2 leads rows 0-1, row 2 is column 2's band
    y = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.375], [0.4375, 0.0, 0.375]], np.float32)
    assert [s[:4] for s in _seg(y, 0.5, 0.25, mode=R.EXCLUSIVE)] == [(2, 0, 2, 2)]


@pytest.mark.parametrize("S", U.S_LIST)
def test_fast_forms_of_the_reference_equal_the_plain_ones(S):
    """The parity tests compare against the vectorised forms; here they are held to the plain loops over the whole shared grid: every W,
    both modes, every (min_windows, max_gap) -- every column up to 257 windows and at S <= 3, one column per dwell beyond (the plain loops
    take a microsecond per window and column)."""
    for W in U.W_LIST:
        x = U.case_scores(W, S)
        if W <= 257 or S <= 3:
            assert np.array_equal(R.best_columns(x), R.best_columns_fast(x))
        columns = range(S) if W <= 257 or S <= 3 else range(min(S, len(U.DWELLS)))
        for mode in U.MODES:
            e = R.effective(x, mode)
            st = U.case_states(W, S, mode)
            for s in columns:
                assert np.array_equal(st[:, s], R.states(e[:, s], U.ON, U.OFF))
                for m, g in U.MG:
                    plain, fast = R.track_segments_plain(x[:, s], st[:, s], m, g), R.track_segments(x[:, s], st[:, s], m, g)
                    assert len(plain) == len(fast)
                    for a, b in zip(plain, fast):
                        assert a[:5] == b[:5] and (a[5] == b[5] or (np.isnan(a[5]) and np.isnan(b[5])))


def _capacity(wo, S, m, g):
    wo = np.ascontiguousarray(wo, np.int64)
    cfg = dl.SegmentConfig(0.5, 0.5, m, g, 0)
    return dsp_amd.load().dsp_segments_capacity(C.byref(cfg), wo.ctypes.data_as(LP), wo.size - 1, S)


def test_capacity_is_the_formula_and_is_met_exactly():
    for wo, S, m, g in (([0, 10, 10, 25], 3, 3, 2), ([5, 5], 1, 1, 0), ([0, 1, 2, 4097], 130, 70, 0), ([0, 8193], 2, 1, 65)):
        want = S * sum((b - a + g + 1) // (m + g + 1) for a, b in zip(wo[:-1], wo[1:]))
        assert _capacity(wo, S, m, g) == want == R.capacity(wo, S, m, g) == dsp_amd.segments_capacity(wo, S, m, g)
    # the adversarial track: min_windows on, max_gap + 1 off, repeated -- nothing joins, nothing is dropped
    for m, g in U.MG + ((2, 1),):
        for W in (1, m - 1, m, m + g, m + g + 1, 2 * m + g + 1, 10 * (m + g + 1) + m - 1, 10 * (m + g + 1) + m):
            if W < 1:
                continue
            x = np.tile(np.r_[np.ones(m), np.zeros(g + 1)], W // (m + g + 1) + 1)[:W].astype(np.float32)
            segs, _ = R.segments(x, [0, W], 0.5, 0.5, m, g)
            full = [s for s in segs if s["n_windows"] == m]
            assert len(full) == R.capacity([0, W], 1, m, g) == _capacity([0, W], 1, m, g)
            assert segs.size == len(full)
    # no seeded case exceeds it
    for S, mode in ((1, 0), (3, 1), (65, 0)):
        for W in U.W_LIST:
            for m, g in U.MG:
                assert U.case_ref(W, S, mode, m, g)[0].size <= R.capacity([0, W], S, m, g)
    assert dsp_amd.segments_capacity([0], 1) == 0


def _window_spans(cfg, wf, hf, offsets):
    L = dsp_amd.load()
    off = np.ascontiguousarray(offsets, np.int64)
    scan = dl.ScanConfig(wf, hf)
    n = L.dsp_scan_window_spans(C.byref(cfg), C.byref(scan), off.ctypes.data_as(LP), off.size - 1, None, None)
    if n < 0:
        return None
    starts, lengths = np.zeros(n, np.int64), np.zeros(n, np.int64)
    assert L.dsp_scan_window_spans(C.byref(cfg), C.byref(scan), off.ctypes.data_as(LP), off.size - 1, starts.ctypes.data_as(LP), lengths.ctypes.data_as(LP)) == n
    return starts, lengths


def _some_segments(offsets, cfg, wf, hf):
    """every (first, n) with n in 1, 2, all, per recording"""
    out = []
    for r, spans in enumerate(R.window_spans(cfg, wf, hf, np.diff(offsets))):
        W = len(spans)
        for first in range(W):
            for n in {1, min(2, W - first), W - first}:
                out.append((r, 0, first, n, n, first, 1.0, 1.0))
    return np.array(out, R.DTYPE)


def test_sample_spans_follow_the_window_spans():
    offsets = np.array([7, 7 + 16000 * 3 + 11, 7 + 16000 * 3 + 11 + 399, 7 + 16000 * 5], np.int64)          # the middle recording: shorter than one window
    # the 512-point plan: dsp_scan_window_spans itself, first window's start .. last window's end
    cfg = dsp_amd.default_config()
    for wf, hf in ((98, 10), (30, 45)):
        ws, wl = _window_spans(cfg, wf, hf, offsets)
        base = np.concatenate(([0], np.cumsum([len(s) for s in R.window_spans(cfg, wf, hf, np.diff(offsets))])))
        segs = _some_segments(offsets, cfg, wf, hf)
        starts, lengths = dsp_amd.segment_sample_spans(cfg, offsets, segs, wf, hf)
        first = base[segs["recording"]] + segs["first_window"]
        last = first + segs["n_windows"] - 1
        assert np.array_equal(starts, ws[first]) and np.array_equal(starts + lengths, ws[last] + wl[last])
        rs, rl = R.sample_spans(cfg, wf, hf, offsets, segs)
        assert np.array_equal(starts, rs) and np.array_equal(lengths, rl)
        assert (lengths[segs["recording"] == 1] == 399).all()
    # the speaker plan is centred: dsp_scan_window_spans refuses it (its windows are not cut out as clips), the segments' spans are the
    # union of the rows' frames, row i = [i hop - frame_length / 2, i hop + frame_length / 2), clipped to the recording
    spk = dsp_amd.speaker_config()
    assert _window_spans(spk, 100, 10, offsets) is None and "DSP_FRAMING_CENTER" in dl.last_error()
    segs = _some_segments(offsets, spk, 100, 10)
    starts, lengths = dsp_amd.segment_sample_spans(spk, offsets, segs, 100, 10)
    rs, rl = R.sample_spans(spk, 100, 10, offsets, segs)
    assert np.array_equal(starts, rs) and np.array_equal(lengths, rl)
    rec0 = segs["recording"] == 0
    w = segs["first_window"][rec0]
    assert np.array_equal(starts[rec0], 7 + np.maximum(0, w * 10 * 160 - 200))
    n0 = int(offsets[1] - offsets[0])
    last_row = (w + segs["n_windows"][rec0] - 1) * 10 + 99
    assert np.array_equal(starts[rec0] + lengths[rec0], 7 + np.minimum(n0, last_row * 160 + 200))
    assert (lengths[segs["recording"] == 1] == 399).all() and (starts[segs["recording"] == 1] == offsets[1]).all()
    # a segment outside its recording's windows
    bad = np.array([(1, 0, 0, 2, 2, 0, 1.0, 1.0)], R.DTYPE)
    with pytest.raises(dsp_amd.DspError, match="outside the windows"):
        dsp_amd.segment_sample_spans(cfg, offsets, bad, 98, 10)
    with pytest.raises(dsp_amd.DspError, match="no such recording"):
        dsp_amd.segment_sample_spans(cfg, offsets, np.array([(3, 0, 0, 1, 1, 0, 1.0, 1.0)], R.DTYPE), 98, 10)


def test_refusals_touch_no_device():
    L = dsp_amd.load()
    h = C.c_void_p()
    assert L.dsp_segmenter_create(0, C.byref(h)) == 0 and h.value
    L.dsp_segmenter_destroy(h)
    assert L.dsp_segmenter_create(-1, C.byref(h)) == -1 and "device" in dl.last_error()
    assert L.dsp_segmenter_create(0, None) == -1
    assert L.dsp_segmenter_create(0, C.byref(h)) == 0
    wo = (C.c_long * 3)(0, 4, 9)
    total = C.c_void_p(64)          # never dereferenced: every call below is refused before a device is touched
    scores, segs = C.c_void_p(64), C.c_void_p(64)
    good = dict(on=0.5, off=0.25, min_windows=1, max_gap=0, mode=0)

    def call(cfg=good, d_scores=scores, n=2, offsets=wo, S=1, d_segments=segs, room=4, d_total=total, handle=None):
        c = None if cfg is None else dl.SegmentConfig(cfg["on"], cfg["off"], cfg["min_windows"], cfg["max_gap"], cfg["mode"])
        return L.dsp_segments_device(h if handle is None else handle, d_scores, n, offsets, S, None if c is None else C.byref(c), d_segments, room, None,
                                     d_total, None)

    refused = [
        (dict(cfg=None), "NULL"),
        (dict(cfg=dict(good, on=NAN)), "NaN"),
        (dict(cfg=dict(good, off=NAN)), "NaN"),
        (dict(cfg=dict(good, off=0.75)), "off must be <= on"),
        (dict(cfg=dict(good, min_windows=0)), "min_windows"),
        (dict(cfg=dict(good, max_gap=-1)), "max_gap"),
        (dict(cfg=dict(good, mode=2)), "mode"),
        (dict(cfg=dict(good, mode=-1)), "mode"),
        (dict(d_scores=None), "d_scores is NULL"),
        (dict(offsets=None), "window_offsets is NULL"),
        (dict(d_total=None), "d_total is NULL"),
        (dict(offsets=(C.c_long * 3)(-1, 4, 9)), "non-negative"),
        (dict(offsets=(C.c_long * 3)(0, 5, 4)), "decrease at recording 1"),
        (dict(S=0), "n_columns"),
        (dict(S=(1 << 19) + 1), "n_columns"),
        (dict(room=-1), "max_segments"),
        (dict(n=-1), "n_recordings"),
        (dict(handle=C.c_void_p()), "segmenter is NULL"),
    ]
    for kwargs, word in refused:
        assert call(**kwargs) == -1, kwargs
        assert word in dl.last_error(), (kwargs, dl.last_error())
    assert call(n=0) == 0                                   # no recording: DSP_OK, no launch
    assert call(d_segments=None, room=-1, n=0) == 0         # max_segments is ignored without d_segments
    cfg = dl.SegmentConfig(0.5, 0.75, 1, 0, 0)
    assert L.dsp_segments_capacity(C.byref(cfg), wo, 2, 1) == -1 and "off must be <= on" in dl.last_error()
    assert L.dsp_segments_capacity(None, wo, 2, 1) == -1
    L.dsp_segmenter_destroy(h)
    L.dsp_segmenter_destroy(None)
    with pytest.raises(ValueError):
        dsp_amd.segments_capacity([0, 3], 1, 0, 0)
    with pytest.raises(ValueError):
        dsp_amd.segments_capacity([3, 0])


def test_ctypes_mirrors_match_the_header():
    assert C.sizeof(dl.Segment) == 32 == R.DTYPE.itemsize == np.dtype(dl.SEGMENT_DTYPE).itemsize
    assert C.sizeof(dl.SegmentConfig) == 20
    assert [f[0] for f in dl.Segment._fields_] == list(R.DTYPE.names) == [f[0] for f in dl.SEGMENT_DTYPE]


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("S", U.S_LIST)
def test_the_shared_cases_are_not_vacuous(S, mode):
    facts = U.family_facts(S, mode)
    for key in ("survivors", "merges", "drops", "cross64", "cross4096", "inherited"):
        assert facts[key] >= 1, (key, facts)
    # the three zones, NaN, both infinities and both thresholds themselves occur
    x = np.concatenate([U.case_scores(W, S).ravel() for W in U.W_LIST])
    with np.errstate(invalid="ignore"):
        assert (x > U.ON).any() and ((x > U.OFF) & (x < U.ON)).any() and (x < U.OFF).any()
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x == U.ON).any() and (x == U.OFF).any()


@pytest.mark.parametrize("name", sorted(U.RAGGED))
def test_the_ragged_cases_hold_empty_recordings_and_segments(name):
    """every ragged family -- one batch at one S and mode, over the four (min_windows, max_gap) -- yields survivors, merges and drops,
    and survivors in more than one recording; with min_windows <= 3 every single case yields survivors.  (min_windows = 70 leaves
    nothing of recordings below 70 windows, and little of the exclusive mode's short stretches: there the answer to match is the
    drops and the zero counts.)"""
    ws = U.RAGGED[name]
    assert 0 in ws
    if name != "long":
        assert ws[0] == 0 and ws[-1] == 0 and 0 in ws[1:-1]
    for S in U.RAGGED_S:
        x, wo = U.ragged_case(name, S)
        for mode in U.MODES:
            st = R.all_states(x, wo, U.ON, U.OFF, mode)
            survivors, merges, drops, recordings = 0, 0, 0, set()
            for m, g in U.MG:
                segs, _ = R.segments(x, wo, U.ON, U.OFF, m, g, mode, state=st)
                assert segs.size or m > 3, (S, mode, m, g)
                survivors += segs.size
                recordings |= set(segs["recording"].tolist())
                for r in range(wo.size - 1):
                    for s in range(S):
                        _, a, d = R.merge_and_drop(R.runs_of(st[wo[r]:wo[r + 1], s]), m, g)
                        merges, drops = merges + a, drops + d
            assert survivors and merges and drops and len(recordings) > 1, (S, mode, survivors, merges, drops)
    # what tests/test_gpu_segments.py asserts of its own cases: the overflow test needs more than two segments to cut
    for S, mode in ((1, R.INDEPENDENT), (65, R.EXCLUSIVE)):
        x, wo = U.ragged_case("small", S)
        assert R.segments(x, wo, U.ON, U.OFF, 3, 2, mode)[0].size > 2
    for S, mode in ((1, R.INDEPENDENT), (3, R.INDEPENDENT), (65, R.INDEPENDENT), (65, R.EXCLUSIVE)):
        x, wo = U.ragged_case("chunks", S)
        assert R.segments(x, wo, U.ON, U.OFF, 3, 2, mode)[0].size


def test_example_main_segments_links_and_refuses_bad_arguments(tmp_path):
    exe = U.build_main_segments(str(tmp_path / "main_segments"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    bad = tmp_path / "model.txt"
    bad.write_text("13 500 4 2\n")
    r = subprocess.run([exe, str(bad), "nothing.wav"], capture_output=True, text=True)
    assert r.returncode == 1 and "not a stop model" in r.stderr
