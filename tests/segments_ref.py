"""Segments from window scores, restated in plain numpy with one Python loop per track (include/dsp_amd.h dsp_segments_device;
DESIGN.md 3.17).  Nothing here calls the library.

A track is one (recording r, column s) of scores[Wt][S]; recording r owns windows [wo[r], wo[r + 1]).
  1. e[w] = x[w] (independent), or x[w] where s is the row's best column and -inf elsewhere (exclusive); the best column is the smallest
     that attains the maximum of the row's non-NaN entries, a row of NaN has none
  2. state[-1] = 0; state[w] = 1 if e[w] >= on; 0 if not (e[w] >= off); else state[w - 1]
  3. runs of state 1
  4. consecutive runs with at most max_gap windows between them are joined, once
  5. spans below min_windows are dropped; nothing is joined again
  6. per survivor over its active windows: n_active, peak, peak_window (the first), mean = float32(fsum / n_active)
Output order: (recording, column, first_window)."""
import itertools
import math

import numpy as np

DTYPE = np.dtype([("recording", "<i4"), ("column", "<i4"), ("first_window", "<i4"), ("n_windows", "<i4"), ("n_active", "<i4"), ("peak_window", "<i4"),
                  ("peak", "<f4"), ("mean", "<f4")])
INDEPENDENT, EXCLUSIVE = 0, 1


def best_columns(scores):
    """[Wt][S] -> int [Wt]: the smallest column that attains the maximum of the row's non-NaN entries, -1 for a row of NaN"""
    x = np.asarray(scores, np.float32)
    best = np.full(x.shape[0], -1, np.int64)
    for w in range(x.shape[0]):
        top = None
        for s in range(x.shape[1]):
            v = x[w, s]
            if not np.isnan(v) and (top is None or v > top):
                top, best[w] = v, s
    return best


def best_columns_fast(scores):
    """the same, vectorised (tests/test_segments_cpu.py compares the two)"""
    x = np.asarray(scores, np.float32)
    if x.shape[0] == 0:
        return np.zeros(0, np.int64)
    nan = np.isnan(x)
    filled = np.where(nan, -np.inf, x)
    best = np.argmax(filled, axis=1).astype(np.int64)        # (the first of equal maxima)
    # -inf entries tie with the filling: the first entry that is really -inf, where the maximum is -inf
    low = np.isneginf(filled.max(axis=1))
    if low.any():
        real = ~nan[low]
        best[low] = np.where(real.any(axis=1), np.argmax(real, axis=1), -1)
    best[nan.all(axis=1)] = -1
    return best


def states(x, on, off):
    """step 2 for one track's effective scores -> uint8 [W]"""
    state = np.zeros(len(x), np.uint8)
    prev = 0
    on, off = np.float32(on), np.float32(off)
    for w, v in enumerate(x):
        if v >= on:
            prev = 1
        elif not (v >= off):
            prev = 0
        state[w] = prev
    return state


def runs_of(state):
    """-> [(first, last)] of the maximal stretches of 1"""
    s = np.concatenate(([0], np.asarray(state, np.int8), [0]))
    d = np.diff(s)
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


def merge_and_drop(runs, min_windows, max_gap):
    """steps 4 and 5 -> ([(first, last)] of the survivors, merges made, segments dropped)"""
    merged = []
    merges = 0
    for first, last in runs:
        if merged and first - merged[-1][1] - 1 <= max_gap:
            merged[-1][1] = last
            merges += 1
        else:
            merged.append([first, last])
    kept = [(a, b) for a, b in merged if b - a + 1 >= min_windows]
    return kept, merges, len(merged) - len(kept)


def states_fast(e, on, off):
    """states() for every column of e[W][S] at once: the state is what the last window that sets or resets left"""
    e = np.asarray(e, np.float32)
    if e.shape[0] == 0:
        return np.zeros(e.shape, np.uint8)
    with np.errstate(invalid="ignore"):
        sets, keeps = e >= np.float32(on), e >= np.float32(off)
    event = sets | ~keeps
    last = np.maximum.accumulate(np.where(event, np.arange(e.shape[0])[:, None], -1), axis=0)
    return (np.take_along_axis(sets, np.maximum(last, 0), axis=0) & (last >= 0)).astype(np.uint8)


def track_segments_plain(x, state, min_windows, max_gap):
    """one track from its scores and states -> [(first_window, n_windows, n_active, peak_window, peak, mean)], segment by segment"""
    kept, _, _ = merge_and_drop(runs_of(state), min_windows, max_gap)
    x = np.asarray(x, np.float32)
    out = []
    for a, b in kept:
        idx = a + np.flatnonzero(state[a:b + 1])
        v = x[idx]
        peak = v.max()
        out.append((a, b - a + 1, idx.size, int(idx[np.argmax(v == peak)]), peak, _mean(v.astype(np.float64).tolist(), idx.size)))
    return out


def _mean(values, n):
    try:
        total = math.fsum(values)
    except (ValueError, OverflowError):                     # +inf and -inf among the active windows (only with off = -inf)
        total = float("nan")
    return np.float32(total / n)


def track_segments(x, state, min_windows, max_gap):
    """track_segments_plain with everything but the fsum taken for all segments of the track at once (tests/test_segments_cpu.py
    compares the two)"""
    kept, _, _ = merge_and_drop(runs_of(state), min_windows, max_gap)
    if not kept:
        return []
    x = np.asarray(x, np.float32)
    W = x.size
    first, last = np.array(kept, np.int64).T
    bounds = np.stack([first, last + 1], axis=1).ravel()                   # reduceat: [first, last + 1) at the even places
    active = np.concatenate((np.asarray(state, bool), [False]))
    masked = np.where(active, np.concatenate((x, [np.float32(0)])), np.float32(-np.inf))
    n_active = (np.concatenate(([0], np.cumsum(active)))[last + 1] - np.concatenate(([0], np.cumsum(active)))[first]).astype(np.int64)
    peak = np.maximum.reduceat(masked, bounds)[::2]
    seg_of = np.full(W + 1, -1, np.int64)
    seg_of[first] = np.arange(first.size)
    seg_of = np.maximum.accumulate(seg_of)                                 # (inside a segment: its number)
    hit = active & (masked == peak[np.maximum(seg_of, 0)]) & (seg_of >= 0)
    peak_window = np.minimum.reduceat(np.where(hit, np.arange(W + 1), W + 1), bounds)[::2]
    xl, al = x.astype(np.float64).tolist(), active.tolist()
    return [(int(a), int(b - a + 1), int(n), int(pw), pk, _mean(itertools.compress(xl[a:b + 1], al[a:b + 1]), int(n)))
            for a, b, n, pw, pk in zip(first.tolist(), last.tolist(), n_active.tolist(), peak_window.tolist(), peak)]


def effective(scores, mode):
    """step 1 -> e[Wt][S]"""
    x = np.asarray(scores, np.float32)
    if mode != EXCLUSIVE:
        return x
    return np.where(np.arange(x.shape[1])[None, :] == best_columns_fast(x)[:, None], x, np.float32(-np.inf))


def all_states(scores, window_offsets, on, off, mode):
    """steps 1 and 2 for every track -> uint8 [Wt][S] (what segments() takes as `state`: it does not depend on min_windows and max_gap)"""
    e = effective(scores, mode)
    wo = np.asarray(window_offsets, np.int64)
    state = np.zeros(e.shape, np.uint8)
    for r in range(wo.size - 1):
        state[wo[r]:wo[r + 1]] = states_fast(e[wo[r]:wo[r + 1]], on, off)
    return state


def segments(scores, window_offsets, on, off, min_windows=1, max_gap=0, mode=INDEPENDENT, state=None):
    """scores [Wt] or [Wt][S] -> (segments as a DTYPE array in output order, counts int32 [n_recordings][S])"""
    x = np.asarray(scores, np.float32)
    if x.ndim == 1:
        x = x[:, None]
    wo = np.asarray(window_offsets, np.int64)
    n, S = wo.size - 1, x.shape[1]
    if state is None:
        state = all_states(x, wo, on, off, mode)
    out, counts = [], np.zeros((n, S), np.int32)
    for r in range(n):
        for s in range(S):
            found = track_segments(x[wo[r]:wo[r + 1], s], state[wo[r]:wo[r + 1], s], min_windows, max_gap)
            counts[r, s] = len(found)
            out += [(r, s) + f for f in found]
    return np.array(out, DTYPE) if out else np.zeros(0, DTYPE), counts


def capacity(window_offsets, n_columns, min_windows, max_gap):
    """the most segments a call can find: k survivors of one track need k m + (k - 1)(g + 1) <= W windows"""
    w = np.diff(np.asarray(window_offsets, np.int64))
    return int(n_columns * ((w + max_gap + 1) // (min_windows + max_gap + 1)).sum())


def mean_bound(ref_mean, n_active, max_abs):
    """what `mean` may differ by: one float32 rounding plus the any-order float64 summation bound"""
    return 2.0 ** -23 * abs(float(ref_mean)) + n_active * 2.0 ** -53 * float(max_abs)


def window_spans(cfg, window_frames, hop_frames, lengths):
    """-> per recording a list of (start, end) in samples within the recording, one per window: dsp_scan_window_spans' rule under the
    complete and stream framings; under the centred framing row i covers [i hop - frame_length / 2, i hop + frame_length / 2) and a
    window its rows' union, clipped to the recording"""
    out = []
    hop, fl = cfg.hop_length, cfg.frame_length
    for n in lengths:
        n = int(n)
        if cfg.framing == 2:
            rows = 1 + n // hop if n > 0 else 0
        elif cfg.framing == 1:
            rows = -(-n // hop) if n > 0 else 0
        else:
            rows = 1 + (n - fl) // hop if n >= fl else 0
        windows = 1 + (rows - window_frames) // hop_frames if rows >= window_frames else 1
        spans = []
        for w in range(windows):
            if cfg.framing == 2:
                last_row = w * hop_frames + max(min(window_frames, rows), 1) - 1
                spans.append((max(0, w * hop_frames * hop - fl // 2), min(n, last_row * hop + fl // 2)))
            else:
                span = window_frames * hop if cfg.framing == 1 else fl + (window_frames - 1) * hop
                a = w * hop_frames * hop
                spans.append((a, a + min(span, n - a)))
        out.append(spans)
    return out


def sample_spans(cfg, window_frames, hop_frames, offsets, segs):
    """-> (starts, lengths) int64 [n_segments]: first window's start .. last window's end, absolute positions"""
    offsets = np.asarray(offsets, np.int64)
    spans = window_spans(cfg, window_frames, hop_frames, np.diff(offsets))
    starts = np.array([offsets[g["recording"]] + spans[g["recording"]][g["first_window"]][0] for g in segs], np.int64)
    ends = np.array([offsets[g["recording"]] + spans[g["recording"]][g["first_window"] + g["n_windows"] - 1][1] for g in segs], np.int64)
    return starts, ends - starts
