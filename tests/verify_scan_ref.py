"""The float speaker scan (include/dsp_amd.h dsp_speaker_float_scan_device) restated in numpy, from its definition:

    windows   a recording of R rows: R >= window gives 1 + (R - window) // hop windows, window w = rows [w hop, w hop + window); fewer
              rows one window of all R.  The windows of all recordings lie back to back.
    per row   ll of tests/verify_ref.py row_ll -- computed once per row and model, whatever the number of windows the row lies in
    per window and model   L = the float64 sum of the window's ll in verify_ref.clip_sum's order, the window taken as a clip: tiles of 64
              rows from the WINDOW's first row, the adjacent pairwise tree inside a tile (absent rows 0), the tiles in ascending order
    outputs   formed from L_u, L_s and the window's row count exactly as verify_ref.verify forms a clip's

float64 by default; dtype=np.float32 is verify_ref's model of the GPU arithmetic.  window_sums is clip_sum for all models and all windows
of one recording at once (the same additions of the same float64 values in the same order, elementwise over an array instead of one
window at a time: clip_sum per (window, model) in Python takes minutes over the shared cases); tests/test_verify_scan_cpu.py proves it
equal to clip_sum, and scan() equal to verify() on cut-out windows.  numpy only."""
import numpy as np

from tests import verify_ref as V


def window_counts(frame_offsets, window, hop):
    """rows per recording -> windows per recording, by the rule above"""
    rows = np.diff(np.asarray(frame_offsets, np.int64))
    return np.where(rows >= window, 1 + (rows - window) // hop, 1).astype(np.int64)


def window_spans(frame_offsets, window, hop):
    """-> (start [Wt], n [Wt]): every window's first row in the matrix and its row count, recordings in order"""
    fo = np.asarray(frame_offsets, np.int64)
    start, n = [], []
    for r, w in enumerate(window_counts(fo, window, hop)):
        rows = int(fo[r + 1] - fo[r])
        if rows < 1:
            raise ValueError(f"recording {r} has no rows")
        start.append(fo[r] + hop * np.arange(w, dtype=np.int64))
        n.append(np.full(w, min(window, rows), np.int64))
    return np.concatenate(start), np.concatenate(n)


def rows_ll(x, ubm, means, dtype=np.float64):
    """x [n][d] -> ll [1 + S][n] in `dtype`: model 0 the UBM, model 1 + s speaker s (lc, means[s], ic)"""
    lc, mu, ic = V.model_of(ubm, dtype)
    x = np.asarray(x).astype(dtype)
    return np.stack([V.row_ll(x, lc, c, ic, dtype) for c in [mu] + list(np.asarray(means).astype(dtype))])


def window_sums(ll, n, hop, count):
    """ll [M][R] of one recording -> L [M][count] float64: windows of n rows starting at 0, hop, 2 hop, ..., each summed as clip_sum sums"""
    win = np.lib.stride_tricks.sliding_window_view(ll, n, axis=1)[:, ::hop][:, :count]          # [M][count][n]
    tiles = -(-n // V.TILE_ROWS)
    a = np.zeros(win.shape[:2] + (tiles * V.TILE_ROWS,), np.float64)
    a[:, :, :n] = win.astype(np.float64)
    a = a.reshape(win.shape[:2] + (tiles, V.TILE_ROWS))
    while a.shape[3] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return np.cumsum(a[..., 0], axis=2, dtype=np.float64)[:, :, -1]


def outputs(L, n, dtype=np.float64):
    """L [1 + S][Wt] float64 sums and n [Wt] rows -> the five outputs, formed as verify_ref.verify forms them"""
    rows = n.astype(np.float64)
    L_u, L_s = L[0], L[1:].T                                                                    # [Wt], [Wt][S]
    out = {"llr": ((L_s - L_u[:, None]) / rows[:, None]).astype(dtype), "ll_ubm": (L_u / rows).astype(dtype),
           "ll_target": (L_s / rows[:, None]).astype(dtype)}
    out["best"] = np.argmax(out["llr"], axis=1).astype(np.int32)                                # the first of the largest
    out["best_llr"] = out["llr"][np.arange(n.size), out["best"]]
    return out


def scan_from_ll(ll, base, frame_offsets, window, hop, dtype=np.float64):
    """ll [1 + S][rows] of the matrix rows from `base` on (rows_ll) -> the five outputs over all windows"""
    fo = np.asarray(frame_offsets, np.int64)
    _, n = window_spans(fo, window, hop)
    counts = window_counts(fo, window, hop)
    L = np.concatenate([window_sums(ll[:, fo[r] - base:fo[r + 1] - base], int(min(window, fo[r + 1] - fo[r])), hop, int(counts[r]))
                        for r in range(fo.size - 1)], axis=1)
    return outputs(L, n, dtype)


def scan(x, frame_offsets, ubm, means, window, hop, dtype=np.float64):
    """recording r = rows [fo[r], fo[r + 1]) of x, means [S][k][d] -> dict(llr [Wt][S], ll_ubm [Wt], ll_target [Wt][S], best [Wt], best_llr [Wt])"""
    fo = np.asarray(frame_offsets, np.int64)
    return scan_from_ll(rows_ll(x[fo[0]:fo[-1]], ubm, means, dtype), int(fo[0]), fo, window, hop, dtype)


def cut_windows(x, frame_offsets, window, hop):
    """the windows as clips of their own -> (rows [sum n][d], clip offsets [Wt + 1])"""
    start, n = window_spans(frame_offsets, window, hop)
    idx = np.concatenate([np.arange(s, s + m) for s, m in zip(start, n)])
    return np.asarray(x)[idx], np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
