"""The contract of dsp_trials_evaluate_device (include/dsp_amd.h) restated in numpy: per column of a score matrix and
pooled, the threshold sweep of 2fa/audio/speaker/evaluate_gmm.py:77-81, the exact ROC step curve as counts and the AUC of
generate_charts.py:68-69.  Everything is an integer count or one float64 operation on such counts and on lo / hi, so the library is
compared with np.array_equal."""
import numpy as np

DTYPE = np.dtype([("n_target", "<i8"), ("n_nontarget", "<i8"), ("n_nan", "<i8"), ("lo", "<f8"), ("hi", "<f8"), ("best_threshold", "<f8"),
                  ("best_correct", "<i8"), ("auc_u2", "<i8"), ("auc", "<f8"), ("best_index", "<i4"), ("reserved", "<i4")])


def thresholds(lo, hi, n):
    """np.linspace(lo, hi, n) spelled out: i * step + lo in two roundings, the last one hi itself; NaN throughout when lo is"""
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(invalid="ignore"):
        t = np.arange(n, dtype=np.float64) * ((hi - lo) / np.float64(n - 1)) + lo
    t[-1] = hi
    return t


def target_lists(truth, S):
    """-> (target_offsets int64 [S + 1], target_rows int64 [targets]): the targets in (column, row) order"""
    truth = np.asarray(truth, np.int64)
    rows = np.flatnonzero(truth >= 0)
    order = np.argsort(truth[rows], kind="stable")
    offsets = np.concatenate(([0], np.cumsum(np.bincount(truth[rows], minlength=S)))).astype(np.int64)
    return offsets, rows[order].astype(np.int64)


def pairs(truth, S):
    """sum over the columns of P_s N_s before any NaN is known"""
    truth = np.asarray(truth, np.int64)
    P = np.bincount(truth[truth >= 0], minlength=S).astype(np.int64)
    return int((P * (truth.size - P)).sum())


def _sweep(tgt, non, lo, hi, n):
    """tgt, non: the non-NaN scores of the two classes as float64 -> (tp [n], fp [n], best_index, best_threshold, best_correct)"""
    t = thresholds(lo, hi, n)
    if np.isnan(lo):                                         # nothing is above a NaN
        tp = fp = np.zeros(n, np.int64)
    else:                                                    # (the scores above t_i: those behind its last place in the sorted list)
        tp = (tgt.size - np.searchsorted(np.sort(tgt), t, side="right")).astype(np.int64)
        fp = (non.size - np.searchsorted(np.sort(non), t, side="right")).astype(np.int64)
    correct = tp + (non.size - fp)
    best = int(np.argmax(correct))
    return tp, fp, best, t[best], int(correct[best])


def _range(x):
    finite = x[np.isfinite(x)]
    return (np.float64(finite.min()), np.float64(finite.max())) if finite.size else (np.float64(np.nan), np.float64(np.nan))


def evaluate(scores, truth, n=200):
    """scores float32 [T][S], truth int [T] -> dict(columns [S + 1] records, sweep_tp, sweep_fp int64 [S + 1][n], target_offsets,
    target_rows, fa_above, fa_equal int32 [targets])"""
    x = np.asarray(scores, np.float32)
    if x.ndim == 1:
        x = x[:, None]
    T, S = x.shape
    truth = np.asarray(truth, np.int64)
    assert truth.shape == (T,) and ((truth >= -1) & (truth < S)).all()
    offsets, rows = target_lists(truth, S)
    cols = np.zeros(S + 1, DTYPE)
    tps, fps = np.zeros((S + 1, n), np.int64), np.zeros((S + 1, n), np.int64)
    above, equal = np.full(rows.size, -1, np.int32), np.full(rows.size, -1, np.int32)
    pn = 0
    for s in range(S):
        col = x[:, s]
        is_t = truth == s
        ok = ~np.isnan(col)
        tgt, non = col[is_t & ok].astype(np.float64), col[~is_t & ok].astype(np.float64)
        c = cols[s]
        c["n_target"], c["n_nontarget"], c["n_nan"] = tgt.size, non.size, T - tgt.size - non.size
        c["lo"], c["hi"] = _range(col)
        tps[s], fps[s], c["best_index"], c["best_threshold"], c["best_correct"] = _sweep(tgt, non, c["lo"], c["hi"], n)
        srt = np.sort(non)
        mine = np.arange(offsets[s], offsets[s + 1])
        xj = col[rows[mine]].astype(np.float64)
        mine, xj = mine[~np.isnan(xj)], xj[~np.isnan(xj)]    # (a NaN target keeps -1 and -1)
        right, left = np.searchsorted(srt, xj, side="right"), np.searchsorted(srt, xj, side="left")
        above[mine], equal[mine] = non.size - right, right - left
        u2 = int((2 * left + (right - left)).sum())          # 2 (N - above - equal) + equal: twice the wins plus the ties
        c["auc_u2"] = u2
        c["auc"] = np.float64(u2) / np.float64(2 * tgt.size * non.size) if tgt.size * non.size else np.nan
        pn += tgt.size * non.size
    is_t = truth[:, None] == np.arange(S)[None, :]
    ok = ~np.isnan(x)
    tgt, non = x[is_t & ok].astype(np.float64), x[~is_t & ok].astype(np.float64)
    c = cols[S]
    c["n_target"], c["n_nontarget"], c["n_nan"] = tgt.size, non.size, T * S - tgt.size - non.size
    c["lo"], c["hi"] = _range(x)
    tps[S], fps[S], c["best_index"], c["best_threshold"], c["best_correct"] = _sweep(tgt, non, c["lo"], c["hi"], n)
    c["auc_u2"] = int(cols["auc_u2"][:S].sum())
    c["auc"] = np.float64(c["auc_u2"]) / np.float64(2 * pn) if pn else np.nan
    return dict(columns=cols, sweep_tp=tps, sweep_fp=fps, target_offsets=offsets, target_rows=rows, fa_above=above, fa_equal=equal)


def same(a, b):
    """np.array_equal with NaN == NaN, for float fields that may be NaN by contract (lo, hi, best_threshold, auc)"""
    return np.array_equal(a, b, equal_nan=True)


def same_columns(a, b):
    return all(same(a[name], b[name]) for name in DTYPE.names)
