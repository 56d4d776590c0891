"""The seeded cases that tests/test_trials_cpu.py (on the reference alone) and tests/test_gpu_trials.py (against the library) share, and the
kernels' constants (dsp_amd/csrc/trial_kernels.hpp; the CPU test reads them out of the header and compares) that the cases straddle.

Scores come in three kinds: "eighths" (a normal variate rounded to eighths: ties within and between the classes), "normal" (plain
float32 normal variates; targets shifted up by 1) and "grid" (every score is -3 + k / 16 with k < n_thresholds, both ends present in
every column: lo = -3 and step = 2^-4 exactly, so the thresholds are representable and scores sit on them).  The first two carry 1 % NaN,
+inf and -inf from 63 rows on, and column 4 of a "normal" matrix holds no finite score at all.  truth comes in five modes: "mixed" (random, -1 included; column 1 without a target and column 2 with
exactly one where there are that many columns), "all" (every row a target of column 0), "none" (all -1), "tile" (column 0 owns one
target more than the pair kernels' LDS tile holds, or every row but one if there are fewer) and "one" (row 0 is column 0's only
target).  Everything is computed once per case and handed out read-only."""
import functools

import numpy as np

from tests import trials_ref as R

# dsp_amd/csrc/trial_kernels.hpp
LANES_ACROSS_COLUMNS = 32            # kTrialLanesAcrossColumns: the regime switch of the min / max and pair kernels
STAT_ROWS_TIME, STAT_ROWS_COLUMNS = 4096, 64
HIST_ROWS, HIST_LDS = 1024, 64 * 1024
PAIR_ROWS_TIME, PAIR_ROWS_COLUMNS = 1024, 32          # rows per chunk (a wavefront's registers)
PAIR_TILE_TIME, PAIR_TILE_COLUMNS = 256, 32           # targets per LDS tile
SEED = 31118


def hist_columns(S, n):
    """trial_hist_columns: the columns of one histogram block"""
    fit = min(HIST_LDS // (2 * (n + 1) * 4 + 32) - 1, 64)
    if fit >= S:
        return S
    p = 1
    while 2 * p <= fit:
        p *= 2
    return p


def pair_tile(S):
    return PAIR_TILE_COLUMNS if S >= LANES_ACROSS_COLUMNS else PAIR_TILE_TIME


S_LIST = (1, 2, LANES_ACROSS_COLUMNS - 1, LANES_ACROSS_COLUMNS, LANES_ACROSS_COLUMNS + 1, 63, 64, 65, 130)
T_LIST = (1, 2, 63, 65, PAIR_ROWS_TIME + 1, 2 * PAIR_ROWS_TIME + 1)
N_LIST = (2, 200, 1024)
KINDS = ("eighths", "normal", "grid")
TRUTHS = ("mixed", "all", "none", "tile", "one")


def _cases():
    out, k = [], 0
    for S in S_LIST:
        for T in T_LIST:                                     # every (S, T); thresholds, scores and labels take turns
            out.append((T, S, N_LIST[k % 3], KINDS[(k // 3) % 3], "mixed" if k % 4 else TRUTHS[1 + (k // 4) % 4]))
            k += 1
    # the LDS tile of targets, overrun by one in both regimes and at a column group's edge; every threshold count on both sides of a
    # histogram block (hist_columns(S, n) < S and == S); the reference's own shape
    out += [(PAIR_ROWS_TIME + 1, 2, 200, "eighths", "tile"), (300, 1, 1024, "normal", "tile"), (65, 64, 2, "eighths", "tile"),
            (2 * PAIR_ROWS_TIME + 1, 65, 200, "normal", "tile"), (65, 5, 1024, "grid", "mixed"), (65, 4, 1024, "eighths", "mixed"),
            (HIST_ROWS + 1, 33, 200, "grid", "mixed"), (92, 1, 200, "normal", "mixed"), (2 * PAIR_ROWS_TIME + 1, 1, 200, "eighths", "all")]
    # the few-column regime (the reference's own) over more than one block of rows: a wavefront of the min / max pass folds
    # STAT_ROWS_TIME rows and a block of the pair pass takes 4 chunks of PAIR_ROWS_TIME, so from one row more several blocks add
    # into one column's counters; two blocks + 1 as well
    for T in (STAT_ROWS_TIME + 1, 4 * PAIR_ROWS_TIME + 1, 2 * STAT_ROWS_TIME + 1):
        for i, S in enumerate((1, 2, LANES_ACROSS_COLUMNS - 1)):
            out += [(T, S, 200, KINDS[i % 2], "mixed"), (T, S, N_LIST[i], KINDS[(i + 1) % 2], "tile")]
    return tuple(dict.fromkeys(out))


CASES = _cases()


def case_id(case):
    return "T{}-S{}-n{}-{}-{}".format(*case)


@functools.lru_cache(maxsize=None)
def case_inputs(T, S, n, kind, truth_mode, salt=0):
    """-> (scores float32 [T][S], truth int32 [T]), read-only"""
    rng = np.random.default_rng([SEED, T, S, n, KINDS.index(kind), TRUTHS.index(truth_mode), salt])
    if truth_mode == "mixed":
        truth = rng.integers(-1, S, T)
        if S >= 3:
            truth[truth == 1] = -1
            truth[truth == 2] = 0
            truth[rng.integers(T)] = 2
    elif truth_mode == "all":
        truth = np.zeros(T, np.int64)
    elif truth_mode == "none":
        truth = np.full(T, -1, np.int64)
    elif truth_mode == "tile":
        truth = rng.integers(-1, S, T)
        truth[truth == 0] = -1
        truth[rng.permutation(T)[:min(pair_tile(S) + 1, T - 1)]] = 0
    else:
        truth = np.full(T, -1, np.int64)
        truth[0] = 0
    is_t = truth[:, None] == np.arange(S)[None, :]
    if kind == "grid":
        x = (np.float32(-3.0) + rng.integers(0, n, (T, S)).astype(np.float32) / np.float32(16.0)).astype(np.float32)
        if T >= 2:
            x[0, :] = -3.0
            x[T - 1, :] = np.float32(-3.0 + (n - 1) / 16.0)
    else:
        x = rng.standard_normal((T, S)).astype(np.float32)
        if kind == "eighths":
            x = (np.round((x + is_t * np.float32(0.5)) * 8) / 8).astype(np.float32)
        else:
            x = (x + is_t.astype(np.float32)).astype(np.float32)
        if T >= 63:
            u = rng.random((T, S))
            x[u < 0.004] = np.nan
            x[(u >= 0.004) & (u < 0.007)] = np.inf
            x[(u >= 0.007) & (u < 0.01)] = -np.inf
        if kind == "normal" and S >= 5:                      # a column without a finite score
            x[:, 4] = np.resize(np.array([np.inf, -np.inf, np.nan], np.float32), T)
    truth = truth.astype(np.int32)
    x.setflags(write=False)
    truth.setflags(write=False)
    return x, truth


@functools.lru_cache(maxsize=None)
def case_ref(T, S, n, kind, truth_mode, salt=0):
    """the reference's answer for case_inputs(...), its arrays read-only"""
    x, truth = case_inputs(T, S, n, kind, truth_mode, salt)
    ref = R.evaluate(x, truth, n)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def facts():
    """What the cases exercise, from the inputs and the reference alone."""
    f = dict(ties=0, no_targets=0, no_nontargets=0, one_target=0, nan=0, nan_targets=0, pos_inf=0, neg_inf=0, on_threshold=0, flat=0, no_finite=0,
             argmax_ties=0, over_tile_time=0, over_tile_columns=0, hist_split=0, hist_whole=0)
    for case in CASES:
        T, S, n = case[:3]
        x, truth = case_inputs(*case)
        ref = case_ref(*case)
        cols = ref["columns"][:S]
        f["ties"] += int((ref["fa_equal"] > 0).sum())
        f["no_targets"] += int(((cols["n_target"] == 0) & (cols["n_nontarget"] > 0)).sum())
        f["no_nontargets"] += int(((cols["n_nontarget"] == 0) & (cols["n_target"] > 0)).sum())
        f["one_target"] += int((cols["n_target"] == 1).sum())
        f["nan"] += int(cols["n_nan"].sum())
        f["nan_targets"] += int((ref["fa_above"] < 0).sum())
        f["pos_inf"] += int(np.isposinf(x).sum())
        f["neg_inf"] += int(np.isneginf(x).sum())
        f["flat"] += int((cols["lo"] == cols["hi"]).sum())
        f["no_finite"] += int(np.isnan(cols["lo"]).sum())
        per_column = np.diff(ref["target_offsets"])
        f["over_tile_time" if S < LANES_ACROSS_COLUMNS else "over_tile_columns"] += int((per_column > pair_tile(S)).sum())
        f["hist_split" if hist_columns(S, n) < S else "hist_whole"] += 1
        for s in range(S):
            if np.isnan(cols["lo"][s]):
                continue
            t = R.thresholds(cols["lo"][s], cols["hi"][s], n)
            f["on_threshold"] += int(np.isin(x[:, s].astype(np.float64), t[1:-1]).sum())
            correct = ref["sweep_tp"][s] + cols["n_nontarget"][s] - ref["sweep_fp"][s]
            f["argmax_ties"] += int((correct == correct.max()).sum() > 1)
    return f
