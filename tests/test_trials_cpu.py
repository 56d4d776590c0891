"""No GPU: the restatement of the trial evaluation (tests/trials_ref.py) against hand-written columns, against the reference's own
expressions (evaluate_gmm.py:77-81), against sklearn and against the reference's recorded trial list (tests/golden/gmm_trials_ref.npz);
the host-only entries and every refusal of the built library; the symbols; and that the shared cases of tests/trials_util.py hold
what tests/test_gpu_trials.py relies on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import trials_ref as R
from tests import trials_util as U

NAN, INF = float("nan"), float("inf")
LP, IP = C.POINTER(C.c_long), C.POINTER(C.c_int)
TRIAL_SYMBOLS = ["dsp_trials_target_offsets", "dsp_trials_pairs", "dsp_trial_evaluator_create", "dsp_trial_evaluator_destroy", "dsp_trials_evaluate_device"]


def _one(x, labels, n=5):
    """one column: labels 1 = target -> (its record, tp, fp, fa_above, fa_equal)"""
    out = R.evaluate(np.asarray(x, np.float32), np.where(np.asarray(labels) == 1, 0, -1), n)
    return out["columns"][0], out["sweep_tp"][0].tolist(), out["sweep_fp"][0].tolist(), out["fa_above"].tolist(), out["fa_equal"].tolist()


def test_hand_written_a_score_on_a_threshold_is_not_above_it():
    # lo 0, hi 4, n 5: thresholds 0 1 2 3 4; targets 2 and 4, non-targets 0, 1, 2
    c, tp, fp, above, equal = _one([0, 1, 2, 2, 4], [0, 0, 0, 1, 1])
    assert R.thresholds(0, 4, 5).tolist() == [0, 1, 2, 3, 4]
    assert tp == [2, 2, 1, 1, 0] and fp == [2, 1, 0, 0, 0]
    assert (c["n_target"], c["n_nontarget"], c["n_nan"], c["lo"], c["hi"]) == (2, 3, 0, 0.0, 4.0)
    # correct = tp + N - fp = 3 4 4 4 3: the first of the three
    assert (c["best_index"], c["best_threshold"], c["best_correct"]) == (1, 1.0, 4)
    # target 2 ties one non-target and beats two; target 4 beats all three
    assert above == [0, 0] and equal == [1, 0]
    assert c["auc_u2"] == (2 * 2 + 1) + 2 * 3 and c["auc"] == 11 / 12


def test_hand_written_flat_column_and_empty_classes():
    c, tp, fp, above, equal = _one([0.5, 0.5, 0.5], [1, 0, 0], 4)                      # lo == hi: every threshold is lo
    assert R.thresholds(0.5, 0.5, 4).tolist() == [0.5] * 4 and tp == [0] * 4 and fp == [0] * 4
    assert (c["best_index"], c["best_threshold"], c["best_correct"]) == (0, 0.5, 2) and above == [0] and equal == [2]
    assert c["auc_u2"] == 2 and c["auc"] == 0.5
    c, tp, fp, above, equal = _one([1, 2, 3], [0, 0, 0], 3)                            # no targets
    assert tp == [0, 0, 0] and fp == [2, 1, 0] and (c["best_index"], c["best_correct"]) == (2, 3)
    assert above == [] and c["auc_u2"] == 0 and np.isnan(c["auc"])
    c, tp, fp, above, equal = _one([1, 2, 3], [1, 1, 1], 3)                            # no non-targets
    assert tp == [2, 1, 0] and fp == [0, 0, 0] and (c["best_index"], c["best_correct"]) == (0, 2)
    assert above == [0, 0, 0] and equal == [0, 0, 0] and c["auc_u2"] == 0 and np.isnan(c["auc"])


def test_hand_written_nan_and_infinities():
    #   NaN target, NaN non-target: out of everything; +inf above every threshold, -inf above none; lo / hi from the finite ones
    c, tp, fp, above, equal = _one([NAN, NAN, INF, -INF, 1, 3, INF, -INF], [1, 0, 1, 1, 1, 0, 0, 0], 3)
    assert (c["n_target"], c["n_nontarget"], c["n_nan"], c["lo"], c["hi"]) == (3, 3, 2, 1.0, 3.0)
    assert tp == [1, 1, 1] and fp == [2, 2, 1]
    assert above == [-1, 0, 2, 2] and equal == [-1, 1, 1, 0]                           # (+inf == +inf, -inf == -inf)
    assert c["auc_u2"] == (2 * 2 + 1) + 1 + 2 * 1
    c, tp, fp, above, equal = _one([NAN, INF, -INF], [0, 1, 0], 3)                     # no finite score: NaN thresholds, nothing above
    assert np.isnan(c["lo"]) and np.isnan(c["hi"]) and np.isnan(c["best_threshold"]) and tp == [0] * 3 and fp == [0] * 3
    assert (c["best_index"], c["best_correct"], c["n_nan"]) == (0, 1, 1) and above == [0] and c["auc"] == 1.0


def test_hand_written_truth_of_none_first_argmax_and_the_pooled_row():
    x = np.array([[0, 5], [1, 1], [2, 0], [3, 2]], np.float32)
    out = R.evaluate(x, [-1, 1, 0, -1], 4)
    cols = out["columns"]
    assert out["target_offsets"].tolist() == [0, 1, 2] and out["target_rows"].tolist() == [2, 1]
    assert cols["n_target"].tolist() == [1, 1, 2] and cols["n_nontarget"].tolist() == [3, 3, 6]
    # column 0: thresholds 0 1 2 3, target 2: tp 1 1 0 0, fp 2 1 1 0 (non-targets 0 1 3) -> correct 2 3 2 3: the first 3
    assert out["sweep_tp"][0].tolist() == [1, 1, 0, 0] and out["sweep_fp"][0].tolist() == [2, 1, 1, 0] and cols["best_index"][0] == 1
    assert out["fa_above"].tolist() == [1, 2] and out["fa_equal"].tolist() == [0, 0]
    assert cols["auc_u2"].tolist() == [4, 2, 6] and cols["auc"].tolist() == [4 / 6, 2 / 6, 6 / 12]
    assert (cols["lo"][2], cols["hi"][2]) == (0.0, 5.0) and R.pairs([-1, 1, 0, -1], 2) == 6


@pytest.mark.parametrize("seed", range(6))
def test_restatement_against_the_reference_lines(seed):
    rng = np.random.default_rng(seed)
    T, n = (92, 200) if seed < 3 else (501, 1024)
    llrs = rng.standard_normal(T).astype(np.float32).astype(np.float64) if seed % 2 else np.round(rng.standard_normal(T) * 4) / 4
    labels = (rng.random(T) < 0.4).astype(np.int64)
    thresholds = np.linspace(min(llrs), max(llrs), n)                                 # evaluate_gmm.py:77-79
    accs = [np.mean((llrs > t) == labels) for t in thresholds]
    best_t = thresholds[np.argmax(accs)]
    c, tp, fp, _, _ = _one(llrs, labels, n)
    assert np.array_equal(R.thresholds(c["lo"], c["hi"], n), thresholds) and np.array_equal(dsp_amd.trial_thresholds(c["lo"], c["hi"], n), thresholds)
    assert tp == [int(((llrs > t) & (labels == 1)).sum()) for t in thresholds] and fp == [int(((llrs > t) & (labels == 0)).sum()) for t in thresholds]
    assert c["best_index"] == np.argmax(accs) and c["best_threshold"] == best_t and c["best_correct"] == round(max(accs) * T)


def _as_result(ref, x, truth):
    """the reference's dict with what TrialEvaluator.evaluate adds for roc_points"""
    rows = ref["target_rows"]
    return dict(ref, target_scores=np.asarray(x, np.float32).reshape(len(truth), -1)[rows, np.asarray(truth)[rows]])


@pytest.mark.parametrize("T,ties", [(92, False), (300, True), (5000, True), (5000, False)])
def test_restatement_against_sklearn(T, ties):
    from sklearn.metrics import auc, roc_curve
    rng = np.random.default_rng(T + ties)
    labels = (rng.random(T) < 0.3).astype(np.int64)
    x = (rng.standard_normal(T) + labels).astype(np.float32)
    if ties:
        x = (np.round(x * 8) / 8).astype(np.float32)
    truth = np.where(labels == 1, 0, -1)
    ref = R.evaluate(x, truth, 200)
    c = ref["columns"][0]
    fpr, tpr, thr = roc_curve(labels, x, drop_intermediate=False)
    N, P = int(c["n_nontarget"]), int(c["n_target"])
    fps, tps = np.rint(fpr * N).astype(np.int64), np.rint(tpr * P).astype(np.int64)
    assert np.abs(fps - fpr * N).max() < 1e-6
    xt = x[ref["target_rows"]]
    at = np.searchsorted(-thr[1:], -xt.astype(thr.dtype)) + 1                          # each target's point: accept when x >= x_j
    assert np.array_equal(thr[at], xt)
    assert np.array_equal(fps[at], ref["fa_above"].astype(np.int64) + ref["fa_equal"])
    assert np.array_equal(tps[at], [(xt >= v).sum() for v in xt])
    area = auc(fpr, tpr)
    assert abs(c["auc"] - area) <= 1e-12
    # roc_points: the corners of sklearn's curve -- every point is one of sklearn's, those at a target's score with its threshold,
    # and the area is the same
    f, t, h = dsp_amd.roc_points(_as_result(ref, x, truth), 0)
    assert f[0] == 0 and t[0] == 0 and h[0] == np.inf and f[-1] == 1 and t[-1] == 1 and (np.diff(h) < 0).all()
    theirs = set(zip(fpr.tolist(), tpr.tolist()))
    assert all(point in theirs for point in zip(f.tolist(), t.tolist()))
    at_target = np.isin(h, xt.astype(np.float64))
    where = np.searchsorted(-thr[1:].astype(np.float64), -h[at_target]) + 1
    assert at_target.sum() == np.unique(xt).size and np.array_equal(thr[where], h[at_target])
    assert np.array_equal(fpr[where], f[at_target]) and np.array_equal(tpr[where], t[at_target])
    assert abs(auc(f, t) - area) <= 1e-12


def test_recorded_trials_of_the_reference(golden):
    g = golden("gmm_trials_ref.npz")
    x, labels = g["llr"].astype(np.float32), g["label"]
    assert x.size == 92 and int(labels.sum()) == 36
    ref = R.evaluate(x, np.where(labels == 1, 0, -1), 200)
    c = ref["columns"][0]
    assert (c["n_target"], c["n_nontarget"], c["n_nan"]) == (36, 56, 0)
    assert c["best_threshold"] == g["best_t"] and c["best_index"] == g["best_index"] and c["best_correct"] == g["best_correct"] == 85
    assert abs(c["best_threshold"] - 0.24) < 0.005                                     # evaluate_gmm.py DEFAULT_THRESHOLD
    assert abs(c["auc"] - g["auc"]) <= 1e-12 and abs(g["auc"] - 0.95436507) < 1e-6
    fps = np.rint(g["fpr_all"] * 56).astype(np.int64)
    xt = x[ref["target_rows"]]
    at = np.searchsorted(-g["roc_thresholds_all"][1:], -xt.astype(np.float64)) + 1
    assert np.array_equal(g["roc_thresholds_all"][at], xt) and np.array_equal(fps[at], ref["fa_above"].astype(np.int64) + ref["fa_equal"])
    # the pooled row of one column is the column
    assert R.same_columns(ref["columns"][:1], ref["columns"][1:]) and np.array_equal(ref["sweep_tp"][0], ref["sweep_tp"][1])


def test_library_host_code_against_the_hand_written_columns():
    """the same columns through what the library itself computes without a device: the thresholds of rule 1 (dsp_amd.trial_thresholds),
    the target lists and the pair count (dsp_trials_target_offsets, dsp_trials_pairs), and roc_points on the hand-written counts"""
    L = dsp_amd.load()
    assert dsp_amd.trial_thresholds(0, 4, 5).tolist() == [0, 1, 2, 3, 4]
    assert dsp_amd.trial_thresholds(0.5, 0.5, 4).tolist() == [0.5] * 4
    assert dsp_amd.trial_thresholds(1, 3, 3).tolist() == [1, 2, 3] and np.isnan(dsp_amd.trial_thresholds(NAN, NAN, 3)).all()
    t = dsp_amd.trial_thresholds(-3, -3 + 199 / 16, 200)
    assert np.array_equal(t, -3 + np.arange(200) / 16) and t[-1] == 9.4375               # representable thresholds: exact
    t = dsp_amd.trial_thresholds(0.1, 0.7, 4)
    assert t.tolist() == [0.1, 1 * ((0.7 - 0.1) / 3) + 0.1, 2 * ((0.7 - 0.1) / 3) + 0.1, 0.7]      # two roundings, the last one hi
    # [[0, 5], [1, 1], [2, 0], [3, 2]] with truth -1 1 0 -1
    truth = (C.c_int * 4)(-1, 1, 0, -1)
    off, rows = (C.c_long * 3)(), (C.c_long * 2)()
    assert L.dsp_trials_target_offsets(truth, 4, 2, off, rows) == 2 and list(off) == [0, 1, 2] and list(rows) == [2, 1]
    assert L.dsp_trials_pairs(truth, 4, 2) == 6
    # [0, 1, 2, 2, 4] with targets 2 and 4: rows 3 and 4, 2 x 3 pairs; the counts of the hand-written test as a curve
    truth = (C.c_int * 5)(-1, -1, -1, 0, 0)
    off, rows = (C.c_long * 2)(), (C.c_long * 2)()
    assert L.dsp_trials_target_offsets(truth, 5, 1, off, rows) == 2 and list(off) == [0, 2] and list(rows) == [3, 4]
    assert L.dsp_trials_pairs(truth, 5, 1) == 6
    cols = np.zeros(2, R.DTYPE)
    cols["n_target"], cols["n_nontarget"] = 2, 3
    res = dict(columns=cols, target_offsets=np.array(off), target_scores=np.array([2, 4], np.float32), fa_above=np.array([0, 0], np.int32),
               fa_equal=np.array([1, 0], np.int32))
    f, tp, h = dsp_amd.roc_points(res, 0)
    # accept at >= 4: one target, no false accept; at >= 2: both targets and the tied non-target; then everything
    assert f.tolist() == [0, 0, 1 / 3, 1] and tp.tolist() == [0, 0.5, 1, 1] and h.tolist() == [INF, 4, 2, -INF]
    assert float(((f[1:] - f[:-1]) * (tp[1:] + tp[:-1])).sum() / 2) == pytest.approx(11 / 12, abs=1e-15)


def test_host_entries_through_the_library():
    L = dsp_amd.load()
    for case in U.CASES[::5]:
        _, truth = U.case_inputs(*case)
        T, S = case[:2]
        tr = np.ascontiguousarray(truth, np.intc)
        off, rows = np.zeros(S + 1, np.int64), np.zeros(T, np.int64)
        n = L.dsp_trials_target_offsets(tr.ctypes.data_as(IP), T, S, off.ctypes.data_as(LP), rows.ctypes.data_as(LP))
        want_off, want_rows = R.target_lists(truth, S)
        assert n == want_rows.size and np.array_equal(off, want_off) and np.array_equal(rows[:n], want_rows)
        assert L.dsp_trials_target_offsets(tr.ctypes.data_as(IP), T, S, None, None) == n
        assert L.dsp_trials_pairs(tr.ctypes.data_as(IP), T, S) == R.pairs(truth, S)
    assert L.dsp_trials_pairs(None, 0, 3) == 0 and L.dsp_trials_target_offsets(None, 0, 3, None, None) == 0
    bad = (C.c_int * 3)(0, 2, -1)
    assert L.dsp_trials_pairs(bad, 3, 2) == -1 and "truth[1] = 2" in dl.last_error()
    assert L.dsp_trials_target_offsets(bad, 3, 2, None, None) == -1 and "truth[1] = 2" in dl.last_error()
    assert L.dsp_trials_pairs(None, 3, 2) == -1 and "truth is NULL" in dl.last_error()
    assert L.dsp_trials_pairs(bad, 3, 0) == -1 and "n_columns" in dl.last_error()
    assert L.dsp_trials_pairs(bad, -1, 2) == -1 and "n_rows" in dl.last_error()


def test_refusals_touch_no_device():
    L = dsp_amd.load()
    h = C.c_void_p()
    assert L.dsp_trial_evaluator_create(0, C.byref(h)) == 0 and h.value
    L.dsp_trial_evaluator_destroy(h)
    assert L.dsp_trial_evaluator_create(-1, C.byref(h)) == -1 and "device" in dl.last_error()
    assert L.dsp_trial_evaluator_create(0, None) == -1
    assert L.dsp_trial_evaluator_create(0, C.byref(h)) == 0
    truth = (C.c_int * 4)(0, -1, 1, 0)
    ptr = C.c_void_p(64)              # never dereferenced: every call below is refused before a device is touched
    outs = dict(cols=ptr, tp=ptr, fp=ptr, above=ptr, equal=ptr)

    def call(n=200, d_scores=ptr, T=4, S=2, tr=truth, handle=None, cfg=True, **kw):
        o = dict(outs, **kw)
        c = dl.TrialsConfig(n)
        return L.dsp_trials_evaluate_device(h if handle is None else handle, d_scores, T, S, tr, C.byref(c) if cfg else None, o["cols"], o["tp"], o["fp"],
                                            o["above"], o["equal"], None)

    big = np.zeros(1 << 24, np.intc)                         # 2^23 targets of column 0 against 2^23 others, and as many of column 1
    big[1::2] = 1
    refused = [
        (dict(handle=C.c_void_p()), "evaluator is NULL"),
        (dict(cfg=False), "dsp_trials_config is NULL"),
        (dict(n=1), "n_thresholds must be 2 .. 1024, got 1"),
        (dict(n=1025), "n_thresholds must be 2 .. 1024, got 1025"),
        (dict(S=0), "n_columns"),
        (dict(S=(1 << 19) + 1), "n_columns"),
        (dict(T=-1), "n_rows"),
        (dict(T=1 << 31), "2^31 rows"),
        (dict(cols=None, tp=None, fp=None, above=None, equal=None), "every output is NULL"),
        (dict(d_scores=None), "d_scores is NULL"),
        (dict(tr=None), "truth is NULL"),
        (dict(tr=(C.c_int * 4)(0, -2, 1, 0)), "truth[1] = -2"),
        (dict(tr=(C.c_int * 4)(0, 1, 1, 2)), "truth[3] = 2"),
        (dict(T=big.size, tr=big.ctypes.data_as(IP)), str(2 * (1 << 23) * (1 << 23)) + " pairs"),
        (dict(T=big.size, tr=big.ctypes.data_as(IP), cols=None, above=None), str(1 << 47) + " pairs"),
    ]
    for kwargs, word in refused:
        assert call(**kwargs) == -1, kwargs
        assert word in dl.last_error(), (kwargs, dl.last_error())
    assert call(T=0) == 0 and call(T=0, d_scores=None, tr=None) == 0      # no trial: DSP_OK, no launch
    L.dsp_trial_evaluator_destroy(h)
    L.dsp_trial_evaluator_destroy(None)
    for bad in (dict(lo=0, hi=1, n=1), dict(lo=0, hi=1, n=1025)):
        with pytest.raises(ValueError):
            dsp_amd.trial_thresholds(**bad)
    with pytest.raises(ValueError):
        dsp_amd.roc_points({}, 0)


def test_symbols_are_declared_exported_and_listed():
    L = dsp_amd.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dsp_amd.build.LIB], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsp_amd.h")) as f:
        header = f.read()
    for name in TRIAL_SYMBOLS:
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported and re.search(r"\b%s\(" % name, header), name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_trial")) == sorted(TRIAL_SYMBOLS)
    assert {"TrialEvaluator", "trial_thresholds", "roc_points"} <= set(dsp_amd.__all__)


def test_ctypes_mirrors_match_the_header():
    assert C.sizeof(dl.TrialColumn) == 80 == R.DTYPE.itemsize == np.dtype(dl.TRIAL_COLUMN_DTYPE).itemsize
    assert C.sizeof(dl.TrialsConfig) == 4
    assert [f[0] for f in dl.TrialColumn._fields_] == list(R.DTYPE.names) == [f[0] for f in dl.TRIAL_COLUMN_DTYPE]
    assert [np.dtype(dl.TRIAL_COLUMN_DTYPE).fields[k][1] for k in R.DTYPE.names] == [getattr(dl.TrialColumn, k).offset for k in R.DTYPE.names]


def test_constants_are_the_kernels():
    with open(os.path.join(os.path.dirname(dsp_amd.build.LIB), "csrc", "trial_kernels.hpp")) as f:
        src = f.read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        return eval(expr.replace("L", ""), {"kTrialPairRegsTime": 16})               # noqa: S307  (our own header: "64 * 1024", "1L << 19")

    assert const("kTrialLanesAcrossColumns") == U.LANES_ACROSS_COLUMNS
    assert (const("kTrialStatRowsTime"), const("kTrialStatRowsColumns")) == (U.STAT_ROWS_TIME, U.STAT_ROWS_COLUMNS)
    assert (const("kTrialHistRows"), const("kTrialHistLds")) == (U.HIST_ROWS, U.HIST_LDS)
    assert const("kTrialPairRegsTime") == 16
    assert (const("kTrialPairRowsTime"), const("kTrialPairRowsColumns")) == (U.PAIR_ROWS_TIME, U.PAIR_ROWS_COLUMNS)
    assert (const("kTrialPairTileTime"), const("kTrialPairTileColumns")) == (U.PAIR_TILE_TIME, U.PAIR_TILE_COLUMNS)
    assert [U.hist_columns(S, n) for S, n in ((1, 2), (130, 2), (31, 200), (130, 200), (5, 1024), (7, 1024), (3, 1024))] == [1, 64, 31, 32, 5, 4, 3]


def test_the_shared_cases_are_not_vacuous():
    f = U.facts()
    for key, least in f.items():
        assert least >= 1, (key, f)
    Ss, Ts, ns = {c[1] for c in U.CASES}, {c[0] for c in U.CASES}, {c[2] for c in U.CASES}
    assert {1, 2, U.LANES_ACROSS_COLUMNS - 1, U.LANES_ACROSS_COLUMNS, U.LANES_ACROSS_COLUMNS + 1, 63, 64, 65, 130} <= Ss
    assert {1, 2, 63, 65, U.PAIR_ROWS_TIME + 1, 2 * U.PAIR_ROWS_TIME + 1} <= Ts and ns == {2, 200, 1024}
    # more than one block of rows in both regimes: across columns (4 x 32 rows per block) and along rows, where a wavefront of the
    # min / max pass folds STAT_ROWS_TIME rows and a block of the pair pass takes 4 x PAIR_ROWS_TIME -- at S = 1, 2 and one below the
    # switch, with random labels and with the target tile overrun, one row past a block and past two (T_LIST holds those inside one)
    assert any(T > 4 * U.PAIR_ROWS_COLUMNS and S >= U.LANES_ACROSS_COLUMNS for T, S, *_ in U.CASES)
    for S in (1, 2, U.LANES_ACROSS_COLUMNS - 1):
        for truth in ("mixed", "tile"):
            Ts = {c[0] for c in U.CASES if c[1] == S and c[4] == truth}
            assert {U.STAT_ROWS_TIME + 1, 4 * U.PAIR_ROWS_TIME + 1, 2 * U.STAT_ROWS_TIME + 1} <= Ts, (S, truth, Ts)
    assert any(T > U.HIST_ROWS for T, *_ in U.CASES) and any(T > 4 * U.STAT_ROWS_COLUMNS and S >= U.LANES_ACROSS_COLUMNS for T, S, *_ in U.CASES)
