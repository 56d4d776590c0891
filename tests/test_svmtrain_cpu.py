"""CPU: the float64 restatement of SVM training (tests/svmtrain_ref.py) against sklearn's libsvm, the host helpers of the C ABI
(dsp_svm_folds, dsp_svm_balanced_weights, dsp_svm_model_from_training) against the restatement, the argument checks of every
dsp_svm_train_* entry point and the loud failure without a GPU.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from dsp_amd import scrubjay as sj

from tests import svm_ref as S
from tests import svmtrain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("nf40", "nf3", "nf1", "cepstrum")
SPREAD = R.SPREAD


@pytest.fixture(scope="module")
def sets(golden):
    g = golden("svmtrain.npz")
    out = {}
    for name in SETS:
        d = {k: g[f"{name}__{k}"] for k in ("x", "labels", "offset", "scale", "gamma", "c", "dual_coef", "support", "intercept", "decision_function", "predict")}
        d["z"] = R.standardise(d["x"], d["offset"], d["scale"])
        d["d2"] = R.distances(d["z"])
        d["gamma"] = float(d["gamma"])
        out[name] = d
    return out


def _problems(name, d):
    if name == "cepstrum":                                             # (8 rows: sklearn's problem only)
        return [("all", np.arange(d["labels"].size, dtype=np.int32), d["c"][0], d["c"][1], d["gamma"])]
    return R.suite_problems(d["labels"], d["c"], d["gamma"], d["x"].shape[1])


@pytest.mark.parametrize("name", SETS)
def test_restatement_is_libsvm(sets, name):
    """The restatement at eps = 1e-9 against sklearn's SVC at tol = 1e-9 (tests/golden/svmtrain.npz): decision values of all rows and
    the intercept within 1e-7 absolute -- with qfloat32, the one thing libsvm does that the trainer does not: the rows of Q it caches
    are float32 (svm.cpp Qfloat).  Measured: 7e-10 .. 7e-9 with it.  Without it, in float64 throughout as the kernels compute, the
    restatement stands 6.3e-8 (nf40), 2.9e-6 (nf3), 9.3e-7 (nf1), 6.8e-8 (cepstrum) from sklearn: libsvm's own rounding, not the solver's
    path.  The support set and the scaler convention are checked on the way."""
    d = sets[name]
    n = d["labels"].size
    rows = np.arange(n)
    assert np.allclose(d["c"], R.balanced_weights(d["labels"], 10.0 if name != "nf1" else 1.0), rtol=1e-15)
    s = R.solve(d["d2"], d["labels"], rows, d["c"][0], d["c"][1], d["gamma"], 1e-9, qfloat32=True)
    dec = R.decisions(d["d2"], s, d["gamma"])
    want = -d["decision_function"]
    allow = 1e-7 * max(1.0, np.abs(want).max() / 10.0)
    assert s["status"] == R.CONVERGED and np.abs(dec - want).max() <= allow and abs(s["rho"] + d["intercept"]) <= allow
    if name != "nf3":                                              # (nf3 has duplicated rows: its alphas are not unique, its decisions are)
        assert np.array_equal(np.nonzero(s["coef"])[0], np.sort(d["support"]))                   # (support_ lists class 0's first)
        assert np.abs(s["coef"][d["support"]] + d["dual_coef"]).max() <= 1e-5 * max(1.0, np.abs(d["dual_coef"]).max())
    assert np.array_equal(np.where(dec > 0, 0, 1), d["predict"])


def test_restatement_against_live_sklearn():
    """the same on a fresh seeded set, where sklearn imports: n = 64 and 200, 40 features, C = 10, balanced"""
    svm = pytest.importorskip("sklearn.svm")
    for n in (64, 200):
        rng = np.random.default_rng(n)
        labels = (rng.random(n) < 0.4).astype(np.int32)
        labels[:2] = 0, 1
        x = ((rng.standard_normal((n, 40)) + labels[:, None] * rng.standard_normal(40)) * rng.uniform(0.5, 5.0, 40)).astype(np.float32)
        z = R.standardise(x, *R.scaler_fit(x))
        gamma = 1.0 / (40 * z.astype(np.float64).var())
        clf = svm.SVC(kernel="rbf", C=10.0, gamma=gamma, class_weight="balanced", tol=1e-9).fit(z.astype(np.float64), labels)
        d2 = R.distances(z)
        s = R.solve(d2, labels, np.arange(n), *R.balanced_weights(labels, 10.0), gamma, 1e-9, qfloat32=True)
        assert np.abs(R.decisions(d2, s, gamma) + clf.decision_function(z.astype(np.float64))).max() <= 1e-7
        assert abs(s["rho"] + clf.intercept_[0]) <= 1e-7


def test_sigmoid_train_against_sklearn(sets):
    """sigmoid_train against sklearn.calibration._sigmoid_calibration on the restated fit's held-out decisions: the same objective
    (Platt's, with the prior-smoothed targets) under another optimiser (L-BFGS), so a loose check.  Observed |dA|, |dB| on the four
    sets: 2.3e-8 / 2.7e-8, 7.7e-9 / 6.4e-9, 3.1e-8 / 1.5e-8, 1.4e-7 / 2.2e-7.  Both stop on a gradient of about 1e-5 and the
    objective's Hessian is of order n p (1 - p) >= 1e-1 here: 1e-4 absolute."""
    cal = pytest.importorskip("sklearn.calibration")
    for name in SETS:
        d = sets[name]
        _attrs, parts = R.fit(d["x"], d["labels"], c=10.0 if name != "nf1" else 1.0, gamma=d["gamma"], eps=1e-7)
        a, b, it = R.sigmoid_train(parts["dec_cv"], d["labels"])
        a2, b2 = cal._sigmoid_calibration(parts["dec_cv"], (d["labels"] == 0).astype(np.float64))
        print(f"{name}: A {a:.9f} B {b:.9f} after {it} steps, sklearn {a2:.9f} {b2:.9f}")
        assert it < 100 and abs(a - a2) <= 1e-4 and abs(b - b2) <= 1e-4


@pytest.mark.parametrize("name", SETS)
def test_restatement_spread(sets, name):
    """The restatement's own spread max |dec_ref(1e-7) - dec_ref(1e-10)| (decisions of all rows, and rho) over the problems the GPU
    tests solve stays within SPREAD, the figure their allowance is four times of; the problems have the structure their names
    promise; and the restated end-to-end fit labels every training row as sklearn does with no row inside SvmRef's bound."""
    d = sets[name]
    worst = 0.0
    for pn, rows, c0, c1, gamma in _problems(name, d):
        a = R.solve(d["d2"], d["labels"], rows, c0, c1, gamma, 1e-7)
        b = R.solve(d["d2"], d["labels"], rows, c0, c1, gamma, 1e-10)
        worst = max(worst, np.abs(R.decisions(d["d2"], a, gamma) - R.decisions(d["d2"], b, gamma)).max(), abs(a["rho"] - b["rho"]))
        assert a["status"] == b["status"] == R.CONVERGED and a["gap"] < 1e-7
        if pn == "bounded":
            assert a["n_bounded"] == a["n_sv"] == rows.size
        if pn == "unbounded":
            assert a["n_bounded"] == 0 and a["n_sv"] > 0
        if pn == "single":
            assert (d["labels"][rows] == 1).sum() == 1
    print(f"{name}: spread {worst:.3e}")
    assert worst <= SPREAD[name]
    attrs, _parts = R.fit(d["x"], d["labels"], c=10.0 if name != "nf1" else 1.0, gamma=d["gamma"], eps=1e-7)
    label, dec, bound, _p1 = S.SvmRef(attrs).predict(d["x"])
    assert (np.abs(dec) < bound).sum() <= 0.01 * label.size and np.array_equal(label, d["predict"])


@pytest.mark.parametrize("name", SETS)
def test_restatement_spread_q_float32(sets, name):
    """the spread of the restatement with the kernel rounded to float32, on the problem on all rows: what the q_float32 mode's parity with
    sklearn on the GPU takes four times of; at eps = 1e-7 the restatement itself stands within that of sklearn"""
    d = sets[name]
    rows = np.arange(d["labels"].size)
    a, b = (R.solve(d["d2"], d["labels"], rows, d["c"][0], d["c"][1], d["gamma"], eps, qfloat32=True) for eps in (1e-7, 1e-10))
    da, db = R.decisions(d["d2"], a, d["gamma"]), R.decisions(d["d2"], b, d["gamma"])
    worst = max(np.abs(da - db).max(), abs(a["rho"] - b["rho"]))
    print(f"{name}: spread {worst:.3e}, at 1e-7 from sklearn {np.abs(da + d['decision_function']).max():.3e}")
    assert worst <= R.SPREAD_Q32[name] and np.abs(da + d["decision_function"]).max() <= 4 * R.SPREAD_Q32[name]


def test_cross_validation_spread(sets):
    """the same spread over the problems of the cross-validation test: three outer folds of nf3, a 2 x 2 grid"""
    d = sets["nf3"]
    ids = R.folds(d["labels"].size, R.CV_FOLDS, R.CV_SEED)
    a, b = (R.cv_reference(d["x"], d["labels"], ids, *R.CV_GRID, eps) for eps in (1e-7, 1e-10))
    print(f"cv: spread {np.abs(a - b).max():.3e}")
    assert np.abs(a - b).max() <= SPREAD["cv"]


def test_folds_weights_and_compaction(sets):
    L = dsp_amd.load()
    for n, k, seed in ((8, 5, 0), (70, 5, 1), (257, 3, 2**63 + 5), (5, 5, 7), (300, 1, 9)):
        ids = sj.svm_folds(n, k, seed)
        assert np.array_equal(ids, R.folds(n, k, seed))
        assert sorted(np.bincount(ids, minlength=k)) == sorted((f + 1) * n // k - f * n // k for f in range(k))
    assert not np.array_equal(sj.svm_folds(70, 5, 1), sj.svm_folds(70, 5, 2))
    d = sets["nf3"]
    labels = d["labels"]
    assert sj.svm_balanced_weights(labels, 10.0) == pytest.approx(R.balanced_weights(labels, 10.0), rel=1e-15)
    rows = np.arange(0, 120, 3)
    assert sj.svm_balanced_weights(labels, 2.5, rows) == pytest.approx(R.balanced_weights(labels, 2.5, rows), rel=1e-15)
    with pytest.raises(dsp_amd.DspError, match="label 1 has no row"):
        sj.svm_balanced_weights(np.zeros(4, np.int32))
    with pytest.raises(dsp_amd.DspError, match="neither 0 nor 1"):
        sj.svm_balanced_weights(np.array([0, 1, 2], np.int32))
    s = R.solve(d["d2"], labels, np.arange(labels.size), d["c"][0], d["c"][1], d["gamma"], 1e-3)
    want = R.model_from_training(d["z"], labels, s["coef"], s["rho"], d["gamma"], d["offset"], d["scale"], 0.0, 0.0)
    sv, coef, n0 = sj.svm_model_from_training(d["z"], labels, s["coef"])
    assert np.array_equal(sv, want["sv"]) and np.array_equal(coef, want["coef"]) and n0 == want["vectors_per_class"][0] and 0 < n0 < coef.size
    z, lab, cf = np.ascontiguousarray(d["z"]), np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(s["coef"])
    assert L.dsp_svm_model_from_training(z.ctypes.data, lab.ctypes.data, cf.ctypes.data, lab.size, 3, None, None, 0, None) == coef.size     # (counting)
    assert L.dsp_svm_model_from_training(z.ctypes.data, lab.ctypes.data, cf.ctypes.data, lab.size, 3, sv.ctypes.data, coef.ctypes.data, coef.size - 1, None) == -1
    assert "capacity" in dl.last_error()


def test_argument_checks_come_before_any_device():
    L = dsp_amd.load()
    h = C.c_void_p()
    assert L.dsp_svm_trainer_create(0, 3, None) == -1 and "out is NULL" in dl.last_error()
    assert L.dsp_svm_trainer_create(-1, 3, C.byref(h)) == -1 and L.dsp_svm_trainer_create(0, 0, C.byref(h)) == -1 and "n_features" in dl.last_error()
    assert L.dsp_svm_trainer_create(0, 3, C.byref(h)) == 0 and h.value                                  # (touches no device)
    feat = np.zeros((4, 3), np.float32)
    fp = feat.ctypes.data                                                                               # (never read: every call below fails first)
    off = np.zeros(3, np.float32)
    rows = np.array([0, 4], np.int32)

    def set_(t=h, f=fp, n=4, sr=None, nsr=0, o=None, s=None):
        return L.dsp_svm_train_set_device(t, f, n, sr, nsr, o, s, None, None, None)

    for call, msg in ((lambda: set_(t=None), "trainer is NULL"), (lambda: set_(f=None), "d_feat is NULL"), (lambda: set_(n=1), "n must be >= 2"),
                      (lambda: set_(n=8193), "above the cap of 8192"), (lambda: set_(o=off.ctypes.data), "given together"),
                      (lambda: set_(sr=rows.ctypes.data, nsr=2), r"scaler_rows\[1\] = 4 is out of range"), (lambda: set_(sr=rows.ctypes.data, nsr=0), "n_scaler_rows")):
        assert call() == -1 and re.search(msg, dl.last_error()), (msg, dl.last_error())
    nan = np.array([0, np.nan, 0], np.float32)
    assert set_(o=nan.ctypes.data, s=off.ctypes.data) == -1 and "feature 1 is not finite" in dl.last_error()
    # no dataset yet
    labels = np.array([0, 1, 0, 1], np.int32)
    res = np.zeros(2, dl.SVM_TRAIN_RESULT_DTYPE)
    prob = (dl.SvmTrainProblem * 1)(dl.SvmTrainProblem(rows.ctypes.data, 2, 1.0, 1.0, 0.5))
    assert L.dsp_svm_train_problems_device(h, prob, 1, None, labels.ctypes.data, res.ctypes.data, fp, None, None) == -1 and "no dataset" in dl.last_error()
    a, b = C.c_double(), C.c_double()
    assert L.dsp_svm_platt_fit_device(h, fp, labels.ctypes.data, None, 0, C.byref(a), C.byref(b), None, None) == -1 and "no dataset" in dl.last_error()
    assert L.dsp_svm_train_rows_host(h, fp, None) == -1 and "no dataset" in dl.last_error()
    for eps, it, q32, msg in ((0.0, 0, 0, "eps"), (np.nan, 0, 0, "eps"), (np.inf, 0, 0, "eps"), (1e-3, -1, 0, "max_iter"), (1e-3, 100000001, 0, "max_iter"),
                              (1e-3, 0, 2, "q_float32"), (1e-3, 0, -1, "q_float32")):
        cfg = dl.SvmTrainConfig(eps, it, q32)
        assert L.dsp_svm_train_problems_device(h, prob, 1, C.byref(cfg), labels.ctypes.data, res.ctypes.data, fp, None, None) == -1 and msg in dl.last_error()
    assert L.dsp_svm_train_problems_device(None, prob, 1, None, labels.ctypes.data, res.ctypes.data, fp, None, None) == -1 and "trainer is NULL" in dl.last_error()
    # dsp_svm_fit_device: the same checks, and its own
    out = {k: np.zeros(s, np.float32) for k, s in (("offset", 3), ("scale", 3), ("sv", 12), ("coef", 4))}
    model = dl.SvmFitModel(*[out[k].ctypes.data for k in ("offset", "scale", "sv", "coef")])
    folds = np.array([0, 1, 0, 2], np.int32)

    def fit(t=h, f=fp, n=4, lab=labels, ids=None, k=2, c0=1.0, c1=1.0, gamma=0.5, cfg=None, m=model):
        return L.dsp_svm_fit_device(t, f, n, None if lab is None else lab.ctypes.data, None if ids is None else ids.ctypes.data, k, 0, c0, c1, gamma, cfg,
                                    None if m is None else C.byref(m), None)

    bad_cfg = dl.SvmTrainConfig(-1.0, 0, 0)
    for call, msg in ((lambda: fit(t=None), "trainer is NULL"), (lambda: fit(f=None), "d_feat is NULL"), (lambda: fit(n=1), "n must be >= 2"),
                      (lambda: fit(n=8193), "above the cap"), (lambda: fit(lab=None), "labels is NULL"),
                      (lambda: fit(lab=np.array([0, 1, 2, 0], np.int32)), r"labels\[2\] = 2 is neither 0 nor 1"), (lambda: fit(k=1), "k_prob"), (lambda: fit(k=5), "k_prob"),
                      (lambda: fit(ids=folds), r"fold_ids\[3\] = 2 is outside"), (lambda: fit(c0=0.0), "c_label0"), (lambda: fit(c1=np.inf), "c_label1"),
                      (lambda: fit(gamma=np.nan), "gamma"), (lambda: fit(gamma=-1.0), "gamma"), (lambda: fit(cfg=C.byref(bad_cfg)), "eps"),
                      (lambda: fit(m=None), "model and its arrays"), (lambda: fit(m=dl.SvmFitModel()), "model and its arrays")):
        assert call() == -1 and re.search(msg, dl.last_error()), (msg, dl.last_error())
    if L.dsp_device_count() <= 0:                                                                       # loud: there is no CPU fallback
        assert set_() == -2 and "no HIP device" in dl.last_error()
        assert fit() == -2 and "no HIP device" in dl.last_error()
    L.dsp_svm_trainer_destroy(h)
    L.dsp_svm_trainer_destroy(None)
    assert L.dsp_svm_folds(0, 1, 0, labels.ctypes.data) == -1 and L.dsp_svm_folds(4, 5, 0, labels.ctypes.data) == -1 and "k must be 1 .. n" in dl.last_error()
    assert L.dsp_svm_folds(4, 2, 0, None) == -1 and "fold_ids is NULL" in dl.last_error()


def test_the_feature_is_wired_in():
    L = dsp_amd.load()
    header = open(os.path.join(ROOT, "include", "dsp_amd.h")).read()
    names = ["dsp_svm_trainer_create", "dsp_svm_trainer_destroy", "dsp_svm_train_set_device", "dsp_svm_train_rows_host", "dsp_svm_train_problems_device",
             "dsp_svm_platt_fit_device", "dsp_svm_folds", "dsp_svm_balanced_weights", "dsp_svm_model_from_training", "dsp_svm_fit_device"]
    for name in names:
        assert name in dl.SYMBOLS and hasattr(L, name) and re.search(r"\b%s\(" % name, header), name
    assert "capi_svmtrain.cpp" in dsp_amd.build.SOURCES and "svmtrain_kernels.hip" in dsp_amd.build.SOURCES and "svmtrain_kernels.hpp" in dsp_amd.build.HEADERS
    for i, name in enumerate(("CONVERGED", "MAX_ITER", "ONE_CLASS", "EMPTY")):
        assert re.search(r"#define DSP_SVM_TRAIN_%s %d\b" % (name, i), header) and getattr(dl, "SVM_TRAIN_" + name) == i == getattr(R, name)
    assert re.search(r"#define DSP_SVM_TRAIN_MAX_ROWS 8192\b", header) and dl.SVM_TRAIN_MAX_ROWS == 8192
    assert C.sizeof(dl.SvmTrainResult) == 40 == np.dtype(dl.SVM_TRAIN_RESULT_DTYPE).itemsize and C.sizeof(dl.SvmTrainProblem) == 40
    assert C.sizeof(dl.SvmTrainConfig) == 16 and C.sizeof(dl.SvmFitModel) == 112
    assert hasattr(sj, "SvmTrainer") and hasattr(sj.ScrubJay, "train")
