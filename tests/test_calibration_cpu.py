"""No GPU: the restatement of score calibration (tests/calibration_ref.py) against its own edge cases -- the five end states, the
damping path, the exclusion of NaN and infinities, a prior other than 0.5 -- and against sklearn through the fixture
tests/golden/gmm_calibration_ref.npz; the host-only entry and every refusal of the built library, in the header's order; the symbols and
the struct sizes; and that the shared cases of tests/calibration_util.py hold what tests/test_gpu_calibration.py relies on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import calibration_ref as R
from tests import calibration_util as U

CAL_SYMBOLS = ["dsp_calibrator_create", "dsp_calibrator_destroy", "dsp_calibration_duration_term", "dsp_calibration_fit_device",
               "dsp_calibration_apply_device"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _theta(rep):
    return np.array([rep["a"], rep["b"], rep["c"]])


# ---- the reference against its own edge cases ----------------------------------------------------------------------------------------

def test_softplus_and_sigmoid_do_not_overflow():
    u = np.array([-800.0, -40.0, -1.0, 0.0, 1.0, 40.0, 800.0])
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        sp, sg = R.softplus(u), R.sigmoid(u)
    assert sp[0] == 0.0 and sp[-1] == 800.0 and sp[3] == np.log(2.0) and np.isfinite(sp).all()
    assert sg[0] == 0.0 and sg[-1] == 1.0 and sg[3] == 0.5 and np.allclose(sg + sg[::-1], 1.0, rtol=0, atol=1e-16)
    assert np.allclose(sp[1:-1], np.log1p(np.exp(u[1:-1])), rtol=1e-15, atol=0)


def test_objective_at_prior_half_is_cllr_and_the_derivatives_are_the_objective_s(golden):
    x, truth, n_frames, _ = U.recorded(golden)
    l = R.duration_term(n_frames)
    theta = np.array([3.0, -0.5, 0.1])
    xs, tgt = x[:, 0].astype(np.float64), truth == 0
    c = theta[0] * xs + theta[1] + theta[2] * l
    cllr = 0.5 * (np.log2(1.0 + np.exp(-c[tgt])).mean() + np.log2(1.0 + np.exp(c[~tgt])).mean())
    assert abs(R.objective(x, truth, l, theta) / np.log(2.0) - cllr) <= 1e-14
    for prior in (0.5, 0.2):
        kept = R._trials(x, truth, l)[:3]
        J, g, H = R.objective_parts(theta, *kept, prior, 3)
        h = 1e-5
        for i in range(3):
            e = np.zeros(3)
            e[i] = h
            Jp, gp, _ = R.objective_parts(theta + e, *kept, prior, 3)
            Jm, gm, _ = R.objective_parts(theta - e, *kept, prior, 3)
            assert abs((Jp - Jm) / (2 * h) - g[i]) <= 1e-7 * max(1.0, abs(g[i])), (prior, i)
            assert np.abs((gp - gm) / (2 * h) - H[i]).max() <= 1e-6 * max(1.0, np.abs(H).max()), (prior, i)
        assert np.array_equal(H, H.T)


def test_converged_on_the_recorded_trials_for_both_models(golden):
    x, truth, n_frames, _ = U.recorded(golden)
    l = U.duration(n_frames)
    for dur in (None, l):
        rep = R.fit(x, truth, dur, tol=U.TOL)
        assert rep["status"] == R.CONVERGED and (rep["n_target"], rep["n_nontarget"], rep["n_excluded"]) == (36, 56, 0)
        assert rep["n_rejected"] == 0 and 5 <= rep["n_iter"] <= 12 and rep["last_step"] <= U.TOL
        assert rep["objective"] < rep["objective_start"] and R.newton_step(x, truth, dur, _theta(rep)) <= U.TOL
        assert rep["objective"] == R.objective(x, truth, dur, _theta(rep))
        assert rep["objective_start"] == R.objective(x, truth, dur, (1.0, 0.0, 0.0))
        assert (rep["c"] == 0.0) == (dur is None)


def test_max_iter_returns_the_last_accepted_parameters_and_a_fit_can_be_continued(golden):
    x, truth, n_frames, _ = U.recorded(golden)
    l = U.duration(n_frames)
    one = R.fit(x, truth, l, tol=U.TOL, max_iter=1)
    assert one["status"] == R.MAX_ITER and _theta(one).tolist() == [1.0, 0.0, 0.0] and one["objective"] == one["objective_start"] and one["n_iter"] == 1
    part = R.fit(x, truth, l, tol=U.TOL, max_iter=3)
    assert part["status"] == R.MAX_ITER and part["n_iter"] == 3 and part["objective"] < part["objective_start"]
    assert part["objective"] == R.objective(x, truth, l, _theta(part))
    rest = R.fit(x, truth, l, tol=U.TOL, init=_theta(part))
    whole = R.fit(x, truth, l, tol=U.TOL)
    assert rest["status"] == whole["status"] == R.CONVERGED and rest["objective_start"] == part["objective"]
    assert R.newton_step(x, truth, l, _theta(rest)) <= U.TOL and np.abs(_theta(rest) - _theta(whole)).max() <= 2 * U.TOL


def test_the_damping_path_reaches_the_same_optimum(golden):
    x, truth, n_frames, _ = U.recorded(golden)
    l = U.duration(n_frames)
    far = (x * np.float32(50.0) + np.float32(20.0)).astype(np.float32)
    for dur in (None, l):
        plain, rep = R.fit(x, truth, dur, tol=U.TOL), R.fit(far, truth, dur, tol=U.TOL)
        assert rep["status"] == R.CONVERGED and rep["n_rejected"] > 0 and rep["n_iter"] > plain["n_iter"]
        assert R.newton_step(far, truth, dur, _theta(rep)) <= U.TOL
        # the same optimum: far = 50 x + 20 rounded to float32, half an ulp of 128 over 50 = 1.5e-7 in x, times A = 5.3 and a gradient
        # weight of 1 at most: the objective moves by less than 1e-6
        assert abs(rep["objective"] - plain["objective"]) <= 1e-6
        assert abs(rep["a"] * 50.0 - plain["a"]) <= 1e-3 and abs(rep["b"] + 20.0 * rep["a"] - plain["b"]) <= 1e-3


def test_stalled_singular_and_no_class():
    x, truth, init = U.saturated()
    rep = R.fit(x, truth, None, init=init)
    assert rep["status"] == R.STALLED and rep["n_rejected"] == R.MAX_HALVINGS + 1 and rep["n_iter"] == R.MAX_HALVINGS + 2
    assert _theta(rep).tolist() == list(init) and rep["objective"] == rep["objective_start"] and np.isnan(rep["last_step"])
    flat = R.fit(np.zeros(50, np.float32), truth[:50], None)                     # every score 0: the first pivot is 0
    assert flat["status"] == R.SINGULAR and flat["n_iter"] == 1 and _theta(flat).tolist() == [1.0, 0.0, 0.0] and flat["objective"] == np.log(2.0)
    huge = R.fit(x, truth, None, init=(1e308, 0.0, 0.0))                         # c overflows: a J that is not finite
    assert huge["status"] == R.SINGULAR and huge["a"] == 1e308 and np.isinf(huge["objective"])
    sx, st = U.separable()
    sep = R.fit(sx, st, None, tol=U.TOL, max_iter=300)
    assert sep["status"] in (R.SINGULAR, R.MAX_ITER) and np.isfinite(_theta(sep)).all() and sep["objective"] <= sep["objective_start"] and sep["a"] > 50
    for xs, tr in ((x, np.full(x.shape[0], -1)), (x, np.zeros(x.shape[0], int)), (np.array([np.nan, 1.0, 2.0], np.float32), [0, -1, -1])):
        rep = R.fit(xs, tr, None, init=(2.0, 1.0, 0.0))
        assert rep["status"] == R.NO_CLASS and _theta(rep).tolist() == [2.0, 1.0, 0.0] and np.isnan(rep["objective"]) and np.isnan(rep["objective_start"])
        assert rep["n_iter"] == 1 and rep["n_target"] * rep["n_nontarget"] == 0


def test_nan_and_infinite_scores_take_no_part():
    x, truth, n_frames = U.case_inputs(257, 1, 0)
    l = U.duration(n_frames)
    keep = np.isfinite(x[:, 0])
    assert 0 < (~keep).sum() < 20 and np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    rep, clean = R.fit(x, truth, l, tol=U.TOL), R.fit(x[keep], truth[keep], l[keep], tol=U.TOL)
    assert rep["n_excluded"] == (~keep).sum() and clean["n_excluded"] == 0 and rep["status"] == R.CONVERGED
    assert {k: v for k, v in rep.items() if k != "n_excluded"} == {k: v for k, v in clean.items() if k != "n_excluded"}
    wide, tw, _ = U.case_inputs(130, 70)
    rep = R.fit(wide, tw, None, tol=U.TOL)
    assert rep["n_excluded"] == (~np.isfinite(wide)).sum() and rep["n_target"] + rep["n_nontarget"] + rep["n_excluded"] == wide.size
    assert rep["n_target"] == (np.isfinite(wide) & (tw[:, None] == np.arange(70)[None, :])).sum()


def test_a_prior_other_than_one_half():
    x, truth, n_frames = U.case_inputs(257, 3)
    l = U.duration(n_frames)
    half, low = R.fit(x, truth, l, prior=0.5, tol=U.TOL), R.fit(x, truth, l, prior=0.1, tol=U.TOL)
    assert half["status"] == low["status"] == R.CONVERGED and R.newton_step(x, truth, l, _theta(low), prior=0.1) <= U.TOL
    assert R.newton_step(x, truth, l, _theta(low), prior=0.5) > 1e-3 and low["objective"] == R.objective(x, truth, l, _theta(low), prior=0.1)
    # the weights and tau move together: the same scores calibrate to nearly the same log-odds (exactly so for a well-specified model)
    assert np.abs(_theta(half) - _theta(low)).max() < 0.5 and not np.array_equal(_theta(half), _theta(low))


def test_apply_rounds_once_and_keeps_nan(golden):
    x = np.array([[np.nan, np.inf, -np.inf], [-0.0, 0.0, 1.5], [3.0e38, -3.0e38, 1e-45]], np.float32)
    l = np.array([0.5, 2.0, 8.0])
    out = R.apply(x, (2.0, 0.25, -0.5), l)
    assert out.dtype == np.float32 and np.isnan(out[0, 0]) and out[0, 1] == np.inf and out[0, 2] == -np.inf
    assert out[1].tolist() == [-0.75, -0.75, 2.25] and out[2, 0] == np.inf and out[2, 1] == -np.inf and out[2, 2] == np.float32(0.25 - 4.0)
    two = R.apply(x, (1.0, 0.0, 0.0))
    assert np.array_equal(two, x, equal_nan=True) and not np.signbit(two[1, 0])       # -0 + 0 = +0
    assert np.signbit(R.apply(x, (1.0, -0.0, 0.0))[1, 0])
    a, b = np.float64(1.0 + 2.0 ** -30), np.float64(2.0 ** -40)                       # the product is rounded before the sum
    v = np.float32(1.0 + 2.0 ** -23)
    assert R.apply(np.array([v]), (a, b, 0.0))[0] == np.float32(a * np.float64(v) + b)
    assert R.apply(np.array([1.0, 2.0], np.float32), (1.0, 0.0, 1.0), np.array([1.0, 2.0])).tolist() == [2.0, 4.0]


# ---- the reference against sklearn, through the fixture -------------------------------------------------------------------------------

def test_restatement_against_sklearn(golden):
    x, truth, n_frames, g = U.recorded(golden)
    assert x.shape == (92, 1) and int((truth == 0).sum()) == 36 and n_frames.min() >= 50 and n_frames.max() <= 3000
    t = golden("gmm_trials_ref.npz")
    assert np.array_equal(g["llr"], t["llr"]) and np.array_equal(g["label"], t["label"])
    assert g["gap3"] < 1e-6 and g["gap2"] < 1e-6
    for dur, key in ((U.duration(n_frames), "theta3"), (None, "theta2")):
        rep = R.fit(x, truth, dur, tol=1e-12)
        gap = np.abs(_theta(rep) - g[key])
        print(key, _theta(rep).tolist(), g[key].tolist(), gap.max())
        assert rep["status"] == R.CONVERGED and gap.max() <= 1e-6, (key, gap)


# ---- the library's host code -----------------------------------------------------------------------------------------------------------

def test_duration_term_is_np_log_within_an_ulp():
    n = np.concatenate([np.arange(0, 5000), np.random.default_rng(3).integers(0, 1 << 40, 5000), [np.iinfo(np.int64).max]]).astype(np.int64)
    got = dsp_amd.ScoreCalibrator.duration_term(n)
    want = np.log(n.astype(np.float64) + 1e-8)
    assert got.dtype == np.float64 and got.shape == n.shape and np.isfinite(got).all()
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all() and got[0] == np.log(1e-8)
    assert np.abs(got - R.duration_term(n)).max() <= np.spacing(np.abs(want)).max()
    assert dsp_amd.ScoreCalibrator.duration_term([]).size == 0
    L = dsp_amd.load()
    out = (C.c_double * 2)()
    assert L.dsp_calibration_duration_term(None, 0, None) == 0
    assert L.dsp_calibration_duration_term((C.c_long * 2)(1, 2), -1, out) == -1 and "n_rows" in dl.last_error()
    assert L.dsp_calibration_duration_term(None, 2, out) == -1 and "NULL" in dl.last_error()
    assert L.dsp_calibration_duration_term((C.c_long * 2)(1, 2), 2, None) == -1 and "NULL" in dl.last_error()
    assert L.dsp_calibration_duration_term((C.c_long * 2)(1, -2), 2, out) == -1 and "n_frames[1] = -2" in dl.last_error()
    with pytest.raises(ValueError):
        dsp_amd.ScoreCalibrator.duration_term([3, -1])


def test_refusals_touch_no_device_and_come_in_the_header_s_order():
    L = dsp_amd.load()
    h = C.c_void_p()
    assert L.dsp_calibrator_create(0, C.byref(h)) == 0 and h.value
    L.dsp_calibrator_destroy(h)
    assert L.dsp_calibrator_create(-1, C.byref(h)) == -1 and "device" in dl.last_error()
    assert L.dsp_calibrator_create(0, None) == -1
    assert L.dsp_calibrator_create(0, C.byref(h)) == 0
    truth, frames = (C.c_int * 4)(0, -1, 1, 0), (C.c_long * 4)(10, 20, 30, 40)
    ptr = C.c_void_p(64)              # never dereferenced: every call below is refused before a device is touched
    rep = dl.CalibrationReport()

    def fit(handle=h, d_scores=ptr, T=4, S=2, tr=truth, nf=frames, prior=0.5, tol=1e-8, max_iter=10, cfg=True, init=None, report=True):
        c = dl.CalibrationConfig(prior, tol, max_iter, 0)
        start = dl.Calibration(*init) if init else None
        return L.dsp_calibration_fit_device(handle, d_scores, T, S, tr, nf, C.byref(c) if cfg else None, C.byref(start) if start else None,
                                            C.byref(rep) if report else None, None)

    def apply(handle=h, d_scores=ptr, T=4, S=2, nf=frames, params=(1.0, 0.0, 0.0), d_out=ptr):
        p = dl.Calibration(*params) if params else None
        return L.dsp_calibration_apply_device(handle, d_scores, T, S, nf, C.byref(p) if p else None, d_out, None)

    nan, inf = float("nan"), float("inf")
    fit_refused = [                                          # include/dsp_amd.h: "the first of"
        (dict(handle=C.c_void_p()), "calibrator is NULL"),
        (dict(cfg=False), "dsp_calibration_config is NULL"),
        (dict(prior=0.0), "prior"), (dict(prior=1.0), "prior"), (dict(prior=nan), "prior"),
        (dict(tol=0.0), "tol"), (dict(tol=nan), "tol"),
        (dict(max_iter=0), "max_iter must be 1 .. 10000, got 0"), (dict(max_iter=10001), "max_iter must be 1 .. 10000, got 10001"),
        (dict(report=False), "report is NULL"),
        (dict(S=0), "n_columns"), (dict(S=(1 << 19) + 1), "n_columns"),
        (dict(T=-1), "n_rows"), (dict(T=1 << 31), "2^31 rows"),
        (dict(init=(nan, 0.0, 0.0)), "init is not finite"), (dict(init=(1.0, inf, 0.0)), "init is not finite"),
        (dict(init=(1.0, 0.0, 0.5), nf=None), "init->c != 0 without n_frames"),
        (dict(d_scores=None), "d_scores is NULL"),
        (dict(tr=None), "truth is NULL"),
        (dict(tr=(C.c_int * 4)(0, -2, 1, 0)), "truth[1] = -2"), (dict(tr=(C.c_int * 4)(0, 1, 1, 2)), "truth[3] = 2"),
        (dict(nf=(C.c_long * 4)(1, 2, -3, -4)), "n_frames[2] = -3"),
    ]
    apply_refused = [
        (dict(handle=C.c_void_p()), "calibrator is NULL"),
        (dict(params=None), "params is NULL"), (dict(params=(1.0, nan, 0.0)), "params are not finite"),
        (dict(S=0), "n_columns"), (dict(T=-1), "n_rows"), (dict(T=1 << 31), "2^31 rows"),
        (dict(params=(1.0, 0.0, 0.5), nf=None), "params->c != 0 without n_frames"),
        (dict(d_scores=None), "d_scores is NULL"),
        (dict(d_out=None), "d_out is NULL"),
        (dict(nf=(C.c_long * 4)(1, -2, 3, 4)), "n_frames[1] = -2"),
    ]
    for call, refused in ((fit, fit_refused), (apply, apply_refused)):
        for kwargs, word in refused:
            assert call(**kwargs) == -1, kwargs
            assert word in dl.last_error(), (kwargs, dl.last_error())
        # the order: of two refusals the earlier one is reported, whichever pair is taken
        for i in range(len(refused) - 1):
            for j in range(i + 1, len(refused)):
                both = dict(refused[j][0], **refused[i][0])
                if set(refused[i][0]) & set(refused[j][0]):
                    continue
                assert call(**both) == -1 and refused[i][1] in dl.last_error(), (refused[i], refused[j], dl.last_error())
    # no trial: DSP_OK, no launch; the fit's report says so
    assert apply(T=0) == 0 and apply(T=0, d_scores=None, d_out=None, nf=None) == 0
    assert fit(T=0, d_scores=None, tr=None, nf=None, init=(2.0, 1.0, 0.0)) == 0
    assert (rep.status, rep.n_iter, rep.n_rejected, rep.n_target, rep.n_nontarget, rep.n_excluded) == (dl.CAL_NO_CLASS, 0, 0, 0, 0, 0)
    assert (rep.params.a, rep.params.b, rep.params.c) == (2.0, 1.0, 0.0) and np.isnan([rep.objective, rep.objective_start, rep.last_step]).all()
    assert fit(T=0, max_iter=0) == -1 and fit(T=0, init=(1.0, 0.0, 1.0), nf=None) == -1      # what comes before "no trial" is still refused
    L.dsp_calibrator_destroy(h)
    L.dsp_calibrator_destroy(None)


def test_symbols_are_declared_exported_and_listed():
    L = dsp_amd.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dsp_amd.build.LIB], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    for name in CAL_SYMBOLS:
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported and re.search(r"\b%s\(" % name, header), name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_calibrat")) == sorted(CAL_SYMBOLS)
    assert "ScoreCalibrator" in dsp_amd.__all__ and hasattr(dsp_amd, "ScoreCalibrator")
    assert "capi_calibrate.cpp" in dsp_amd.build.SOURCES and "calibrate_kernels.hip" in dsp_amd.build.SOURCES and "calibrate_kernels.hpp" in dsp_amd.build.HEADERS
    for i, name in enumerate(("CONVERGED", "MAX_ITER", "STALLED", "SINGULAR", "NO_CLASS")):
        assert re.search(r"#define DSP_CAL_%s %d\b" % (name, i), header) and getattr(dl, "CAL_" + name) == i == getattr(R, name)
    assert dl.CAL_STATUS == ("converged", "max_iter", "stalled", "singular", "no_class")


def test_ctypes_mirrors_match_the_header():
    assert C.sizeof(dl.Calibration) == 24 and C.sizeof(dl.CalibrationConfig) == 24 and C.sizeof(dl.CalibrationReport) == 88
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "capi_calibrate.cpp")) as f:
        src = f.read()
    assert "static_assert(sizeof(dsp_calibration_report) == 88" in src and "static_assert(sizeof(dsp_calibration_config) == 24" in src
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct dsp_calibration_report \{(.*?)\} dsp_calibration_report;", header, re.S).group(1)
    names = [n for line in body.split(";") for n in re.sub(r"/\*.*?\*/", "", line, flags=re.S).replace(",", " ").split()[1:]]
    assert names == [f[0] for f in dl.CalibrationReport._fields_]
    d = dl.Calibration()
    assert (d.a, d.b, d.c) == (0.0, 0.0, 0.0)               # (ctypes zero-fills; the library's default, init == NULL, is 1, 0, 0)


def test_constants_are_the_kernels_and_the_shapes_reach_every_level():
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "calibrate_kernels.hpp")) as f:
        src = f.read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        return eval(expr, {"kCalRowsColumns": U.ROWS_COLUMNS})                       # noqa: S307  (our own header: "4 * kCalRowsColumns")

    assert (const("kCalRowsTime"), const("kCalRowsColumns"), const("kCalBlockRowsColumns"), const("kCalFanIn")) == (U.ROWS_TIME, U.ROWS_COLUMNS,
                                                                                                                  U.BLOCK_ROWS_COLUMNS, U.FAN_IN)
    assert const("kCalMaxHalvings") == R.MAX_HALVINGS and "kTrialLanesAcrossColumns" in src
    assert U.tree(92, 1) == [1] and U.tree(63, 1) == [1] and U.tree(257, 3) == [3] and U.tree(65, 32) == [1] and U.tree(130, 70) == [2]
    # two nodes or more at every level, in both layouts, and a ragged last node at each
    assert U.tree(300000, 1) == [293, 19, 2] and U.tree(5000, 70) == [40, 3]
    for shape in U.DEEP:
        levels = U.tree(*shape)
        assert len(levels) >= 2 and min(levels) >= 2 and all(n % U.FAN_IN for n in levels[:-1])
    assert {S >= U.LANES_ACROSS_COLUMNS for _, S in U.DEEP} == {True, False}
    assert any(S >= U.LANES_ACROSS_COLUMNS and S % 64 for _, S in U.SHAPES) and any(T % U.BLOCK_ROWS_COLUMNS and S >= 32 for T, S in U.SHAPES)


def test_the_shared_cases_are_decisive(golden):
    """what tests/test_gpu_calibration.py relies on (tests/calibration_util.py says why): no full Newton step inside the noise zone"""
    for T, S in U.SHAPES:
        x, truth, n_frames = U.case_inputs(T, S)
        assert not x.flags.writeable and x.shape == (T, S) and truth.min() >= -1 and truth.max() < S
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        for with_frames in (False, True):
            rep, trace = U.case_ref(T, S, with_frames)
            assert rep["status"] == R.CONVERGED and rep["n_iter"] <= 25 and U.decisive(trace), (T, S, rep, U.full_steps(trace))
            assert rep["n_target"] >= 5 and rep["n_nontarget"] >= 5 and rep["n_excluded"] == (~np.isfinite(x)).sum() > 0
            assert U.decisive_rejections(trace) <= rep["n_rejected"] and len(trace) == rep["n_iter"]
            assert R.newton_step(x, truth, U.duration(n_frames) if with_frames else None, _theta(rep)) <= U.TOL
    # the recorded trials: plain, from the miscalibrated start, and continued after three passes
    x, truth, n_frames, _ = U.recorded(golden)
    far = (x * np.float32(50.0) + np.float32(20.0)).astype(np.float32)
    for dur in (None, U.duration(n_frames)):
        part = R.fit(x, truth, dur, tol=U.TOL, max_iter=3)
        for scores, init in ((x, None), (far, None), (x, _theta(part))):
            trace = []
            rep = R.fit(scores, truth, dur, tol=U.TOL, init=init, trace=trace)
            assert rep["status"] == R.CONVERGED and U.decisive(trace), U.full_steps(trace)
    assert U.decisive([("start", 1.0, np.nan, 0.0), ("accept", 0.9, 1.0, 1e-3), ("accept", 0.9, 0.9, 1e-9)])
    assert not U.decisive([("start", 1.0, np.nan, 0.0), ("accept", 0.9, 1.0, 1e-3), ("reject", 0.9, 0.9, 2e-8), ("accept", 0.9, 0.9, 1e-8)])
    assert U.decisive_rejections([("reject", 2.0, 1.0, 1.0), ("reject", 1.0 + 1e-15, 1.0, 1e-9), ("reject", np.nan, 1.0, 1.0)]) == 2
