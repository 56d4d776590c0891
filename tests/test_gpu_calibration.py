"""GPU: score calibration (dsp_calibration_fit_device, dsp_calibration_apply_device; dsp_amd.ScoreCalibrator) against
tests/calibration_ref.py.

apply is float64 arithmetic of fixed order rounded once: np.array_equal.  A fit's sums run in another order than numpy's, so the fit is
held to what does not depend on the order: the counts and the status are the reference's; at the GPU's own parameters the float64
reference's Newton step max |H^-1 g| is tol = 1e-8 at most; objective and objective_start are within 1e-12 relative of the reference's J
at the same parameters (positive terms: the sum inherits the few-ulp error of the device's exp and log1p; 1e-12 leaves three orders over
that and sits five below a float32 accumulator's 6e-8); the recorded trials meet sklearn's answer within 1e-6.  A report is the same
bits on a second call, after another call dirtied or grew the workspace, and on another stream.

n_iter and n_rejected: the shared cases are decisive (tests/calibration_util.py says what that means and why; tests/test_calibration_cpu.py
checks it on the reference), so the number of accepted passes, n_iter - n_rejected, is the reference's and n_rejected is at least the
reference's decisive rejections.  Behind the first Newton step of tol or less, whether a pass is accepted is decided by the rounding of
J in its last bit: the number of rejected passes there may differ from numpy's, and both counts are printed beside the reference's.

Every output buffer is filled with a sentinel and has spare entries behind it, which are checked.  The tree's depth at the shapes used
-- two nodes or more at every level in both layouts -- is checked without a GPU by tests/test_calibration_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import calibration_ref as R
from tests import calibration_util as U
from tests import trials_ref

pytestmark = pytest.mark.gpu
IP, LP = C.POINTER(C.c_int), C.POINTER(C.c_long)
SPARE = 3
SENTINEL = -7.0
FIT_CASES = [(T, S, wf) for T, S in U.SHAPES for wf in (False, True)]
PARAMS = (1.2345678901234567, -0.3, 0.7)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cal(torch_cuda):
    import dsp_amd
    c = dsp_amd.ScoreCalibrator()
    yield c
    c.close()


def _device(torch, x):
    return x if isinstance(x, torch.Tensor) else torch.tensor(np.ascontiguousarray(x, np.float32), device="cuda")


def _fit(torch, cal, scores, truth, n_frames=None, tol=U.TOL, max_iter=100, prior=0.5, init=None, stream=None):
    """dsp_calibration_fit_device into a report filled with 0xA5 -> (the report as the reference's dict, its 88 bytes)"""
    import dsp_amd
    dl = dsp_amd.lib
    x = _device(torch, scores)
    truth = np.ascontiguousarray(truth, np.intc)
    T, S = truth.size, (x.shape[1] if x.dim() == 2 else 1)
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int64)
    cfg, rep = dl.CalibrationConfig(prior, tol, max_iter, 0), dl.CalibrationReport()
    C.memset(C.byref(rep), 0xA5, C.sizeof(rep))
    start = dl.Calibration(*init) if init is not None else None
    torch.cuda.synchronize()
    rc = cal._L.dsp_calibration_fit_device(cal._h, x.data_ptr(), T, S, truth.ctypes.data_as(IP), nf.ctypes.data_as(LP) if nf is not None else None,
                                           C.byref(cfg), C.byref(start) if start is not None else None, C.byref(rep),
                                           C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, dl.last_error()
    out = {k: getattr(rep, k) for k in R.REPORT_KEYS if k not in ("a", "b", "c")}
    out.update(a=rep.params.a, b=rep.params.b, c=rep.params.c)
    assert rep.reserved == 0
    return out, np.frombuffer(bytes(rep), np.uint8).copy()


def _apply(torch, cal, scores, params, n_frames=None, in_place=False):
    """dsp_calibration_apply_device into a sentinel-filled buffer with SPARE entries behind it (in place: the scores lie in that buffer)
    -> float32 of the scores' shape, the spare checked"""
    import dsp_amd
    dl = dsp_amd.lib
    x = np.ascontiguousarray(scores, np.float32)
    T, S = x.shape[0], (x.shape[1] if x.ndim == 2 else 1)
    buf = torch.full((x.size + SPARE,), SENTINEL, dtype=torch.float32, device="cuda")
    if in_place:
        buf[:x.size] = torch.tensor(x.reshape(-1), device="cuda")
        src = buf
    else:
        src = torch.tensor(x.reshape(-1), device="cuda")
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int64)
    p = dl.Calibration(*params)
    torch.cuda.synchronize()
    rc = cal._L.dsp_calibration_apply_device(cal._h, src.data_ptr(), T, S, nf.ctypes.data_as(LP) if nf is not None else None, C.byref(p), buf.data_ptr(),
                                             None)
    assert rc == 0, dl.last_error()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[x.size:] == SENTINEL).all(), "wrote behind the output"
    if not in_place:
        assert np.array_equal(src.cpu().numpy().view(np.uint32), x.reshape(-1).view(np.uint32)), "the input was written"
    return out[:x.size].reshape(x.shape)


def _same_floats(got, ref):
    """the same float32 values bit for bit (the sign of a zero included), NaN where the reference has NaN"""
    nan = np.isnan(ref)
    return got.dtype == ref.dtype == np.float32 and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))


def _theta(rep):
    return np.array([rep["a"], rep["b"], rep["c"]])


def _check_fit(got, x, truth, dur, init=(1.0, 0.0, 0.0), prior=0.5, tol=U.TOL):
    """what holds whatever the order of the sums: optimality at the GPU's parameters and the two objectives"""
    assert R.newton_step(x, truth, dur, _theta(got), prior) <= tol
    for key, theta in (("objective", _theta(got)), ("objective_start", init)):
        ref = R.objective(x, truth, dur, theta, prior)
        print(key, got[key], ref, abs(got[key] - ref) / abs(ref))
        assert abs(got[key] - ref) <= 1e-12 * abs(ref), key
    assert got["objective"] <= got["objective_start"] and got["last_step"] <= tol


@pytest.mark.parametrize("T,S,with_frames", FIT_CASES, ids=lambda v: str(v))
def test_fit_against_the_reference(torch_cuda, cal, T, S, with_frames):
    x, truth, n_frames = U.case_inputs(T, S)
    ref, trace = U.case_ref(T, S, with_frames)
    got, _ = _fit(torch_cuda, cal, x, truth, n_frames if with_frames else None)
    print({k: (got[k], ref[k]) for k in R.REPORT_KEYS})
    for key in ("status", "n_target", "n_nontarget", "n_excluded"):
        assert got[key] == ref[key], key
    assert got["status"] == R.CONVERGED and (got["c"] == 0.0) == (not with_frames)
    _check_fit(got, x, truth, U.duration(n_frames) if with_frames else None)
    assert got["n_iter"] - got["n_rejected"] == ref["n_iter"] - ref["n_rejected"]
    assert U.decisive_rejections(trace) <= got["n_rejected"] <= U.decisive_rejections(trace) + R.MAX_HALVINGS
    assert np.abs(_theta(got) - _theta(ref)).max() <= 2 * U.TOL


def test_the_smallest_matrix_has_no_second_class(torch_cuda, cal):
    for truth, n_frames in (([0], None), ([-1], [7])):
        got, _ = _fit(torch_cuda, cal, np.array([[0.5]], np.float32), truth, n_frames, init=(2.0, 1.0, 0.0))
        ref = R.fit(np.array([[0.5]], np.float32), truth, None if n_frames is None else U.duration(n_frames), init=(2.0, 1.0, 0.0))
        assert got["status"] == R.NO_CLASS == ref["status"] and _theta(got).tolist() == [2.0, 1.0, 0.0]
        assert np.isnan([got["objective"], got["objective_start"], got["last_step"]]).all()
        for key in ("n_target", "n_nontarget", "n_excluded", "n_iter", "n_rejected"):
            assert got[key] == ref[key], key
    got, _ = _fit(torch_cuda, cal, np.array([[np.nan], [1.0], [2.0]], np.float32), [0, -1, -1])      # the only target is excluded
    assert (got["status"], got["n_target"], got["n_nontarget"], got["n_excluded"], got["n_iter"]) == (R.NO_CLASS, 0, 2, 1, 1)


def test_recorded_trials_meet_sklearn(torch_cuda, cal, golden):
    x, truth, n_frames, g = U.recorded(golden)
    for nf, key in ((n_frames, "theta3"), (None, "theta2")):
        dur = None if nf is None else U.duration(nf)
        got, _ = _fit(torch_cuda, cal, x, truth, nf)
        ref = R.fit(x, truth, dur, tol=U.TOL)
        print(key, _theta(got).tolist(), g[key].tolist(), {k: (got[k], ref[k]) for k in ("n_iter", "n_rejected")})
        assert got["status"] == R.CONVERGED and (got["n_target"], got["n_nontarget"], got["n_excluded"]) == (36, 56, 0)
        assert np.abs(_theta(got) - g[key]).max() <= 1e-6
        _check_fit(got, x, truth, dur)
        assert got["n_iter"] - got["n_rejected"] == ref["n_iter"] - ref["n_rejected"]


def test_a_miscalibrated_start_is_damped_to_the_same_optimum(torch_cuda, cal, golden):
    x, truth, n_frames, _ = U.recorded(golden)
    far = (x * np.float32(50.0) + np.float32(20.0)).astype(np.float32)
    for nf in (None, n_frames):
        dur = None if nf is None else U.duration(nf)
        got, _ = _fit(torch_cuda, cal, far, truth, nf)
        plain, _ = _fit(torch_cuda, cal, x, truth, nf)
        trace = []
        ref = R.fit(far, truth, dur, tol=U.TOL, trace=trace)
        print({k: (got[k], ref[k]) for k in R.REPORT_KEYS})
        assert got["status"] == R.CONVERGED == ref["status"] and got["n_rejected"] > 0
        _check_fit(got, far, truth, dur)
        assert got["n_iter"] - got["n_rejected"] == ref["n_iter"] - ref["n_rejected"] and got["n_rejected"] >= U.decisive_rejections(trace) >= 10
        # the same optimum as from the scores themselves: far = 50 x + 20 rounded to float32 moves x by 1.5e-7 at most and J by less than 1e-6
        assert abs(got["objective"] - plain["objective"]) <= 1e-6
        assert abs(got["a"] * 50.0 - plain["a"]) <= 1e-3 and abs(got["b"] + 20.0 * got["a"] - plain["b"]) <= 1e-3


def test_separable_scores_end_finite(torch_cuda, cal):
    x, truth = U.separable()
    for nf in (None, np.arange(50, 50 + truth.size) * 7):
        got, _ = _fit(torch_cuda, cal, x, truth, nf, max_iter=300)
        print(got)
        assert got["status"] in (R.SINGULAR, R.MAX_ITER) and np.isfinite(_theta(got)).all() and got["objective"] <= got["objective_start"]
        assert (got["n_target"], got["n_nontarget"], got["n_excluded"]) == (31, 61, 0)


def test_a_step_that_never_helps_stalls_and_a_zero_pivot_is_singular(torch_cuda, cal):
    x, truth, init = U.saturated()
    got, _ = _fit(torch_cuda, cal, x, truth, None, init=init)
    ref = R.fit(x, truth, None, tol=U.TOL, init=init)
    assert got["status"] == R.STALLED == ref["status"] and _theta(got).tolist() == list(init) and np.isnan(got["last_step"])
    assert (got["n_iter"], got["n_rejected"]) == (ref["n_iter"], ref["n_rejected"]) == (R.MAX_HALVINGS + 2, R.MAX_HALVINGS + 1)
    assert got["objective"] == got["objective_start"] and abs(got["objective"] - ref["objective"]) <= 1e-12 * ref["objective"]
    flat, _ = _fit(torch_cuda, cal, np.zeros((50, 1), np.float32), truth[:50])
    assert (flat["status"], flat["n_iter"], _theta(flat).tolist()) == (R.SINGULAR, 1, [1.0, 0.0, 0.0]) and abs(flat["objective"] - np.log(2.0)) <= 1e-15
    huge, _ = _fit(torch_cuda, cal, x, truth, None, init=(1e308, 0.0, 0.0))
    assert huge["status"] == R.SINGULAR and huge["a"] == 1e308 and np.isinf(huge["objective"])
    one, _ = _fit(torch_cuda, cal, x, truth, None, max_iter=1)
    assert one["status"] == R.MAX_ITER and _theta(one).tolist() == [1.0, 0.0, 0.0] and one["objective"] == one["objective_start"] and one["n_iter"] == 1


def test_a_report_is_the_same_bits_whatever_came_before(torch_cuda, cal):
    import dsp_amd
    for T, S, with_frames in ((257, 3, True), (5000, 70, False), (65, 32, True)):
        x, truth, n_frames = U.case_inputs(T, S)
        nf = n_frames if with_frames else None
        xd = _device(torch_cuda, x)
        first = _fit(torch_cuda, cal, xd, truth, nf)[1]
        assert np.array_equal(_fit(torch_cuda, cal, xd, truth, nf)[1], first), "a second call"
        other = U.case_inputs(T, S, 99)
        _fit(torch_cuda, cal, other[0], other[1], other[2])                                  # the same shape: every partial is dirtied
        assert np.array_equal(_fit(torch_cuda, cal, xd, truth, nf)[1], first), "a dirtied workspace"
        big = U.case_inputs(300000, 1)
        _fit(torch_cuda, cal, big[0], big[1], big[2], max_iter=2)                            # grows the workspace
        assert np.array_equal(_fit(torch_cuda, cal, xd, truth, nf)[1], first), "a grown workspace"
        stream = torch_cuda.cuda.Stream()
        fresh = dsp_amd.ScoreCalibrator()
        assert np.array_equal(_fit(torch_cuda, fresh, xd, truth, nf, stream=stream)[1], first), "another stream, another calibrator"
        fresh.close()


def test_a_fit_continues_from_where_max_iter_ended_it(torch_cuda, cal, golden):
    x, truth, n_frames, _ = U.recorded(golden)
    for nf in (None, n_frames):
        dur = None if nf is None else U.duration(nf)
        part, _ = _fit(torch_cuda, cal, x, truth, nf, max_iter=3)
        assert part["status"] == R.MAX_ITER and part["n_iter"] == 3 and part["objective"] < part["objective_start"]
        ref = R.objective(x, truth, dur, _theta(part))
        assert abs(part["objective"] - ref) <= 1e-12 * ref
        rest, _ = _fit(torch_cuda, cal, x, truth, nf, init=tuple(_theta(part)))
        whole, _ = _fit(torch_cuda, cal, x, truth, nf)
        assert rest["status"] == whole["status"] == R.CONVERGED and rest["objective_start"] == part["objective"]
        _check_fit(rest, x, truth, dur, init=_theta(part))
        _check_fit(whole, x, truth, dur)


@pytest.mark.parametrize("T,S", U.SHAPES + ((92, 1), (1, 1)), ids=lambda v: str(v))
def test_apply_is_the_reference_bit_for_bit(torch_cuda, cal, T, S):
    x, _, n_frames = U.case_inputs(T, S)
    x = x.copy()
    x.reshape(-1)[0] = -0.0
    if x.size > 4:
        x.reshape(-1)[1] = 0.0
        x.reshape(-1)[-3:] = (np.nan, np.inf, -np.inf)
    dur = U.duration(n_frames)
    for params, nf in ((PARAMS, n_frames), ((PARAMS[0], PARAMS[1], 0.0), n_frames), ((PARAMS[0], PARAMS[1], 0.0), None), ((1.0, 0.0, 0.0), None),
                       ((-2.5, -0.0, 0.0), None), ((0.0, 1.0, -1.0), n_frames)):
        ref = R.apply(x, params, None if nf is None else dur)
        for in_place in (False, True):
            assert _same_floats(_apply(torch_cuda, cal, x, params, nf, in_place), ref), (params, nf is None, in_place)
    if S == 1:                                               # [T]: one column
        assert _same_floats(_apply(torch_cuda, cal, x[:, 0].copy(), PARAMS, n_frames), R.apply(x[:, 0], PARAMS, dur))


def test_calibrated_scores_go_straight_to_the_evaluator(torch_cuda, cal, golden):
    import dsp_amd
    x, truth, n_frames, _ = U.recorded(golden)
    xd = _device(torch_cuda, x)
    rep = cal.fit(xd, truth, n_frames, tol=U.TOL)
    assert rep["status"] == dsp_amd.lib.CAL_CONVERGED and rep["status_name"] == "converged"
    out = cal.apply(xd, rep, n_frames)
    ref = R.apply(x, rep["params"], U.duration(n_frames))
    assert _same_floats(out.cpu().numpy(), ref)
    ev = dsp_amd.TrialEvaluator()
    got = ev.evaluate(out, truth, want=("columns",))["columns"]
    want = trials_ref.evaluate(ref, truth, 200)["columns"]
    assert got["best_correct"][1] == want["best_correct"][1] and got["best_correct"][0] == want["best_correct"][0]
    ev.close()


def test_the_python_layer(torch_cuda, cal):
    import dsp_amd
    T, S = 130, 70
    x, truth, n_frames = U.case_inputs(T, S)
    xd = _device(torch_cuda, x)
    rep = cal.fit(xd, truth, n_frames, tol=U.TOL)
    raw, _ = _fit(torch_cuda, cal, xd, truth, n_frames)
    assert {k: rep[k] for k in R.REPORT_KEYS} == raw and rep["params"] == (rep["a"], rep["b"], rep["c"]) and rep["status_name"] == "converged"
    two = cal.fit(xd, truth, tol=U.TOL, prior=0.7)                 # (decisive at this prior: steps 5.5e-06, 1.8e-11)
    assert two["c"] == 0.0 and two["status"] == 0 and R.newton_step(x, truth, None, _theta(two), prior=0.7) <= U.TOL
    ref = R.apply(x, rep["params"], U.duration(n_frames))
    assert _same_floats(cal.apply(xd, rep, n_frames).cpu().numpy(), ref) and _same_floats(cal.apply(xd, rep["params"], n_frames).cpu().numpy(), ref)
    out = torch_cuda.full_like(xd, SENTINEL)
    assert cal.apply(xd, (2.0, 1.0, 0.0), out=out) is out and _same_floats(out.cpu().numpy(), R.apply(x, (2.0, 1.0, 0.0)))
    mine = xd.clone()
    assert cal.apply(mine, rep, n_frames, out=mine) is mine and _same_floats(mine.cpu().numpy(), ref)
    assert _same_floats(cal.apply(xd[:, 0].contiguous(), (2.0, 1.0, 0.5), n_frames).cpu().numpy(), R.apply(x[:, 0], (2.0, 1.0, 0.5), U.duration(n_frames)))
    assert np.array_equal(dsp_amd.ScoreCalibrator.duration_term(n_frames), U.duration(n_frames))
    for bad in (dict(truth=truth[:-1]), dict(truth=np.where(truth == 0, S, truth)), dict(n_frames=n_frames[:-1]), dict(n_frames=-n_frames), dict(prior=1.0),
                dict(tol=0.0), dict(max_iter=0), dict(init=(1.0, 0.0, float("nan"))), dict(init=(1.0, 0.0, 1.0), n_frames=None)):
        with pytest.raises(ValueError):
            cal.fit(xd, **dict(dict(truth=truth, n_frames=n_frames), **bad))
    for bad in (dict(params=(1.0, 0.0, 1.0)), dict(params=(1.0, float("inf"), 0.0)), dict(params=(1.0, 0.0, 0.0), out=xd[:-1]),
                dict(params=(1.0, 0.0, 0.0), out=xd.double()), dict(params=(1.0, 0.0, 0.0), n_frames=n_frames[:-1])):
        with pytest.raises(ValueError):
            cal.apply(xd, **bad)
    with pytest.raises(ValueError):
        cal.fit(xd.cpu(), truth)
    with pytest.raises(ValueError):
        cal.apply(xd.double(), (1.0, 0.0, 0.0))
