"""GPU: labelled trials (dsp_trials_evaluate_device; dsp_amd.TrialEvaluator).

Every output is an integer count or one correctly rounded float64 operation on counts and on lo / hi, so everything is compared with
np.array_equal against tests/trials_ref.py (NaN where the contract says NaN), and stays the same bits whatever the other columns, the
outputs asked for, the stream and what the workspace held.  Every output buffer is filled with a sentinel and has spare entries
behind it, which are checked.  What the shared cases exercise -- ties, empty classes, scores on thresholds, NaN and infinities, every
constant of the kernels from both sides -- is checked on the reference alone, without a GPU, by tests/test_trials_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import trials_ref as R
from tests import trials_util as U

pytestmark = pytest.mark.gpu
IP = C.POINTER(C.c_int)
SPARE = 3
SENTINEL = -7
ALL = ("columns", "sweep_tp", "sweep_fp", "fa_above", "fa_equal")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def ev(torch_cuda):
    import dsp_amd
    e = dsp_amd.TrialEvaluator()
    yield e
    e.close()


def _raw(torch, ev, scores, truth, n, want=ALL, stream=None):
    """dsp_trials_evaluate_device into sentinel-filled buffers with SPARE entries behind each -> the outputs named in `want` as numpy, the
    spare (and every buffer not asked for) checked"""
    import dsp_amd
    x = scores if isinstance(scores, torch.Tensor) else torch.tensor(np.ascontiguousarray(scores, np.float32), device="cuda")
    truth = np.ascontiguousarray(truth, np.intc)
    T, S = truth.size, (x.shape[1] if x.dim() == 2 else 1)
    n_tgt = int((truth >= 0).sum())
    size = {"columns": (S + 1) * 10, "sweep_tp": (S + 1) * n, "sweep_fp": (S + 1) * n, "fa_above": n_tgt, "fa_equal": n_tgt}
    bufs = {key: torch.full((size[key] + SPARE,), SENTINEL, dtype=torch.int32 if key.startswith("fa_") else torch.int64, device="cuda") for key in ALL}
    cfg = dsp_amd.lib.TrialsConfig(n)
    torch.cuda.synchronize()
    rc = ev._L.dsp_trials_evaluate_device(ev._h, x.data_ptr(), T, S, truth.ctypes.data_as(IP), C.byref(cfg),
                                          *[bufs[key].data_ptr() if key in want else None for key in ALL],
                                          C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, dsp_amd.lib.last_error()
    torch.cuda.synchronize()
    out = {}
    for key in ALL:
        a = bufs[key].cpu().numpy()
        assert (a[size[key]:] == SENTINEL).all(), f"{key}: wrote behind the output"
        if key not in want:
            assert (a == SENTINEL).all(), f"{key}: written though not asked for"
        elif key == "columns":
            out[key] = a[:size[key]].copy().view(R.DTYPE).reshape(-1)
        else:
            out[key] = a[:size[key]].reshape((S + 1, n)) if key.startswith("sweep") else a[:size[key]]
    return out


def _check(got, ref, keys=ALL):
    for key in keys:
        if key == "columns":
            for name in R.DTYPE.names:
                assert R.same(got[key][name], ref[key][name]), (name, got[key][name], ref[key][name])
        else:
            assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), key


def _bits(got, keys=ALL):
    return {key: np.ascontiguousarray(got[key]).view(np.uint8).copy() for key in keys}


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_parity_with_the_reference(torch_cuda, ev, case):
    x, truth = U.case_inputs(*case)
    _check(_raw(torch_cuda, ev, x, truth, case[2]), U.case_ref(*case))


def test_recorded_trials_of_the_reference(torch_cuda, ev, golden):
    g = golden("gmm_trials_ref.npz")
    x, truth = g["llr"].astype(np.float32), np.where(g["label"] == 1, 0, -1)
    got = _raw(torch_cuda, ev, x, truth, 200)
    _check(got, R.evaluate(x, truth, 200))
    c = got["columns"][0]
    assert c["best_threshold"] == g["best_t"] and c["best_index"] == g["best_index"] and c["best_correct"] == g["best_correct"] == 85
    assert abs(c["auc"] - g["auc"]) <= 1e-12
    fps = np.rint(g["fpr_all"] * 56).astype(np.int64)
    xt = x[truth == 0]
    at = np.searchsorted(-g["roc_thresholds_all"][1:], -xt.astype(np.float64)) + 1
    assert np.array_equal(fps[at], got["fa_above"].astype(np.int64) + got["fa_equal"])


@pytest.mark.parametrize("n", U.N_LIST)
def test_a_column_does_not_see_the_others(torch_cuda, ev, n):
    T, S = 2 * U.PAIR_ROWS_TIME + 1, 130
    x, truth = U.case_inputs(T, S, n, "normal" if n == 200 else "eighths", "mixed", 7)
    big = _raw(torch_cuda, ev, x, truth, n)
    off = R.target_lists(truth, S)[0]
    for s in (0, 1, 2, 4, 63, 64, 129):
        alone = _raw(torch_cuda, ev, np.ascontiguousarray(x[:, s:s + 1]), np.where(truth == s, 0, -1), n)
        for name in R.DTYPE.names:
            assert R.same(alone["columns"][name][0], big["columns"][name][s]), (s, name)
        assert np.array_equal(alone["columns"][:1].view(np.uint8), big["columns"][s:s + 1].view(np.uint8)), s     # the same bits
        assert np.array_equal(alone["sweep_tp"][0], big["sweep_tp"][s]) and np.array_equal(alone["sweep_fp"][0], big["sweep_fp"][s])
        assert np.array_equal(alone["fa_above"], big["fa_above"][off[s]:off[s + 1]]) and np.array_equal(alone["fa_equal"], big["fa_equal"][off[s]:off[s + 1]])


@pytest.mark.parametrize("case", [(U.PAIR_ROWS_TIME + 1, 2, 200, "eighths", "tile"), (2 * U.PAIR_ROWS_TIME + 1, 65, 200, "normal", "tile"),
                                  (65, 5, 1024, "grid", "mixed")], ids=U.case_id)
def test_every_subset_of_the_outputs_equals_the_full_call(torch_cuda, ev, case):
    x, truth = U.case_inputs(*case)
    full = _bits(_raw(torch_cuda, ev, x, truth, case[2]))
    subsets = [("columns",), ("sweep_tp",), ("sweep_fp",), ("sweep_tp", "sweep_fp"), ("fa_above",), ("fa_equal",), ("fa_above", "fa_equal"),
               ("columns", "fa_above", "fa_equal"), ("columns", "sweep_tp", "sweep_fp"), ("sweep_fp", "fa_above")]
    for want in subsets:
        part = _bits(_raw(torch_cuda, ev, x, truth, case[2], want=want), want)
        for key in want:
            assert np.array_equal(part[key], full[key]), (want, key)


def test_a_small_call_after_a_large_one_and_another_stream(torch_cuda, ev):
    import dsp_amd
    large, small = (2 * U.PAIR_ROWS_TIME + 1, 130, 1024, "eighths", "mixed"), (63, 2, 2, "eighths", "mixed")
    _raw(torch_cuda, ev, *U.case_inputs(*large, 3), large[2])
    _check(_raw(torch_cuda, ev, *U.case_inputs(*small), small[2]), U.case_ref(*small))
    fresh = dsp_amd.TrialEvaluator()
    stream = torch_cuda.cuda.Stream()
    for case in (small, (U.PAIR_ROWS_TIME + 1, 33, 200, "normal", "mixed")):
        x = torch_cuda.tensor(np.ascontiguousarray(U.case_inputs(*case)[0]), device="cuda")
        torch_cuda.cuda.synchronize()
        _check(_raw(torch_cuda, fresh, x, U.case_inputs(*case)[1], case[2], stream=stream), U.case_ref(*case))
    fresh.close()


def test_the_python_layer(torch_cuda, ev):
    import dsp_amd
    case = (65, 33, 200, "eighths", "mixed")
    x, truth = U.case_inputs(*case)
    ref = U.case_ref(*case)
    xd = torch_cuda.tensor(np.ascontiguousarray(x), device="cuda")
    got = ev.evaluate(xd, truth)
    assert got["n_thresholds"] == 200 and got["columns"].dtype == np.dtype(dsp_amd.lib.TRIAL_COLUMN_DTYPE)
    _check(got, ref)
    assert np.array_equal(got["target_offsets"], ref["target_offsets"]) and np.array_equal(got["target_rows"], ref["target_rows"])
    assert np.array_equal(got["target_scores"], x[ref["target_rows"], truth[ref["target_rows"]]], equal_nan=True)
    only = ev.evaluate(xd, truth, n_thresholds=2, want=("sweep",))
    assert sorted(only) == ["n_thresholds", "sweep_fp", "sweep_tp"] and only["sweep_tp"].shape == (34, 2)
    one = ev.evaluate(xd[:, 0].contiguous(), np.where(truth == 0, 0, -1), want=("columns", "roc"))      # [T]: one column
    assert R.same_columns(one["columns"][:1], ref["columns"][:1])
    f, t, h = dsp_amd.roc_points(one, 0)
    assert f[0] == 0 and t[0] == 0 and f[-1] == 1 and t[-1] == 1 and (np.diff(f) >= 0).all() and (np.diff(t) >= 0).all()
    area = float(((f[1:] - f[:-1]) * (t[1:] + t[:-1])).sum() / 2)
    assert abs(area - one["columns"]["auc"][0]) <= 1e-12
    for bad in (dict(truth=truth[:-1]), dict(truth=np.where(truth == 0, 33, truth)), dict(n_thresholds=1), dict(want=()), dict(want=("auc",))):
        with pytest.raises(ValueError):
            ev.evaluate(xd, **dict(dict(truth=truth), **bad))
    with pytest.raises(ValueError):
        ev.evaluate(xd.cpu(), truth)
    with pytest.raises(ValueError):
        ev.evaluate(xd.double(), truth)


def test_verified_scores_go_straight_to_the_evaluator(torch_cuda, ev, golden):
    import dsp_amd
    from tests.verify_util import fixture_case
    case = fixture_case(golden)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    feats = torch_cuda.tensor(np.ascontiguousarray(case["feats"], np.float32), device="cuda")
    means = torch_cuda.tensor(np.ascontiguousarray(case["means"], np.float32), device="cuda")
    llr = ver.verify(feats, case["fo"], means, want=("llr",))["llr"]
    truth = np.arange(12)                                    # clip i is speaker i's
    got = ev.evaluate(llr, truth)
    _check(got, R.evaluate(llr.cpu().numpy(), truth, 200))
    assert got["columns"]["n_target"].tolist() == [1] * 12 + [12] and got["columns"]["n_nontarget"].tolist() == [11] * 12 + [132]
    ver.close()
