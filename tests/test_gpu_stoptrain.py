"""GPU: stop-net training (dsp_stop_train_*, StopTrainer, StopModel.train) against the float64 restatement of
tests/stoptrain_ref.py on the three cases of stoptrain_ref.case():

  A  3 x 7, units 4-2-2-1, 23 clips of 2 .. 9 frames, batch 4, 6 epochs: truncation and padding, F_used 21 far below the block, 17
     training rows give a short last batch
  B  13 x 50, units 16-16-16-1, 70 clips of 50 frames, batch 32, 5 epochs: every unit slot, F_used 650 no multiple of the block
  C  13 x 500, units 4-2-2-1, 40 clips of 98 frames, batch 32, 12 epochs, patience 3: F_used 1274 of 6500, early stopping triggers

each with dropout on and off, at batch 1 and at batch >= n_train.  The parity allowance is imported, not a constant: four times the
restatement's own spread between the layer-1 feature sum taken ascending and descending over these runs, floored at 1e-9 relative
(stoptrain_ref.case_reference, asserted on the CPU by tests/test_stoptrain_cpu.py test_restatement_spread; measured spreads 6e-16 ..
7e-15, so the floor holds).  Relative means: of the array's largest magnitude (stoptrain_ref.relative).  Nothing here is derived from
what the GPU returns.  The other kernel forms, unequal layers and more than 256 rows: tests/test_gpu_stoptrain_shapes.py, through the
same helpers (tests/stoptrain_util.py)."""
import ctypes as C
import re

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl

from tests import stoptrain_ref as R
from tests import stoptrain_util as U
from tests.stoptrain_util import INT_FIELDS

pytestmark = pytest.mark.gpu
CASES = R.CASES_OLD
_cuda, _bytes = U.cuda, U.result_bytes


@pytest.fixture(scope="module")
def cases():
    """per case: the restatement's answers (computed once, left unchanged) and the device's, from ONE launch of all of its runs"""
    yield from U.trained_cases(CASES)


@pytest.mark.parametrize("name", CASES)
def test_scaler_and_rows(cases, name):
    """the fitted Scaler equals the restatement's float64 results rounded to float32 bit for bit (the restatement takes the kernel's
    summation tree), in the layout dsp_stop_model_params reads; Z equals the inference expression bit for bit"""
    c = cases[name]
    z = U.check_scaler_and_rows(c)
    if name == "A":
        assert z.shape[1] == 21 and (np.diff(c["frame_offsets"]) > 7).any() and (np.diff(c["frame_offsets"]) < 7).any()


@pytest.mark.parametrize("name", CASES)
def test_trajectories(cases, name):
    """history, params and prob within the imported allowance, the integer results exactly -- after asserting that the restatement's
    deciding comparisons have their margin"""
    c = cases[name]
    assert len(c["runs"]) == 4 and c["runs"][1]["dropout"] == (0.0, 0.0, 0.0) and c["runs"][2]["batch_size"] == 1
    assert c["runs"][3]["batch_size"] >= c["train_rows"].size and max(c["runs"][0]["dropout"] if "dropout" in c["runs"][0] else R.HYPER["dropout"]) > 0
    U.check_trajectories(c)
    if name == "C":
        assert any(r["status"] == dl.STOP_TRAIN_CONVERGED_EARLY and r["n_epochs"] < 12 for r in c["res"])


def test_bit_identity(cases):
    """one run alone, among 40 others, in the reversed launch, after a larger dataset has grown the workspace, and launched twice: equal
    bytes of history, params, prob and result"""
    c = cases["A"]
    t = c["trainer"]
    run = c["runs"][0]
    alone = _bytes(*t.train([run], c["labels"]), 0)
    others = [dict(run, seed=1000 + k, batch_size=1 + k % 7, epochs=1 + k % 6) for k in range(40)]
    mixed = others[:20] + [run] + others[20:]
    assert _bytes(*t.train(mixed, c["labels"]), 20) == alone
    assert _bytes(*t.train(mixed[::-1], c["labels"]), 20) == alone
    rng = np.random.default_rng(0)
    t.set(_cuda(rng.standard_normal((9 * 300, 3)).astype(np.float32)), np.arange(301) * 9)        # 300 clips, 64 runs: Z, the slabs and the tables grow
    big = t.train([dict(train_rows=np.arange(300), val_rows=None, seed=s, epochs=1) for s in range(64)], np.arange(300) % 2)[0]
    assert (big["status"] == dl.STOP_TRAIN_NO_VALIDATION).all() and (big["n_epochs"] == 1).all()
    t.set(c["d_mfcc"], c["frame_offsets"], scaler_rows=c["train_rows"])
    again = _bytes(*t.train([run], c["labels"]), 0)
    assert again == alone and _bytes(*t.train([run], c["labels"]), 0) == again


def test_statuses(cases):
    """empty train_rows is EMPTY with every output defined; empty val_rows is NO_VALIDATION and returns the last weights; one-label
    training rows train normally"""
    c = cases["A"]
    t, labels = c["trainer"], c["labels"]
    one = c["train_rows"][labels[c["train_rows"]] == 1].astype(np.int32)
    runs = [dict(train_rows=[], val_rows=c["val_rows"], seed=5, epochs=4),
            dict(train_rows=c["train_rows"], val_rows=None, seed=6, epochs=4, batch_size=4, learning_rate=1e-2),
            dict(train_rows=one, val_rows=c["val_rows"], seed=7, epochs=4, batch_size=4, learning_rate=1e-2)]
    res, hist, prob, params = t.train(runs, labels)
    hist, prob, params = hist.cpu().numpy(), prob.cpu().numpy(), params.cpu().numpy()
    refs = [R.train_run(c["z"], labels, c["n_coef"], c["max_frames"], c["units"], r) for r in runs]
    assert [int(s) for s in res["status"]] == [dl.STOP_TRAIN_EMPTY, dl.STOP_TRAIN_NO_VALIDATION, res["status"][2]] and res["status"][2] in (0, 1)
    for k, ref in enumerate(refs):
        for field in INT_FIELDS:
            assert res[k][field] == ref[field], (k, field)
        assert R.relative(hist[k], ref["history"]) <= c["allow"] and R.relative(params[k], ref["params"]) <= c["allow"]
        assert R.relative(prob[k], ref["prob"]) <= c["allow"] and np.isfinite(prob[k]).all()
    assert res[0]["n_epochs"] == 0 and res[0]["best_epoch"] == -1 and np.isnan(res[0]["best_val_loss"]) and np.isnan(res[0]["last_loss"]) and np.isnan(hist[0]).all()
    assert np.array_equal(params[0], R.init(c["n_coef"], c["max_frames"], c["units"], 5))               # the initial weights, bit for bit
    assert res[1]["n_epochs"] == 4 and res[1]["best_epoch"] == -1 and np.isnan(res[1]["best_val_loss"]) and np.isnan(hist[1][:, 1]).all() and res[1]["val_correct"] == 0
    assert np.isfinite(hist[1][:, 0]).all() and np.isfinite(hist[2][:res[2]["n_epochs"]]).all()


def test_row_checks(cases):
    """the row lists are checked against the dataset before a kernel is launched"""
    c = cases["A"]
    t = c["trainer"]
    n = c["labels"].size
    L = dsp_amd.load()
    res = np.zeros(1, dl.STOP_TRAIN_RESULT_DTYPE)
    import torch
    hist, par = torch.zeros(100, dtype=torch.float64, device="cuda"), torch.zeros(t.n_params, dtype=torch.float64, device="cuda")
    tr, va = np.array([0, 2], np.int32), np.array([1], np.int32)
    up, far = np.array([2, 0], np.int32), np.array([0, n], np.int32)

    def call(train=tr, n_train=2, val=va, n_val=1, labels=c["labels"]):
        r = (dl.StopTrainRun * 1)(dl.StopTrainRun(None if train is None else train.ctypes.data, None if val is None else val.ctypes.data, n_train, n_val, 0,
                                                  1e-3, (C.c_double * 3)(0.3, 0.3, 0.2), 32, 2, 2, 1))
        labels = np.ascontiguousarray(labels, np.int32)
        return L.dsp_stop_train_runs_device(t._h, r, 1, labels.ctypes.data, res.ctypes.data, hist.data_ptr(), None, par.data_ptr(), None)

    bad = c["labels"].copy()
    bad[1] = 2
    for f, msg in ((lambda: call(train=None), "train_rows is NULL"), (lambda: call(n_train=n + 1), "n_train must be 0 .. n"),
                   (lambda: call(train=up), r"train_rows must be strictly ascending \(train_rows\[1\]\)"), (lambda: call(val=np.array([1, 1], np.int32), n_val=2), "val_rows must be strictly ascending"),
                   (lambda: call(train=far), r"train_rows\[1\] = %d is out of range" % n), (lambda: call(val=None), "val_rows is NULL"),
                   (lambda: call(labels=bad), r"labels\[1\] = 2 is neither 0 nor 1")):
        assert f() == -1 and re.search(msg, dl.last_error()), (msg, dl.last_error())
    assert call() == 0
    with pytest.raises(ValueError, match="unknown keys"):
        t.train([dict(train_rows=tr, val_rows=va, lr=1.0)], c["labels"])


def test_round_trip_and_fit(cases):
    """the fitted model through dsp_stop_model_from_training -> dsp_stop_model_create -> dsp_stop_predict_device on the dataset's own MFCC
    reproduces d_prob within StopNet's own first-order bound (the one tests/test_gpu_consumer_models.py uses); StopTrainer.fit over 16
    seeds returns the run with the lowest best_val_loss"""
    c = cases["C"]
    t = c["trainer"]
    assert c["labels"].size == 40 and (np.diff(c["frame_offsets"]) == 98).all() and c["n_coef"] == 13
    U.check_round_trip(c, 0, range(0, 40, 3))
    seeds = list(range(16))
    hyper = {key: c["runs"][0][key] for key in ("batch_size", "epochs", "patience", "learning_rate")}
    fitted, report = t.fit(c["labels"], c["train_rows"], c["val_rows"], seeds=seeds, **hyper)
    res = report["results"]
    loss = np.where(np.isnan(res["best_val_loss"]), np.inf, res["best_val_loss"])
    assert report["best"] == int(np.argmin(loss)) and report["seed"] == seeds[report["best"]] and len(res) == 16
    ref = R.train_run(c["z"], c["labels"], c["n_coef"], c["max_frames"], c["units"], dict(train_rows=c["train_rows"], val_rows=c["val_rows"], seed=report["seed"], **hyper))
    assert R.relative(report["params"], ref["params"]) <= c["allow"] and abs(res["best_val_loss"][report["best"]] - ref["best_val_loss"]) <= c["allow"]
    assert np.array_equal(fitted["kernel0"], ref["params"][:6500 * 4].astype(np.float32)) or R.relative(fitted["kernel0"], ref["params"][:6500 * 4]) < 1e-6
    assert report["n_dead_runs"] == int((res["n_dead_units"] > 0).sum())


def test_from_audio():
    """tests/signals.py tone bursts against noise, 24 one-second clips, the reference plan: StopModel.train followed by
    classify_signal_batch separates the training clips when the restatement does on the same MFCC (asserted first)"""
    import torch
    from tests import signals as S
    n, fs = 24, 16000.0
    labels = np.arange(n) % 2
    clips = np.stack([(0.05 * S.uniform_pm1(16000, 100 + i) + (S.tone_burst(16000, fs, [(0.2 + 0.01 * i, 0.6 + 0.01 * i)], [700.0, 1900.0], [0.3, 0.2]) if labels[i] else 0.0)).astype(np.float32)
                      for i in range(n)])
    plan = dsp_amd.MfccPlan(dsp_amd.default_config())
    d_clips = torch.from_numpy(clips).cuda()
    mfcc = plan.clips(d_clips, 500).cpu().numpy()
    t_frames = mfcc.shape[1]
    hyper = dict(epochs=40, patience=40, learning_rate=1e-2, batch_size=8, dropout=(0.1, 0.1, 0.0))
    seeds = list(range(8))
    fo = np.arange(n + 1) * t_frames
    x = R.features(mfcc.reshape(-1, 13), fo, 13, 500)
    mean, scale = R.scaler_fit(x, 13, 500)
    z = R.standardise(x, mean, scale, 13, 500)
    rows = np.arange(n)
    refs = [R.train_run(z, labels, 13, 500, (4, 2, 2, 1), dict(train_rows=rows, val_rows=rows, seed=s, **hyper)) for s in seeds]
    best = int(np.argmin([r["best_val_loss"] for r in refs]))
    assert refs[best]["val_correct"] == n and refs[best]["p_margin"] > 0.05                       # the restatement separates the clips
    model, report = dsp_amd.StopModel.train(plan, d_clips, labels, seeds=seeds, **hyper)
    assert report["best"] == best and report["results"]["val_correct"][best] == n
    p = model.classify_signal_batch(plan, d_clips).cpu().numpy()
    assert np.array_equal(p > 0.5, labels == 1), p
    assert np.abs(p - refs[best]["prob"]).max() < 1e-3
    model.close()
