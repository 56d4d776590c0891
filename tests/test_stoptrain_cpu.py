"""CPU: the float64 restatement of stop-net training (tests/stoptrain_ref.py) against torch.autograd, Adam's closed first step and a
hand-made early-stopping sequence; the host helpers of the C ABI (dsp_stop_train_uniform / _order / _init / _param_count,
dsp_stop_model_from_training) against the restatement, bit for bit; that the restatement learns a planted direction (and that one seed
dies); the spread the GPU tests' allowance is four times of; the argument checks of every dsp_stop_train_* entry point and the loud
failure without a GPU.  No kernel runs here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dsp_amd
from dsp_amd import consumers as dc
from dsp_amd import lib as dl

from tests import consumer_ref as CR
from tests import stoptrain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the restatement-learns test: seeds picked on the CPU -- the first three reach 100 % validation accuracy with every hidden unit live, the
# last ends in the dead-ReLU plateau (a whole hidden layer dead, the output a constant)
LEARN = dict(n_coef=5, max_frames=12, units=(4, 2, 2, 1), n=96, n_train=64, epochs=60, learning_rate=2e-2, dropout=(0.1, 0.1, 0.0), patience=60)
LIVE_SEEDS, DEAD_SEED = (0, 4, 9), 38


def _small(seed=0, n_coef=3, max_frames=7, units=(4, 3, 2, 1), batch=6):
    rng = np.random.default_rng(seed)
    ws, bs = R.unpack(R.init(n_coef, max_frames, units, seed), n_coef, max_frames, units)
    bs = [b + 0.1 * rng.standard_normal(b.shape) for b in bs]
    zb = rng.standard_normal((batch, n_coef * max_frames)).astype(np.float32).astype(np.float64)
    yb = (rng.random(batch) < 0.5).astype(np.float64)
    return ws, bs, zb, yb, units


def test_batch_gradient_is_autograd():
    """the restated batch gradient equals torch.autograd's in float64 with the same weights, batch and dropout masks, to 1e-12 relative"""
    import torch
    for seed, rates in ((0, (0.0, 0.0, 0.0)), (1, (0.3, 0.3, 0.2)), (2, (0.5, 0.0, 0.4))):
        ws, bs, zb, yb, units = _small(seed)
        masks = R.dropout_masks(seed, 7, zb.shape[0], units, rates)
        scales = [1.0 / (1.0 - r) for r in rates]
        loss, gw, gb = R.batch_gradient(ws, bs, zb, yb, masks, scales)
        tw = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
        tb = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
        h = torch.tensor(zb, dtype=torch.float64)
        for l in range(3):
            h = torch.relu(h @ tw[l] + tb[l])
            if masks[l] is not None:
                h = h * torch.tensor(masks[l], dtype=torch.float64) * scales[l]
        a = (h @ tw[3] + tb[3])[:, 0]
        tl = torch.nn.functional.binary_cross_entropy_with_logits(a, torch.tensor(yb, dtype=torch.float64), reduction="mean")
        tl.backward()
        assert abs(loss.mean() - tl.item()) <= 1e-12 * abs(tl.item())
        for got, want in zip(gw + gb, [w.grad.numpy() for w in tw] + [b.grad.numpy() for b in tb]):
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (seed, np.abs(got - want).max())
        assert any(np.abs(g).max() > 0 for g in gw)


def test_first_adam_step_is_the_closed_form():
    """at t = 1 every weight with a non-zero gradient moves by lr g / (|g| + eps / sqrt(1 - beta2))"""
    rng = np.random.default_rng(3)
    g = rng.standard_normal(200) * 10.0 ** rng.uniform(-9, 2, 200)
    g[::7] = 0.0
    w0 = rng.standard_normal(200)
    w, m, v = w0.copy(), np.zeros(200), np.zeros(200)
    lr = 1e-3
    R.adam_step(w, m, v, g, lr, 1)
    want = lr * g / (np.abs(g) + R.ADAM_EPS / math.sqrt(1.0 - R.BETA2))
    nz = g != 0
    assert np.abs((w0 - w)[nz] - want[nz]).max() <= 1e-12 * lr and np.array_equal(w[~nz], w0[~nz])


def test_weights_of_unused_features_never_change():
    """clips shorter than max_frames: the run on the used features returns the initial draw on the others, and equals (to rounding) the
    run that is handed every feature, whose padded inputs standardise to exactly 0"""
    c = R.case("A")
    short = np.minimum(np.diff(c["frame_offsets"]), 4)                # T_used = 4 < max_frames = 7
    fo = np.concatenate([[0], np.cumsum(short)])
    mfcc = np.concatenate([c["mfcc"][a:a + t] for a, t in zip(c["frame_offsets"][:-1], short)])
    x = R.features(mfcc, fo, c["n_coef"], c["max_frames"])
    assert x.shape[1] == 3 * 4
    mean, scale = R.scaler_fit(x, c["n_coef"], c["max_frames"])
    z = R.standardise(x, mean, scale, c["n_coef"], c["max_frames"])
    run = c["runs"][0]
    got = R.train_run(z, c["labels"], c["n_coef"], c["max_frames"], c["units"], run)
    idx = R.used_index(c["n_coef"], c["max_frames"], 4)
    w0 = R.unpack(R.init(c["n_coef"], c["max_frames"], c["units"], run["seed"]), c["n_coef"], c["max_frames"], c["units"])[0][0]
    w1 = R.unpack(got["params"], c["n_coef"], c["max_frames"], c["units"])[0][0]
    unused = np.setdiff1d(np.arange(w0.shape[0]), idx)
    assert np.array_equal(w1[unused], w0[unused]) and not np.array_equal(w1[idx], w0[idx])
    z_full = np.zeros((z.shape[0], w0.shape[0]), np.float32)
    z_full[:, idx] = z
    full = R.train_run(z_full.reshape(z.shape[0], 3, 7).reshape(z.shape[0], -1), c["labels"], c["n_coef"], c["max_frames"], c["units"],
                       run, feature_order="asc")
    w1_full = R.unpack(full["params"], c["n_coef"], c["max_frames"], c["units"])[0][0]
    assert np.array_equal(w1_full[unused], w0[unused]) and R.relative(full["params"], got["params"]) <= 1e-12


def test_early_stopping_sequence():
    """EarlyStopping on hand-made val_loss sequences: the strict <, a NaN entry, patience, and the weights a run restores"""
    nan = math.nan
    assert R.early_stopping([1.0, 0.9, 0.9, 0.95, 0.8, 0.85], 2, 6) == (4, 1, 1)            # the equal 0.9 does not improve: stops before the 0.8
    assert R.early_stopping([1.0, 0.9, 0.9, 0.95, 0.8, 0.85], 3, 6) == (6, 4, 4)
    assert R.early_stopping([1.0, nan, 0.5, nan, nan, 0.4], 2, 6) == (5, 2, 2)              # NaN never improves and counts as a wait
    assert R.early_stopping([nan, nan, nan], 5, 3) == (3, -1, -1)
    assert R.early_stopping([0.5, 0.6, 0.7], 0, 3) == (2, 0, 0)
    # a run restores the snapshot of its best epoch: the same run cut off right there ends with the same weights
    c = R.case_reference("C")
    k = next(i for i, r in enumerate(c["numpy"]) if r["status"] == R.CONVERGED_EARLY)
    r = c["numpy"][k]
    assert r["n_epochs"] == r["best_epoch"] + 1 + c["runs"][k]["patience"] and r["n_epochs"] < c["runs"][k]["epochs"]
    assert np.nanargmin(r["history"][:, 1]) == r["best_epoch"] and r["best_val_loss"] == r["history"][r["best_epoch"], 1]
    cut = R.train_run(c["z"], c["labels"], c["n_coef"], c["max_frames"], c["units"], {**c["runs"][k], "epochs": r["best_epoch"] + 1, "restore_best": False})
    assert np.array_equal(cut["params"], r["params"])
    last = R.train_run(c["z"], c["labels"], c["n_coef"], c["max_frames"], c["units"], {**c["runs"][k], "restore_best": False})
    assert not np.array_equal(last["params"], r["params"]) and np.array_equal(last["history"], r["history"], equal_nan=True)


def test_order_is_a_keyed_permutation():
    for n in (1, 2, 3, 5, 64, 65, 1000):
        o = dc.stop_train_order(n, 7, 0)
        assert np.array_equal(np.sort(o), np.arange(n)) and np.array_equal(o, R.order(n, 7, 0))
        if n >= 64:
            assert not np.array_equal(o, dc.stop_train_order(n, 7, 1)) and not np.array_equal(o, dc.stop_train_order(n, 8, 0))
        assert np.array_equal(dc.stop_train_order(n, 2**63 + 11, 49), R.order(n, 2**63 + 11, 49))
    L = dsp_amd.load()
    o = np.zeros(4, np.int32)
    assert L.dsp_stop_train_order(0, 0, 0, o.ctypes.data) == -1 and "n must be 1 .. 65536" in dl.last_error()
    assert L.dsp_stop_train_order(4, 0, -1, o.ctypes.data) == -1 and L.dsp_stop_train_order(4, 0, 0, None) == -1 and "order is NULL" in dl.last_error()


def test_draws_and_initial_weights_are_the_restatement():
    for seed, stream, counter in ((0, 0, 0), (1, 2, 3), (2**64 - 1, 2, 2**40 + 5), (12345, 1, 49)):
        u = dc.stop_train_uniform(seed, stream, counter)
        assert u == R.uniform(seed, stream, counter) == R.uniform_v(seed, stream, [counter])[0] and 0.0 <= u < 1.0
    for n_coef, max_frames, units in ((3, 7, (4, 2, 2, 1)), (13, 50, (16, 16, 16, 1)), (13, 500, (4, 2, 2, 1))):
        assert dc.stop_train_param_count(n_coef, max_frames, units) == R.param_count(n_coef, max_frames, units)
        p = dc.stop_train_init(n_coef, max_frames, units, 2**63 + 9)
        assert np.array_equal(p, R.init(n_coef, max_frames, units, 2**63 + 9))
        ws, bs = R.unpack(p, n_coef, max_frames, units)
        for w, b in zip(ws, bs):
            limit = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))
            assert np.abs(w).max() <= limit and (w.size < 64 or np.abs(w).max() > 0.9 * limit) and not b.any()
    assert dc.stop_train_param_count(13, 500, (4, 2, 2, 1)) == 26000 + 4 + 8 + 2 + 4 + 2 + 2 + 1


def test_model_from_training_round_trips_into_stopnet():
    n_coef, max_frames, units = 3, 7, (4, 3, 2, 1)
    rng = np.random.default_rng(4)
    params = R.init(n_coef, max_frames, units, 5) + 0.01 * rng.standard_normal(R.param_count(n_coef, max_frames, units))
    mean, scale = rng.standard_normal(21).astype(np.float32), rng.uniform(0.5, 2.0, 21).astype(np.float32)
    scale[3] = 0.0
    got, want = dc.stop_model_from_training(n_coef, max_frames, units, params, mean, scale), R.model_from_training(n_coef, max_frames, units, params, mean, scale)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    net = CR.StopNet(got)
    assert net.units == list(units) and np.array_equal(net.w[0], R.unpack(params, n_coef, max_frames, units)[0][0].astype(np.float32))
    mfcc = rng.standard_normal((5, n_coef)).astype(np.float32)
    z = R.standardise(R.features(mfcc, [0, 5], n_coef, max_frames), mean, scale, n_coef, max_frames)
    full = np.zeros((1, 21), np.float32)                                # the padded frames standardise to (0 - mean) / div
    full[0] = net.standardise(np.zeros(21, np.float32))
    full[0, R.used_index(n_coef, max_frames, 5)] = z[0]
    ws, bs = R.unpack(params, n_coef, max_frames, units)
    p64 = R.sigmoid(R.forward([w.astype(np.float32).astype(np.float64) for w in ws], [b.astype(np.float32).astype(np.float64) for b in bs], full.astype(np.float64))[0])[0]
    p, bound = net.prob(mfcc)
    assert abs(float(p) - p64) <= bound + 1e-6
    L = dsp_amd.load()
    u = (C.c_int * 4)(*units)
    bad = params.copy()
    bad[5] = np.nan
    arrays, m = np.zeros(2 * 21 + params.size, np.float32), dl.StopModelParams()
    assert L.dsp_stop_model_from_training(n_coef, max_frames, u, bad.ctypes.data, mean.ctypes.data, scale.ctypes.data, arrays.ctypes.data, C.byref(m)) == -1
    assert "params[5] is not finite" in dl.last_error()
    assert L.dsp_stop_model_from_training(n_coef, max_frames, u, None, mean.ctypes.data, scale.ctypes.data, arrays.ctypes.data, C.byref(m)) == -1


def _learn_set():
    h = LEARN
    mfcc, fo, labels = R.planted(21, h["n_coef"], [h["max_frames"]] * h["n"], 3)
    x = R.features(mfcc, fo, h["n_coef"], h["max_frames"])
    rows = np.arange(h["n"])
    train_rows, val_rows = rows[:h["n_train"]], rows[h["n_train"]:]
    z = R.standardise(x, *R.scaler_fit(x, h["n_coef"], h["max_frames"], train_rows), h["n_coef"], h["max_frames"])
    return z, labels, train_rows, val_rows


def test_the_restatement_learns_and_one_seed_dies():
    """On a set separable by a planted direction the picked seeds reach 100 % validation accuracy with a live unit in every layer.  One
    further seed ends on the plateau tests/golden/make_golden.py works around: its last hidden layer is dead on every training row, the
    output is a constant and val_loss stays at ln 2.  A seed alone cannot kill EVERY hidden unit -- once a layer is dead no gradient
    reaches the layers below it, which therefore stay as alive as they were -- so n_dead_units equal to all of them is shown on an input
    that does it: training clips that are all alike standardise to 0, every pre-activation is its zero bias, and nothing ever moves."""
    h = LEARN
    z, labels, train_rows, val_rows = _learn_set()
    hyper = {k: h[k] for k in ("epochs", "learning_rate", "dropout", "patience")}
    for seed in LIVE_SEEDS + (DEAD_SEED,):
        r = R.train_run(z, labels, h["n_coef"], h["max_frames"], h["units"], dict(train_rows=train_rows, val_rows=val_rows, seed=seed, **hyper))
        ws, bs = R.unpack(r["params"], h["n_coef"], h["max_frames"], h["units"])
        live = [int((hl.max(axis=0) > 0).sum()) for hl in R.forward(ws, bs, z[train_rows].astype(np.float64))[1]]
        print(f"seed {seed}: val {r['val_correct']}/{val_rows.size}, live units {live}, dead {r['n_dead_units']}, best_val_loss {r['best_val_loss']:.4f}")
        assert r["n_dead_units"] == sum(h["units"][:3]) - sum(live)
        if seed == DEAD_SEED:
            assert live[2] == 0 and r["n_dead_units"] >= h["units"][2] and np.ptp(r["prob"]) == 0.0 and abs(r["best_val_loss"] - math.log(2.0)) < 1e-3
        else:
            assert r["val_correct"] == val_rows.size and min(live) >= 1 and r["n_dead_units"] == 0
    alike = np.zeros_like(z)
    r = R.train_run(alike, labels, h["n_coef"], h["max_frames"], h["units"], dict(train_rows=train_rows, val_rows=val_rows, seed=0, **{**hyper, "epochs": 3}))
    assert r["n_dead_units"] == sum(h["units"][:3]) and np.ptp(r["prob"]) == 0.0


@pytest.mark.parametrize("name", R.CASES_OLD + R.CASES_NEW)
def test_restatement_spread(name):
    """The restatement with the layer-1 feature sum ascending and descending: the largest relative difference in history, params and prob
    over the GPU tests' runs is the spread; the device's allowance is 4 x it (the factor of DESIGN.md 3.20), floored at 1e-9.  Measured:
    A 6.1e-16, B 5.0e-15, C 6.5e-15, D 3.4e-15, E 2.4e-16, F 2.0e-15, G 1.2e-15, H 4.9e-15.  The runs' conditions are asserted here too: every deciding val_loss comparison and every
    validation row's |P - 0.5| has a margin above 1e-6, the two orders take the same decisions, and case C stops early.  (What the
    cases D .. H reach is asserted in tests/test_stoptrain_shapes_cpu.py.)"""
    c = R.case_reference(name)
    print(f"{name}: spread {c['spread']:.3e}, allowance {c['allow']:.3e}")
    assert c["spread"] < 1e-10 and c["allow"] == max(4 * c["spread"], R.FLOOR)
    for a, d, m in zip(c["asc"], c["desc"], c["numpy"]):
        for k in ("n_epochs", "best_epoch", "status", "val_correct", "n_dead_units"):
            assert a[k] == d[k] == m[k], k
        assert m["margin"] > 1e-6 and m["p_margin"] > 1e-6
        assert max(R.relative(m[k], a[k]) for k in ("history", "params", "prob")) <= c["allow"]
    if name == "C":
        assert any(r["status"] == R.CONVERGED_EARLY for r in c["numpy"]) and c["z"].shape[1] == 1274
    if name == "A":
        assert c["z"].shape[1] == 21 and c["train_rows"].size % c["runs"][0]["batch_size"] == 1


def test_argument_checks_come_before_any_device():
    L = dsp_amd.load()
    h = C.c_void_p()
    units = (C.c_int * 4)(4, 2, 2, 1)
    assert L.dsp_stop_trainer_create(0, 3, 7, units, None) == -1 and "out is NULL" in dl.last_error()
    for args, msg in (((-1, 3, 7, units), "device"), ((0, 0, 7, units), "n_coef"), ((0, 3, 0, units), "max_frames"), ((0, 3, 7, None), "units is NULL"),
                      ((0, 3, 7, (C.c_int * 4)(4, 17, 2, 1)), r"units\[1\] must be 1 .. 16"), ((0, 3, 7, (C.c_int * 4)(4, 2, 0, 1)), r"units\[2\]"),
                      ((0, 3, 7, (C.c_int * 4)(4, 2, 2, 2)), r"units\[3\] must be 1")):
        assert L.dsp_stop_trainer_create(*args, C.byref(h)) == -1 and re.search(msg, dl.last_error()), (msg, dl.last_error())
    assert L.dsp_stop_trainer_create(0, 3, 7, units, C.byref(h)) == 0 and h.value                       # (touches no device)
    mfcc = np.zeros((8, 3), np.float32)
    fp = mfcc.ctypes.data                                                                               # (never read: every call below fails first)
    fo = np.array([0, 2, 5, 8], np.int64)
    bad_fo = np.array([0, 5, 2, 8], np.int64)
    neg_fo = np.array([-1, 2, 5, 8], np.int64)
    rows = np.array([0, 3], np.int32)
    ok21 = np.zeros(21, np.float32)
    nan21 = ok21.copy()
    nan21[4] = np.nan

    def set_(t=h, f=fp, n=3, o=fo, sr=None, nsr=0, m=None, s=None):
        return L.dsp_stop_train_set_device(t, f, n, None if o is None else o.ctypes.data, sr, nsr, m, s, None, None, None)

    for call, msg in ((lambda: set_(t=None), "trainer is NULL"), (lambda: set_(f=None), "d_mfcc is NULL"), (lambda: set_(n=0), "n must be >= 1"),
                      (lambda: set_(n=65537, o=fo), "above the cap of 65536"), (lambda: set_(o=None), "frame_offsets is NULL"),
                      (lambda: set_(o=bad_fo), "frame_offsets decrease at clip 1"), (lambda: set_(o=neg_fo), "non-negative"),
                      (lambda: set_(m=ok21.ctypes.data), "given together"), (lambda: set_(s=ok21.ctypes.data), "given together"),
                      (lambda: set_(m=nan21.ctypes.data, s=ok21.ctypes.data), "feature 4 is not finite"),
                      (lambda: set_(sr=rows.ctypes.data, nsr=2), r"scaler_rows\[1\] = 3 is out of range"), (lambda: set_(sr=rows.ctypes.data, nsr=0), "n_scaler_rows")):
        assert call() == -1 and re.search(msg, dl.last_error()), (msg, dl.last_error())
    # no dataset yet
    labels = np.array([0, 1, 0], np.int32)
    res = np.zeros(1, dl.STOP_TRAIN_RESULT_DTYPE)
    tr, va = np.array([0, 2], np.int32), np.array([1], np.int32)

    def run(**kw):
        d = dict(train_rows=tr.ctypes.data, val_rows=va.ctypes.data, n_train=2, n_val=1, seed=0, learning_rate=1e-3, dropout=(0.3, 0.3, 0.2), batch_size=32,
                 epochs=5, patience=2, restore_best=1)
        d.update(kw)
        return (dl.StopTrainRun * 1)(dl.StopTrainRun(d["train_rows"], d["val_rows"], d["n_train"], d["n_val"], d["seed"], d["learning_rate"],
                                                     (C.c_double * 3)(*d["dropout"]), d["batch_size"], d["epochs"], d["patience"], d["restore_best"]))

    def runs_(t=h, r=None, n_runs=1, lab=labels, out=res, hist=fp, par=fp, null_runs=False):
        return L.dsp_stop_train_runs_device(t, None if null_runs else (run() if r is None else r), n_runs, None if lab is None else lab.ctypes.data,
                                            None if out is None else out.ctypes.data, hist, None, par, None)

    # what needs no dataset to be judged is refused first, then the missing dataset (the row lists are checked against it:
    # tests/test_gpu_stoptrain.py test_row_checks)
    for call, msg in ((lambda: runs_(t=None), "trainer is NULL"), (lambda: runs_(n_runs=-1), "n_runs must be 0 .. 4096"), (lambda: runs_(n_runs=4097), "n_runs"),
                      (lambda: runs_(null_runs=True), "runs is NULL"), (lambda: runs_(out=None), "results is NULL"), (lambda: runs_(hist=None), "d_history is NULL"),
                      (lambda: runs_(par=None), "d_params is NULL"), (lambda: runs_(lab=None), "labels is NULL"),
                      (lambda: runs_(r=run(learning_rate=0.0)), "learning_rate"), (lambda: runs_(r=run(learning_rate=np.nan)), "learning_rate"),
                      (lambda: runs_(r=run(dropout=(0.3, 1.0, 0.2))), r"dropout\[1\]"), (lambda: runs_(r=run(dropout=(-0.1, 0.0, 0.2))), r"dropout\[0\]"),
                      (lambda: runs_(r=run(batch_size=0)), "batch_size must be 1 .. 256"), (lambda: runs_(r=run(batch_size=257)), "batch_size"),
                      (lambda: runs_(r=run(epochs=0)), "epochs must be 1 .. 10000"), (lambda: runs_(r=run(epochs=10001)), "epochs"),
                      (lambda: runs_(r=run(patience=-1)), "patience"), (lambda: runs_(r=run(restore_best=2)), "restore_best"),
                      (lambda: runs_(), "no dataset")):
        assert call() == -1 and re.search(msg, dl.last_error()), (msg, dl.last_error())
    assert L.dsp_stop_train_rows_host(h, fp, None) == -1 and "no dataset" in dl.last_error()
    assert L.dsp_stop_train_rows_host(h, None, None) == -1 and "z is NULL" in dl.last_error()
    assert L.dsp_stop_train_used_features(h) == 0 and L.dsp_stop_train_used_features(None) == -1
    if L.dsp_device_count() <= 0:                                                                       # loud: there is no CPU fallback
        assert set_() == -2 and "no HIP device" in dl.last_error()
    L.dsp_stop_trainer_destroy(h)
    L.dsp_stop_trainer_destroy(None)
    assert L.dsp_stop_train_param_count(0, 7, units) == -1 and L.dsp_stop_train_param_count(3, 7, None) == -1
    assert L.dsp_stop_train_init(3, 7, units, 0, None) == -1 and "params is NULL" in dl.last_error()


def test_python_argument_checks():
    """the Python layer's own checks raise ValueError (they are not asserts) before any device call"""
    with pytest.raises(ValueError, match="four layer widths"):
        dc.StopTrainer(3, 7, (4, 2, 1))
    with pytest.raises(dsp_amd.DspError, match=r"units\[3\] must be 1"):
        dc.StopTrainer(3, 7, (4, 2, 2, 2))
    t = dc.StopTrainer(3, 7)
    with pytest.raises(ValueError, match="at least one clip"):
        t.set(None, [0])
    with pytest.raises(ValueError, match="CUDA tensor"):
        t.set(np.zeros((4, 3), np.float32), [0, 4])
    with pytest.raises(ValueError, match="labels must hold"):
        t.train([], [0, 1])
    with pytest.raises(ValueError, match="params must hold"):
        dc.stop_model_from_training(3, 7, (4, 2, 2, 1), np.zeros(5), np.zeros(21), np.ones(21))
    t.close()


def test_the_feature_is_wired_in():
    L = dsp_amd.load()
    header = open(os.path.join(ROOT, "include", "dsp_amd.h")).read()
    exports = open(os.path.join(ROOT, "dsp_amd", "csrc", "exports.map")).read()
    names = ["dsp_stop_trainer_create", "dsp_stop_trainer_destroy", "dsp_stop_train_set_device", "dsp_stop_train_used_features", "dsp_stop_train_rows_host",
             "dsp_stop_train_runs_device", "dsp_stop_train_param_count", "dsp_stop_train_uniform", "dsp_stop_train_order", "dsp_stop_train_init",
             "dsp_stop_model_from_training"]
    assert re.search(r"^\s*dsp_\*;", exports, re.M)                    # (the export list takes every dsp_ name of the header)
    for name in names:
        assert name in dl.SYMBOLS and hasattr(L, name) and re.search(r"\b%s\(" % name, header), name
    assert "capi_stoptrain.cpp" in dsp_amd.build.SOURCES and "stoptrain_kernels.hip" in dsp_amd.build.SOURCES and "stoptrain_kernels.hpp" in dsp_amd.build.HEADERS
    for i, name in enumerate(("CONVERGED_EARLY", "MAX_EPOCHS", "NO_VALIDATION", "EMPTY")):
        assert re.search(r"#define DSP_STOP_TRAIN_%s %d\b" % (name, i), header) and getattr(dl, "STOP_TRAIN_" + name) == i == getattr(R, name)
    for name, cap in (("ROWS", 65536), ("UNITS", 16), ("BATCH", 256), ("EPOCHS", 10000), ("RUNS", 4096)):
        assert re.search(r"#define DSP_STOP_TRAIN_CAP_%s %d\b" % (name, cap), header) and getattr(dl, "STOP_TRAIN_CAP_" + name) == cap
    assert C.sizeof(dl.StopTrainRun) == 88 and C.sizeof(dl.StopTrainResult) == 40 == np.dtype(dl.STOP_TRAIN_RESULT_DTYPE).itemsize
    assert hasattr(dsp_amd, "StopTrainer") and hasattr(dsp_amd.StopModel, "train")
    assert dc.StopTrainer.HYPER == R.HYPER
