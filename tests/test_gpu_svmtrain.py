"""GPU: SVM training (dsp_svm_train_*, dsp_svm_fit_device, SvmTrainer) against the float64 restatement of
tests/svmtrain_ref.py and sklearn's answers of tests/golden/svmtrain.npz.

The parity allowance is four times the restatement's own spread max |dec_ref(1e-7) - dec_ref(1e-10)| over the problems solved here,
measured on the CPU and asserted there (tests/test_svmtrain_cpu.py test_restatement_spread, svmtrain_ref.SPREAD): 5.3e-8 (nf40),
2.4e-7 (nf3), 2.1e-7 (nf1), 6.9e-8 (cepstrum), 2.0e-7 (the cross-validation grid) -- two solvers that stop at different points inside
the same eps shell.  Nothing here is derived from what the GPU returns.  Iteration counts are not compared: a last-ulp difference in
exp may fork the path."""
import numpy as np
import pytest

from dsp_amd import lib as dl
from dsp_amd import scrubjay as sj

from tests import svm_ref as S
from tests import svmtrain_ref as R

pytestmark = pytest.mark.gpu
SETS = ("nf40", "nf3", "nf1", "cepstrum")
EPS = 1e-7


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _problems(name, d):
    if name == "cepstrum":                                             # (8 rows: sklearn's problem only)
        return [("all", np.arange(d["labels"].size, dtype=np.int32), d["c"][0], d["c"][1], d["gamma"])]
    return R.suite_problems(d["labels"], d["c"], d["gamma"], d["x"].shape[1])


@pytest.fixture(scope="module")
def sets(golden):
    """per golden set: its arrays, the restatement's answers to its problems (computed once, left unchanged) and the device's, from ONE
    launch of all of them on the golden Scaler"""
    g = golden("svmtrain.npz")
    out = {}
    for name in SETS:
        d = {k: g[f"{name}__{k}"] for k in ("x", "labels", "offset", "scale", "gamma", "c", "intercept", "decision_function", "predict")}
        d["gamma"] = float(d["gamma"])
        d["z"] = R.standardise(d["x"], d["offset"], d["scale"])
        d["d2"] = R.distances(d["z"])
        d["problems"] = _problems(name, d)
        d["ref"] = [R.solve(d["d2"], d["labels"], rows, c0, c1, gamma, EPS) for _pn, rows, c0, c1, gamma in d["problems"]]
        d["feat"] = _cuda(d["x"])
        t = sj.SvmTrainer(d["x"].shape[1])
        t.set(d["feat"], offset=d["offset"], scale=d["scale"])
        res, coef, dec = t.problems([p[1:] for p in d["problems"]], d["labels"], eps=EPS)
        d["trainer"], d["res"], d["coef"], d["dec"] = t, res, coef.cpu().numpy(), dec.cpu().numpy()
        out[name] = d
    yield out
    for d in out.values():
        d["trainer"].close()


@pytest.mark.parametrize("name", SETS)
def test_scaler_and_rows(sets, name):
    """the fitted Scaler (all rows, a subset) against the restatement's to the last float32 ulp (another order of the float64 sums may
    move a rounding), and the standardised rows bit for bit under the same Scaler"""
    d = sets[name]
    n = d["labels"].size
    t = sj.SvmTrainer(d["x"].shape[1])
    for rows in (None, np.arange(1, n, 2, dtype=np.int32)):
        off, scl = t.set(d["feat"], scaler_rows=rows)
        want_off, want_scl = R.scaler_fit(d["x"], rows)
        assert np.all(np.abs(off - want_off) <= np.spacing(np.abs(want_off))) and np.all(np.abs(scl - want_scl) <= np.spacing(want_scl))
        assert np.array_equal(t.rows(), R.standardise(d["x"], off, scl))
    const = d["x"].copy()
    const[:, 0] = 2.5                                                 # a constant feature: std 0 gives scale 1
    off, scl = t.set(_cuda(const))
    assert off[0] == 2.5 and scl[0] == 1.0 and np.all(t.rows()[:, 0] == 0.0)
    t.close()


@pytest.mark.parametrize("name", SETS)
def test_feasible_and_optimal(sets, name):
    """0 <= alpha <= C per label, |sum alpha y| <= 1e-12 sum C, the reported violation below eps and the violation recomputed in
    float64 from the returned coef within eps + 1e-9; the counts and the objective agree with the returned coef"""
    d = sets[name]
    lab = d["labels"]
    for k, (pn, rows, c0, c1, gamma) in enumerate(d["problems"]):
        coef, res = d["coef"][k], d["res"][k]
        y = np.where(lab[rows] == 0, 1.0, -1.0)
        cb = np.where(lab[rows] == 0, c0, c1)
        alpha = coef[rows] * y
        off = np.ones(lab.size, bool)
        off[rows] = False
        assert res["status"] == dl.SVM_TRAIN_CONVERGED and np.all(coef[off] == 0.0), pn
        assert np.all(alpha >= 0.0) and np.all(alpha <= cb) and abs((alpha * y).sum()) <= 1e-12 * cb.sum(), pn
        gap = R.violation_gap(d["d2"], lab, rows, coef, c0, c1, gamma)
        print(f"{name} {pn}: {res['n_iter']} steps, gap {res['gap']:.3e} reported, {gap:.3e} recomputed")
        assert res["gap"] < EPS and gap <= EPS + 1e-9, pn
        assert res["n_sv"] == (alpha > 0).sum() and res["n_bounded"] == (alpha >= cb).sum(), pn
        sub = np.exp(-gamma * d["d2"][np.ix_(rows, rows)])
        objective = 0.5 * coef[rows] @ sub @ coef[rows] - alpha.sum()
        assert abs(res["objective"] - objective) <= 1e-9 * max(1.0, abs(objective)), pn
        if pn == "bounded":
            assert res["n_bounded"] == rows.size                      # (no free alpha: rho is the midpoint of the bounds)
        if pn == "unbounded":
            assert res["n_bounded"] == 0


@pytest.mark.parametrize("name", SETS)
def test_parity_with_the_restatement(sets, name):
    """decisions of all rows, members and held-out, and rho, within 4 x the restatement's own spread"""
    d = sets[name]
    allow = 4 * R.SPREAD[name]
    for k, (pn, _rows, _c0, _c1, gamma) in enumerate(d["problems"]):
        want = R.decisions(d["d2"], d["ref"][k], gamma)
        scale = max(1.0, np.abs(want).max() / 10.0)
        err, rho = np.abs(d["dec"][k] - want).max(), abs(d["res"][k]["rho"] - d["ref"][k]["rho"])
        print(f"{name} {pn}: |dec - ref| {err:.3e}, |rho - ref| {rho:.3e}, allowance {allow * scale:.3e}")
        assert err <= allow * scale and rho <= allow * scale, pn


@pytest.mark.parametrize("name", SETS)
def test_parity_with_sklearn(sets, name):
    """The problem on all rows against sklearn's SVC at tol = 1e-9 (tests/golden/svmtrain.npz), solved with q_float32: the solver's
    kernel values rounded to float32 as libsvm rounds the rows of Q it caches (svm.cpp Qfloat).  Decisions of all rows and rho within
    4 x the spread of the restatement in that mode (svmtrain_ref.SPREAD_Q32, measured and asserted on the CPU: 5.1e-8, 2.2e-7, 9.9e-8,
    6.9e-8), against sklearn and against the restatement; the solution is feasible, and optimal under the rounded kernel.

    In float64, the default, the answer is that of another problem -- the kernel not rounded to 6e-8 -- and stands from sklearn at
    6.3e-8 (nf40), 2.87e-6 (nf3), 8.70e-7 (nf1), 6.8e-8 (cepstrum) on an MI355X, as the float64 restatement does on the CPU: printed
    here, held to the float64 restatement in test_parity_with_the_restatement, and its labels held to sklearn's here."""
    d = sets[name]
    lab = d["labels"]
    _pn, rows, c0, c1, gamma = d["problems"][0]
    res, coef, dec = d["trainer"].problems([(rows, c0, c1, gamma)], lab, eps=EPS, q_float32=True)
    coef, dec = coef.cpu().numpy()[0], dec.cpu().numpy()[0]
    allow = 4 * R.SPREAD_Q32[name]
    want = -d["decision_function"]
    err, rho = np.abs(dec - want).max(), abs(res[0]["rho"] + d["intercept"])
    ref = R.solve(d["d2"], lab, rows, c0, c1, gamma, EPS, qfloat32=True)
    err_ref, rho_ref = np.abs(dec - R.decisions(d["d2"], ref, gamma)).max(), abs(res[0]["rho"] - ref["rho"])
    print(f"{name}: q_float32 |dec - sklearn| {err:.3e}, |rho - sklearn| {rho:.3e}, |dec - ref| {err_ref:.3e}, allowance {allow:.3e}; "
          f"float64 |dec - sklearn| {np.abs(d['dec'][0] - want).max():.3e}")
    assert res[0]["status"] == dl.SVM_TRAIN_CONVERGED and res[0]["gap"] < EPS
    assert err <= allow and rho <= allow and err_ref <= allow and rho_ref <= allow
    alpha = coef * np.where(lab == 0, 1.0, -1.0)
    assert np.all(alpha >= 0) and np.all(alpha <= np.where(lab == 0, c0, c1)) and abs(coef.sum()) <= 1e-12 * np.where(lab == 0, c0, c1).sum()
    assert R.violation_gap(d["d2"], lab, rows, coef, c0, c1, gamma, qfloat32=True) <= EPS + 1e-9
    assert np.array_equal(np.where(dec > 0, 0, 1), d["predict"]) and np.array_equal(np.where(d["dec"][0] > 0, 0, 1), d["predict"])


def _bits(res, coef, dec, k):
    return res[k:k + 1].tobytes(), coef[k].cpu().numpy().tobytes(), dec[k].cpu().numpy().tobytes()


def test_bit_identity(sets):
    """a problem's coef, dec and result are the same bits alone, among 200 others, reordered, and from a trainer whose workspace has
    grown from a smaller dataset"""
    d = sets["nf3"]
    n = d["labels"].size
    t = d["trainer"]
    mine = d["problems"][4][1:]                                        # first65
    others = [(np.arange(k % 7, 20 + k, dtype=np.int32), 1.0 + k, 2.0, 0.05 * (k % 9)) for k in range(200)]
    alone = _bits(*t.problems([mine], d["labels"], eps=EPS), 0)
    assert alone == _bits(d["res"], _cuda(d["coef"]), _cuda(d["dec"]), 4)
    assert alone == _bits(*t.problems(others[:77] + [mine] + others[77:], d["labels"], eps=EPS), 77)
    assert alone == _bits(*t.problems([mine] + others[::-1], d["labels"], eps=EPS), 0)
    grown = sj.SvmTrainer(3)
    grown.set(d["feat"][:40].contiguous())
    grown.problems([(np.arange(40, dtype=np.int32), 1.0, 1.0, 0.3)], d["labels"][:40])
    grown.set(d["feat"], offset=d["offset"], scale=d["scale"])
    assert alone == _bits(*grown.problems(others[:3] + [mine], d["labels"], eps=EPS), 3)
    grown.close()
    assert n == 300


@pytest.mark.parametrize("name", SETS)
def test_platt(sets, name):
    """A, B against the restatement's sigmoid_train on the device's own held-out decisions within 1e-9 relative (only the order of the
    sums differs), and the same bits on a second run"""
    import torch
    d = sets[name]
    lab, n = d["labels"], d["labels"].size
    ids = sj.svm_folds(n, 5, 3)
    rows = np.arange(n, dtype=np.int32)
    t = d["trainer"]
    _res, _coef, dec = t.problems([(rows[ids != f], d["c"][0], d["c"][1], d["gamma"]) for f in range(5)], lab, eps=EPS)
    dec_cv = dec[_cuda(ids.astype(np.int64)), torch.arange(n, device=dec.device)].contiguous()
    a, b, it = t.platt(dec_cv, lab)
    want_a, want_b, want_it = R.sigmoid_train(dec_cv.cpu().numpy(), lab)
    print(f"{name}: A {a!r} B {b!r} after {it} steps; restatement {want_a!r} {want_b!r} after {want_it}")
    assert abs(a - want_a) <= 1e-9 * abs(want_a) and abs(b - want_b) <= 1e-9 * abs(want_b) and it == want_it
    assert t.platt(dec_cv, lab) == (a, b, it)
    half = rows[::2].copy()
    a2, b2, _ = t.platt(dec_cv, lab, half)
    want = R.sigmoid_train(dec_cv.cpu().numpy()[half], lab[half])
    assert abs(a2 - want[0]) <= 1e-9 * abs(want[0]) and abs(b2 - want[1]) <= 1e-9 * abs(want[1])


@pytest.mark.parametrize("name", SETS)
def test_fit_end_to_end(sets, name):
    """dsp_svm_fit_device: the returned model through SvmModel.predict labels the training rows as sklearn's fitted SVC does, rows
    whose |dec| is inside SvmRef's bound left out (at most 1 %; none on the CPU: test_restatement_spread), its float32 decision within
    that bound of the float64 decision of the same model, and the model agrees with the restated fit"""
    d = sets[name]
    c = 10.0 if name != "nf1" else 1.0
    t = sj.SvmTrainer(d["x"].shape[1])
    attrs, report = t.fit(d["feat"], d["labels"], C=c, gamma=d["gamma"], eps=EPS)
    want, parts = R.fit(d["x"], d["labels"], c=c, gamma=d["gamma"], eps=EPS)
    assert report["status"] == "converged" and report["gap"] < EPS and report["C"] == pytest.approx(tuple(d["c"]), rel=1e-15)
    for k in ("offset", "scale"):
        assert np.all(np.abs(attrs[k] - want[k]) <= np.spacing(np.abs(want[k])))
    model = sj.SvmModel(attrs)
    label, dec32, _p1 = model.predict(d["feat"])
    ref = S.SvmRef(attrs)
    ref_label, dec64, bound, _ = ref.predict(d["x"])
    assert np.all(np.abs(dec32.cpu().numpy() - dec64) <= bound)
    near = np.abs(dec64) < bound
    assert near.sum() <= 0.01 * near.size and np.array_equal(label.cpu().numpy()[~near], d["predict"][~near])
    allow = 4 * R.SPREAD[name] + 2 * bound.max()                      # (+ the model's float32 coef, rho and Scaler ulps, which SvmRef's bound covers)
    assert np.abs(dec64 - R.decisions(parts["d2"], parts["final"], parts["gamma"])).max() <= allow
    assert abs(float(attrs["prob_a"][0]) - float(want["prob_a"][0])) <= 1e-4 and abs(float(attrs["prob_b"][0]) - float(want["prob_b"][0])) <= 1e-4
    assert attrs["sv"].shape[0] == attrs["coef"].size == report["n_sv"] == int(attrs["vectors_per_class"].sum())
    # gamma="scale", the default, is sklearn's; and the fit with libsvm's rounding of Q labels the rows as sklearn does, too
    attrs2, report2 = t.fit(d["feat"], d["labels"], C=c, q_float32=True)
    assert report2["gamma"] == pytest.approx(d["gamma"], rel=1e-6) and report2["status"] == "converged"
    model2 = sj.SvmModel(attrs2)
    assert np.array_equal(model2.predict(d["feat"])[0].cpu().numpy(), d["predict"])
    model2.close()
    model.close()
    t.close()


def test_round_trip_through_scrubjay(sets):
    """features of the reference's own training clips -> ScrubJay.train -> its SVM labels them as sklearn's fit does"""
    d = sets["cepstrum"]
    jay, report = sj.ScrubJay.train(d["feat"], d["labels"], eps=EPS)
    label, _dec, p1 = jay.svm.predict(d["feat"])
    assert report["status"] == "converged" and np.array_equal(label.cpu().numpy(), d["predict"])
    assert np.all(np.isfinite(p1.cpu().numpy()))


def test_cross_validate(sets):
    """each outer fold's held-out decisions over the grid against per-fold restated fits, and the scores from them"""
    d = sets["nf3"]
    lab = d["labels"]
    ids = sj.svm_folds(lab.size, R.CV_FOLDS, R.CV_SEED)
    t = sj.SvmTrainer(3)
    got = t.cross_validate(d["feat"], lab, ids, *R.CV_GRID, eps=EPS)
    t.close()
    want = R.cv_reference(d["x"], lab, ids, *R.CV_GRID, EPS)
    err = np.abs(got["dec"].cpu().numpy() - want).max()
    print(f"cross_validate: |dec - ref| {err:.3e}, allowance {4 * R.SPREAD['cv']:.3e}")
    assert err <= 4 * R.SPREAD["cv"] and np.all(got["status"] == dl.SVM_TRAIN_CONVERGED) and len(got["grid"]) == 4
    pred = want <= 0
    tp = (pred & (lab == 1)).sum(axis=1)
    assert np.allclose(got["precision"].cpu().numpy(), tp / np.maximum(pred.sum(axis=1), 1), rtol=1e-12)
    assert np.allclose(got["recall"].cpu().numpy(), tp / (lab == 1).sum(), rtol=1e-12)
    assert np.all(got["f1"].cpu().numpy() > 0.5)


def test_status_words(sets):
    """rows of one label, no rows and a problem stopped at max_iter are reported in the status word, and their neighbours in the launch
    are the same bits as without them"""
    d = sets["nf3"]
    lab, t = d["labels"], d["trainer"]
    rows = np.arange(lab.size, dtype=np.int32)
    two, bounded, everything = d["problems"][1][1:], d["problems"][8][1:], d["problems"][0][1:]
    only0, only1 = (rows[lab == 0][:9], 1.0, 1.0, 0.3), (rows[lab == 1][:1], 1.0, 1.0, 0.3)
    empty = (np.zeros(0, np.int32), 1.0, 1.0, 0.3)
    res, coef, dec = t.problems([two, only0, empty, bounded, only1, everything], lab, eps=EPS, max_iter=50)
    assert list(res["status"]) == [dl.SVM_TRAIN_CONVERGED, dl.SVM_TRAIN_ONE_CLASS, dl.SVM_TRAIN_EMPTY, dl.SVM_TRAIN_CONVERGED, dl.SVM_TRAIN_ONE_CLASS,
                                   dl.SVM_TRAIN_MAX_ITER]
    coef_h, dec_h = coef.cpu().numpy(), dec.cpu().numpy()
    assert np.all(coef_h[[1, 2, 4]] == 0.0) and np.all(dec_h[1] == 1.0) and np.all(dec_h[2] == 0.0) and np.all(dec_h[4] == -1.0)
    for k in (1, 2, 4):
        assert res[k]["n_iter"] == res[k]["n_sv"] == 0 and res[k]["rho"] == 0.0
    for k, suite in ((0, 1), (3, 8)):
        assert _bits(res, coef, dec, k) == _bits(d["res"], _cuda(d["coef"]), _cuda(d["dec"]), suite)
    stopped = res[5]
    alpha = coef_h[5] * np.where(lab == 0, 1.0, -1.0)
    assert stopped["n_iter"] == 50 and stopped["gap"] >= EPS and np.all(alpha >= 0) and np.all(alpha <= np.where(lab == 0, *d["c"]))
    assert abs(stopped["gap"] - R.violation_gap(d["d2"], lab, rows, coef_h[5], d["c"][0], d["c"][1], d["gamma"])) <= 1e-9


def test_a_problem_above_48_kb_of_lds():
    """2 900 members take the solver's LDS past 48 KB, where the launch asks for the larger allocation: the solution is feasible and
    optimal by the violation recomputed in float64"""
    rng = np.random.default_rng(2900)
    n = 2900
    lab = (np.arange(n) % 3 == 0).astype(np.int32)
    x = (rng.standard_normal((n, 3)) + 2.5 * lab[:, None]).astype(np.float32)
    t = sj.SvmTrainer(3)
    off, scl = t.set(_cuda(x))
    rows = np.arange(n, dtype=np.int32)
    res, coef, _ = t.problems([(rows, 1.0, 2.0, 0.5)], lab, eps=1e-3, decisions=False)
    t.close()
    coef = coef.cpu().numpy()[0]
    alpha = coef * np.where(lab == 0, 1.0, -1.0)
    d2 = R.distances(R.standardise(x, off, scl))
    gap = R.violation_gap(d2, lab, rows, coef, 1.0, 2.0, 0.5)
    print(f"n = {n}: {res[0]['n_iter']} steps, gap {res[0]['gap']:.3e} reported, {gap:.3e} recomputed")
    assert res[0]["status"] == dl.SVM_TRAIN_CONVERGED and res[0]["gap"] < 1e-3 and gap <= 1e-3 + 1e-9
    assert np.all(alpha >= 0) and np.all(alpha <= np.where(lab == 0, 1.0, 2.0)) and abs(coef.sum()) <= 1e-12 * np.where(lab == 0, 1.0, 2.0).sum()
