"""CPU: the numpy SVM reference of tests/svm_ref.py against libsvm itself (tests/golden/svm_libsvm_ref.npz, and sklearn.svm._libsvm
on random models where sklearn is installed) and against the float32 C oracle, within the reference's own per-row bound B."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import svm_ref as R

# (nf, n_sv, gamma, balanced): the shapes the device paths take, small enough for the oracle's per-row calls
MODELS = [(1, 1, 0.5, True), (2, 63, 1e-4, True), (7, 65, 0.025, False), (26, 129, 1.0 / 26, True), (40, 55, 0.025, True),
          (64, 300, 1.0, True), (65, 2, 50.0, False), (256, 200, 0.0, True)]


def _oracle_model(a):
    m = {k: a[k] for k in ("offset", "scale", "sv", "coef")}
    m.update(gamma=float(a["kernel_params"][0]), rho=float(a["rho"][0]), prob_a=float(a["prob_a"][0]), prob_b=float(a["prob_b"][0]))
    return m


def _draw(i):
    nf, n_sv, gamma, bal = MODELS[i]
    rng = np.random.default_rng(700 + i)
    a = R.random_svm(rng, nf, n_sv, gamma, bal)
    return rng, a, R.probe_rows(rng, a)


def test_reproduces_libsvm_fixture(golden):
    m, r = golden("scrubjay_svm.npz"), golden("svm_libsvm_ref.npz")
    ref = R.SvmRef({k: m[k] for k in m.files})
    for feat, dec_l, proba, vote in ((r["feat"], r["decision"], r["proba"], r["label_vote"]),
                                     (r["labelled_feat"], r["labelled_decision"], r["labelled_proba"], r["labelled_vote"])):
        label, dec, bound, p1 = ref.predict(feat)
        assert np.all(np.abs(dec - dec_l) <= 1e-9 * np.maximum(1.0, np.abs(dec_l)))      # both float64 after the float32 Scaler
        assert np.all(bound < 5e-4) and np.all(bound > 0)                                # worst case: ~60x the typical error
        assert np.array_equal(label, vote)
        assert np.abs(p1 - proba[:, 1]).max() <= 1e-9


@pytest.mark.parametrize("i", range(len(MODELS)))
def test_oracle_within_bound(i):
    """the C oracle's float32 sequential sum lies within B (its order: n_sv terms in one chain); its tail equals the reference's
    on its own decision values, up to the iteration's stopping test"""
    _rng, a, x = _draw(i)
    ref = R.SvmRef(a)
    dec, _b = ref.decision(x)
    _d, bound = ref.decision(x, terms=ref.n_sv)
    far = R.far_rows(a, x)
    worst = 0.0
    for k in range(x.shape[0]):
        lab, odec, op1 = O.svm_predict(_oracle_model(a), x[k])
        err = abs(odec - dec[k])
        assert err <= bound[k], (k, odec, dec[k], bound[k])
        worst = max(worst, err / bound[k])
        assert lab == (0 if odec > 0 else 1)
        if far[k]:
            assert odec == float(np.float32(a["rho"][0]))
        outs, _flip = R.tail_outcomes(np.array([odec]), ref.prob_a, ref.prob_b)
        assert np.abs(outs[0] - op1).min() <= 2.5e-7
    assert worst < 1.0
    if ref.gamma > 0:
        assert far.any()
    kv = np.exp(-ref.gamma * ((ref.standardise(x[:1]).astype(np.float64) - ref.sv.astype(np.float64)) ** 2).sum(axis=1))
    assert kv.max() > 0.9                                         # the first probe row sits on SV 0


@pytest.mark.parametrize("i", range(len(MODELS)))
def test_sklearn_libsvm_random_models(i):
    pytest.importorskip("sklearn")
    from sklearn.svm import _libsvm
    from tools.pin_svm_libsvm import libsvm_model
    _rng, a, x = _draw(i)
    ref = R.SvmRef(a)
    label, dec, bound, p1 = ref.predict(x)
    m = {"sv": a["sv"], "coef": a["coef"], "vectors_per_class": a["vectors_per_class"], "rho": a["rho"], "prob_a": a["prob_a"],
         "prob_b": a["prob_b"], "kernel_params": a["kernel_params"]}
    kw = libsvm_model(m)
    z = np.ascontiguousarray(ref.standardise(x), np.float64)
    ldec = _libsvm.decision_function(z, **kw).reshape(-1)
    lproba = _libsvm.predict_proba(z, **kw)
    lvote = _libsvm.predict(z, **kw).astype(np.int64)
    assert np.all(np.abs(ldec - dec) <= bound)
    firm = np.abs(dec) > bound
    assert firm.sum() >= x.shape[0] // 2
    assert np.array_equal(lvote[firm], label[firm])
    outs, flip = R.tail_outcomes(dec, ref.prob_a, ref.prob_b)
    d = np.abs(lproba[:, 1] - p1)
    ok = (d <= 1e-6) | (flip & (np.abs(outs - lproba[:, 1:2]).min(axis=1) <= 1e-6))
    assert ok.all(), (np.nonzero(~ok)[0], d[~ok])


def test_tail_regimes():
    """the tail's edges: the vote at 0, the clamps, and the iteration's dead zone and stopping boundaries"""
    lab, p1 = R.tail(np.array([0.0, -0.0, 1e-30, -1e-30]), -1.0, 0.0)
    assert lab.tolist() == [1, 1, 0, 1] and np.all(p1 == 0.5)
    assert R.sigmoid_r01(np.array([200.0, -200.0]), 1.0, 0.0).tolist() == [R.R01_MIN, 1.0 - R.R01_MIN]
    b = R.stop_boundaries(n=100001)
    assert np.any(np.abs(b - 0.495) < 1e-9) and np.any(np.abs(b - 0.505) < 1e-9) and b.size >= 4
    p, s = R.multiclass_p1(np.array([0.4951, 0.5, 0.5049, 0.4949, 0.5051]))
    assert np.all(p[:3] == 0.5) and np.all(s[:3] == 0) and np.all(s[3:] == 1)
