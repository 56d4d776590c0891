#!/usr/bin/env python3
"""sklearn's libsvm answers for the SVM trainer: seeded feature sets, and the reference's own training clips.

Runs only in the build container (needs sklearn; the `cepstrum` set also /root/reference).  Writes tests/golden/svmtrain.npz -- data only,
per set <name>:
    <name>__x        float32 [n][nf]  pooled features          <name>__labels   int32 [n]  0 / 1
    <name>__offset / __scale  float32 [nf]   the Scaler (tests/svmtrain_ref.py scaler_fit: float64 mean and 1 / population std)
    <name>__gamma    float64, a float32 value: sklearn's "scale" on z = fl32(fl32(x - offset) * scale)
    <name>__c        float64 [2]   the box bound of label 0, label 1 (class_weight="balanced" on C)
    SVC(kernel="rbf", C, gamma, class_weight="balanced", tol=1e-9).fit(z as float64, labels), as sklearn returns them:
    <name>__dual_coef, __support, __intercept, __decision_function (of all rows), __predict
sklearn's binary decision_function is -(libsvm's decision value): the trainer's dec = -decision_function, coef = -dual_coef, rho = -intercept.
Sets: nf40 (300 rows), nf3 (300 rows, 12 duplicated rows with the same label and 6 with the opposite one), nf1 (257 rows), and
cepstrum: the WAV files of cepstrum/data/{pos,neg} (the MP3s cannot be decoded offline), label 1 = pos as cepstrum/train.py:45 sets it,
features by tools/pin_svm_libsvm.py:librosa_like_features as tests/golden/make_golden_labelled_audio.py computes them."""
import glob
import importlib.util
import os
import sys

import numpy as np
from sklearn.svm import SVC

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("DSP_REF", "/root/reference")
sys.path.insert(0, ROOT)
from tests import svmtrain_ref as R  # noqa: E402


def synthetic(seed, n, nf, duplicates=0, flipped=0):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.4).astype(np.int32)
    labels[0], labels[1] = 0, 1
    shift = rng.standard_normal(nf)
    x = (rng.standard_normal((n, nf)) + labels[:, None] * shift) * rng.uniform(0.5, 5.0, nf) + rng.normal(0.0, 3.0, nf)
    for k in range(duplicates + flipped):                              # row n - 1 - k repeats row k, the last `flipped` with the other label
        x[n - 1 - k] = x[k]
        labels[n - 1 - k] = labels[k] if k < duplicates else 1 - labels[k]
    return x.astype(np.float32), labels


def golden(name, x, labels, c):
    offset, scale = R.scaler_fit(x)
    z = R.standardise(x, offset, scale).astype(np.float64)
    gamma = float(np.float32(1.0 / (x.shape[1] * z.var())))
    clf = SVC(kernel="rbf", C=c, gamma=gamma, class_weight="balanced", tol=1e-9).fit(z, labels)
    print(f"{name}: n {x.shape[0]}, nf {x.shape[1]}, gamma {gamma:.6g}, {clf.support_.size} SVs, max |dec| {np.abs(clf.decision_function(z)).max():.3f}")
    return {f"{name}__x": x, f"{name}__labels": labels, f"{name}__offset": offset, f"{name}__scale": scale, f"{name}__gamma": np.float64(gamma),
            f"{name}__c": np.array(R.balanced_weights(labels, c)), f"{name}__dual_coef": clf.dual_coef_[0], f"{name}__support": clf.support_.astype(np.int32),
            f"{name}__intercept": clf.intercept_[0], f"{name}__decision_function": clf.decision_function(z), f"{name}__predict": clf.predict(z).astype(np.int32)}


def cepstrum_clips():
    spec = importlib.util.spec_from_file_location("pin_svm", os.path.join(ROOT, "tools", "pin_svm_libsvm.py"))
    pin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pin)
    feats, labels = [], []
    for label, sub in ((1, "pos"), (0, "neg")):
        for path in sorted(glob.glob(os.path.join(REF, "cepstrum", "data", sub, "*"))):
            if not path.lower().endswith(".wav"):
                continue
            try:
                y, sr = pin.read_wav_mono(path)
            except Exception as e:  # noqa: BLE001  (a WAV flavour the reader does not take)
                print(f"skipped {os.path.basename(path)}: {e}")
                continue
            feats.append(pin.librosa_like_features(y, sr))
            labels.append(label)
            print(f"{sub}/{os.path.basename(path)}: {y.size} samples @ {sr} Hz")
    return np.asarray(feats, np.float32), np.asarray(labels, np.int32)


def main():
    out = {}
    out.update(golden("nf40", *synthetic(40, 300, 40), 10.0))
    out.update(golden("nf3", *synthetic(3, 300, 3, duplicates=12, flipped=6), 10.0))
    out.update(golden("nf1", *synthetic(1, 257, 1), 1.0))
    if os.path.isdir(os.path.join(REF, "cepstrum", "data")):
        x, labels = cepstrum_clips()
        if (labels == 0).any() and (labels == 1).any():
            out.update(golden("cepstrum", x, labels, 10.0))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "svmtrain.npz"), **out)
    print("wrote tests/golden/svmtrain.npz")


if __name__ == "__main__":
    sys.exit(main())
