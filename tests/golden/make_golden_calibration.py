#!/usr/bin/env python3
"""Writes tests/golden/gmm_calibration_ref.npz: sklearn's answer to the calibration fit on the reference's recorded trial list.

    python tests/golden/make_golden_calibration.py

Data only.  The trials are the 92 of tests/golden/gmm_trials_ref.npz (the `llr` and `label` columns of the reference's
2fa/audio/results/gmm_results.csv: 36 target, 56 non-target), the scores as the library sees them: the float32-rounded llr widened back
to float64.  The reference records no frame counts, so `n_frames` is seeded and synthetic, 50 .. 3000 rows per trial, and is stored as
data; l = np.log(n_frames + 1e-8).  The answers are those of
    LogisticRegression(penalty=None, tol=1e-12, max_iter=10000, class_weight={1: 0.5 * T / P, 0: 0.5 * T / N})
on (llr, l) -> theta3 = (coef_[0], intercept_, coef_[1]) and on (llr) alone -> theta2 = (coef_, intercept_): the prior-weighted objective
at prior 0.5, whose tau is 0.  lbfgs stops on its gradient, not on theta: the gap to the Newton restatement (tests/calibration_ref.py at
tol = 1e-12) is printed and stored as gap3 / gap2; the tests gate at 1e-6 per parameter.  Nothing of tests/calibration_ref.py goes
into the answers."""
import os
import sys

import numpy as np
from sklearn.linear_model import LogisticRegression

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import calibration_ref as R
    g = np.load(os.path.join(HERE, "gmm_trials_ref.npz"))
    llr, label = g["llr"], g["label"]
    assert llr.size == 92 and int(label.sum()) == 36
    x = llr.astype(np.float32).astype(np.float64)
    n_frames = np.random.default_rng(20261019).integers(50, 3001, llr.size).astype(np.int64)
    l = np.log(n_frames.astype(np.float64) + 1e-8)
    T, P = llr.size, int(label.sum())
    kw = dict(penalty=None, tol=1e-12, max_iter=10000, class_weight={1: 0.5 * T / P, 0: 0.5 * T / (T - P)})
    m3 = LogisticRegression(**kw).fit(np.stack([x, l], axis=1), label)
    m2 = LogisticRegression(**kw).fit(x[:, None], label)
    theta3 = np.array([m3.coef_[0, 0], m3.intercept_[0], m3.coef_[0, 1]])
    theta2 = np.array([m2.coef_[0, 0], m2.intercept_[0], 0.0])
    truth = np.where(label == 1, 0, -1)
    r3 = R.fit(x.astype(np.float32), truth, l, tol=1e-12)
    r2 = R.fit(x.astype(np.float32), truth, None, tol=1e-12)
    gap3 = float(np.abs(theta3 - [r3["a"], r3["b"], r3["c"]]).max())
    gap2 = float(np.abs(theta2 - [r2["a"], r2["b"], r2["c"]]).max())
    print(f"theta3 {theta3.tolist()} (Newton: {r3['n_iter']} passes, status {r3['status']}, gap {gap3:.3e})")
    print(f"theta2 {theta2.tolist()} (Newton: {r2['n_iter']} passes, status {r2['status']}, gap {gap2:.3e})")
    assert r3["status"] == r2["status"] == R.CONVERGED and gap3 < 1e-6 and gap2 < 1e-6
    path = os.path.join(HERE, "gmm_calibration_ref.npz")
    np.savez_compressed(path, llr=llr, label=label, n_frames=n_frames, theta3=theta3, theta2=theta2, gap3=gap3, gap2=gap2)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 8192


if __name__ == "__main__":
    main()
