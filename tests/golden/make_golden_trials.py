#!/usr/bin/env python3
"""Writes tests/golden/gmm_trials_ref.npz: the reference's recorded trial list and what its own lines make of it.

    python tests/golden/make_golden_trials.py            (DSP_REF: the reference checkout, default /root/reference)

Data only: the `llr` and `label` columns of 2fa/audio/results/gmm_results.csv (92 trials: 36 target, 56 non-target).  The answers are
those of the literal reference lines on the scores the library sees, the float32-rounded llr widened back to float64:
  evaluate_gmm.py:77-81      thresholds = np.linspace(min(llrs), max(llrs), 200); accs = [np.mean((llrs > t) == labels) ...];
                             best_t = thresholds[np.argmax(accs)] -> best_t, best_index, best_correct (85 of 92)
  generate_charts.py:68-69   roc_curve(labels, llrs), auc(fpr, tpr) -> fpr, tpr, roc_thresholds, auc; and roc_curve with
                             drop_intermediate=False -> fpr_all, tpr_all, roc_thresholds_all
sklearn and numpy only; nothing of tests/trials_ref.py goes into the file."""
import csv
import os

import numpy as np
from sklearn.metrics import auc, roc_curve

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DSP_REF", "/root/reference")


def main():
    with open(os.path.join(REF, "2fa", "audio", "results", "gmm_results.csv"), newline="") as f:
        rows = list(csv.DictReader(f))
    llr = np.array([float(r["llr"]) for r in rows], np.float64)
    label = np.array([int(r["label"]) for r in rows], np.int32)
    assert llr.size == 92 and int(label.sum()) == 36
    llrs, labels = llr.astype(np.float32).astype(np.float64), label
    thresholds = np.linspace(min(llrs), max(llrs), 200)
    accs = [np.mean((llrs > t) == labels) for t in thresholds]
    best_index = int(np.argmax(accs))
    best_t = thresholds[best_index]
    best_correct = int(round(max(accs) * llrs.size))
    fpr, tpr, thr = roc_curve(labels, llrs)
    fpr_all, tpr_all, thr_all = roc_curve(labels, llrs, drop_intermediate=False)
    area = auc(fpr, tpr)
    print(f"best_t {best_t!r} at index {best_index}, {best_correct} of {llrs.size} correct; auc {area!r}; {thr_all.size} points")
    assert best_correct == 85 and abs(best_t - 0.24) < 0.005 and abs(area - auc(fpr_all, tpr_all)) < 1e-15
    path = os.path.join(HERE, "gmm_trials_ref.npz")
    np.savez_compressed(path, llr=llr, label=label, best_t=best_t, best_index=best_index, best_correct=best_correct, fpr=fpr, tpr=tpr,
                        roc_thresholds=thr, fpr_all=fpr_all, tpr_all=tpr_all, roc_thresholds_all=thr_all, auc=area)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 8192


if __name__ == "__main__":
    main()
