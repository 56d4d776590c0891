#!/usr/bin/env python3
"""Timing of SVM training at the reference's dataset size and at a larger one:

    fit70     SvmTrainer.fit at n = 70, 40 features (cepstrum/train.py's dataset): Scaler, D2, 5 + 1 problems in one launch, Platt
    fit2000   the same at n = 2 000
    grid2000  a 5-fold x 8 x 8 (C, gamma) grid at n = 2 000: per outer fold one dataset and ONE launch of 64 problems of 1 600 members

    python tools/time_svmtrain.py [--only fit70|fit2000|grid2000] [--rounds 5] [--eps 1e-3] [--no-sklearn]

Features are normal variates, 40 % of the rows label 1 and shifted by one normal draw per feature, C = 10 balanced, gamma "scale"; the
grid is C = 0.1 .. 1000 and gamma = scale / 16 .. 8 scale in eight logarithmic steps each.  Times are medians over the rounds of the whole
call, host work and the wait included.  `resident_per_cu` is how many problems of the launch's largest size share a CU: the smaller of
what the solver's LDS (17 bytes per member + 176) leaves of 160 KiB and its 6 waves per SIMD of 77 VGPRs (tools/kernel_resources.py).
Where sklearn imports, the same work runs through sklearn's libsvm on 16 processes (joblib) as a baseline, not a gate.
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CS = [0.1 * 10 ** (4 * k / 7) for k in range(8)]
GAMMA_STEPS = [2.0 ** (k - 4) for k in range(8)]


def dataset(n, nf=40, seed=0):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.4).astype(np.int32)
    labels[:2] = 0, 1
    x = (rng.standard_normal((n, nf)) + labels[:, None] * rng.standard_normal(nf)) * rng.uniform(0.5, 5.0, nf) + rng.normal(0.0, 3.0, nf)
    return x.astype(np.float32), labels


def resident_per_cu(members):
    return int(min(6, (160 * 1024) // (17 * members + 176)))


def median_ms(fn, rounds):
    import torch
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out))


def sklearn_fit(x, labels, gamma, eps):
    from sklearn.svm import SVC
    t0 = time.perf_counter()
    SVC(kernel="rbf", probability=True, class_weight="balanced", C=10.0, gamma=gamma, tol=eps).fit(x, labels)
    return (time.perf_counter() - t0) * 1e3


def sklearn_grid(z_folds, labels, ids, scale_gamma, eps):
    from joblib import Parallel, delayed
    from sklearn.svm import SVC

    def one(z, train, c, gamma):
        clf = SVC(kernel="rbf", class_weight="balanced", C=c, gamma=gamma, tol=eps).fit(z[train], labels[train])
        return clf.decision_function(z)

    jobs = [(z_folds[f], np.nonzero(ids != f)[0], c, g * scale_gamma[f]) for f in range(len(z_folds)) for c in CS for g in GAMMA_STEPS]
    t0 = time.perf_counter()
    Parallel(n_jobs=16)(delayed(one)(*j) for j in jobs)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("fit70", "fit2000", "grid2000"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    import torch
    from dsp_amd import scrubjay as sj
    if not torch.cuda.is_available():
        raise SystemExit("time_svmtrain.py measures on a GPU: none found")
    try:
        import sklearn  # noqa: F401
        baseline = not args.no_sklearn
    except ImportError:
        baseline = False
    t = sj.SvmTrainer(40)
    for name in ([args.only] if args.only else ["fit70", "fit2000", "grid2000"]):
        n = 70 if name == "fit70" else 2000
        x, labels = dataset(n)
        feat = torch.from_numpy(x).cuda()
        line = {"shape": name, "rows": n, "features": 40, "eps": args.eps}
        if name != "grid2000":
            attrs, report = t.fit(feat, labels, eps=args.eps)                     # warm-up: code objects, the ring, the workspace
            med, low = median_ms(lambda: t.fit(feat, labels, eps=args.eps), args.rounds)
            members = n - n // 5
            line.update(fit_ms_median=round(med, 3), fit_ms_min=round(low, 3), problems=6, final_steps=report["n_iter"], n_sv=report["n_sv"],
                        status=report["status"], resident_per_cu=resident_per_cu(n), inner_resident_per_cu=resident_per_cu(members))
            if baseline:
                z = ((x - attrs["offset"]) * attrs["scale"]).astype(np.float64)
                line["sklearn_fit_ms"] = round(float(np.median([sklearn_fit(z, labels, report["gamma"], args.eps) for _ in range(3)])), 3)
        else:
            ids = sj.svm_folds(n, 5, 0)
            launch, steps, z_folds, scale_gamma = [], [], [], []
            for rnd in range(args.rounds + 1):                                    # (round 0 warms up)
                for f in range(5):
                    train = np.nonzero(ids != f)[0].astype(np.int32)
                    t.set(feat, scaler_rows=train)
                    z = t.rows()
                    g0 = 1.0 / (40 * float(z[train].astype(np.float64).var()))
                    c0, c1 = sj.svm_balanced_weights(labels, 1.0, train)
                    problems = [(train, c * c0, c * c1, g * g0) for c in CS for g in GAMMA_STEPS]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res, _coef, _dec = t.problems(problems, labels, eps=args.eps)
                    torch.cuda.synchronize()
                    if rnd:
                        launch.append((time.perf_counter() - t0) * 1e3)
                    else:
                        steps.append(res["n_iter"].copy())
                        z_folds.append(z.astype(np.float64))
                        scale_gamma.append(g0)
                        line["not_converged"] = line.get("not_converged", 0) + int((res["status"] != 0).sum())
            steps = np.concatenate(steps)
            line.update(launches=5, problems_per_launch=64, members=int((ids != 0).sum()), launch_ms_median=round(float(np.median(launch)), 3),
                        launch_ms_min=round(min(launch), 3), grid_ms=round(5 * float(np.median(launch)), 3), steps_median=int(np.median(steps)),
                        steps_max=int(steps.max()), steps_total=int(steps.sum()), resident_per_cu=resident_per_cu(int((ids != 0).sum())))
            if baseline:
                print(json.dumps(line), file=sys.stderr, flush=True)              # (the baseline takes far longer than what it is compared with)
                line["sklearn_grid_ms_16_processes"] = round(sklearn_grid(z_folds, labels, ids, scale_gamma, args.eps), 1)
        print(json.dumps(line), flush=True)
    t.close()


if __name__ == "__main__":
    main()
