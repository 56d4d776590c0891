#!/usr/bin/env python3
"""Writes tests/golden/kmeans_ref.npz: the k-means fixture of tests/test_kmeans_cpu.py and tests/test_gpu_kmeans.py.

    python tests/golden/make_golden_kmeans.py

Per case the rows are drawn here (a mixture of k Gaussians; d = 1: one Gaussian, on which Lloyd creeps and stops by tol) and stored as
int16 at 1 / 4096, so that float32 holds them exactly; the start is k rows of the data.  The answers are sklearn's own, computed in
float64 on those rows: KMeans(init=<the start>, n_init=1, algorithm="lloyd", tol=1e-4) centres, labels, n_iter_ and inertia_;
_estimate_gaussian_parameters of the one-hot labels (what GaussianMixture(init_params="kmeans") starts EM from); and for the case
"strict" GaussianMixture from that start after max_iter = 10 at tol = 0.  The seed of each case is the first at which, by the float64
restatement (tests/kmeans_ref.py): the stop is the one the case is named for, no cluster is ever empty, every row's relative label margin
against the float32-rounded centres is at least 16 x 2 (d + 3) 2^-24 at every iteration, and (tol) no shift lies within 1e-3 of the limit.
Needs scikit-learn; the tests read the file and never import it."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import kmeans_ref as K  # noqa: E402

CASES = {"strict": (1500, 8, 13, "strict"), "strict32": (1025, 32, 13, "strict"), "tol": (700, 5, 1, "tol")}
REG, TOL = 1e-6, 1e-4


def draw_case(n, k, d, seed):
    rng = np.random.default_rng(seed)
    if d == 1:
        x = rng.normal(0.0, 1.5, (n, 1))
    else:
        mu = rng.normal(0.0, 2.0, (k, d))
        x = mu[rng.integers(0, k, n)] + rng.normal(0.0, 0.7, (n, d))
    rows_q = np.clip(np.rint(x * 4096.0), -32767, 32767).astype(np.int16)
    return rows_q, np.sort(rng.choice(n, k, replace=False))


def conditions(x, ref, d, want_stop):
    if ref["stop"] != want_stop or ref["n_iter"] < 3 or ref["n_empty"]:
        return False
    limit = K.shift_limit(x, TOL)
    for centres, labels, _, shift in ref["trace"]:
        s32 = K.sq_dists(x, centres.astype(np.float32).astype(np.float64))
        if K.margins(s32).min() < 16.0 * K.rounding_bound(d) or np.bincount(labels, minlength=centres.shape[0]).min() == 0:
            return False
        if want_stop == "tol" and abs(shift - limit) <= 1e-3 * limit:
            return False
    s32 = K.sq_dists(x, ref["centres"].astype(np.float32).astype(np.float64))
    return K.margins(s32).min() >= 16.0 * K.rounding_bound(d)


def main():
    from sklearn.cluster import KMeans
    from sklearn.mixture import GaussianMixture
    from sklearn.mixture._gaussian_mixture import _estimate_gaussian_parameters
    out = {"reg_covar": np.float64(REG), "tol": np.float64(TOL)}
    for tag, (n, k, d, want_stop) in CASES.items():
        for seed in range(1, 200):
            rows_q, start = draw_case(n, k, d, 1000 * k + seed)
            x = rows_q.astype(np.float32) / np.float32(4096.0)
            assert np.array_equal(x.astype(np.float64) * 4096.0, rows_q)
            x64 = x.astype(np.float64)
            ref = K.lloyd(x, x64[start], 300, TOL, REG, history=True)
            if conditions(x, ref, d, want_stop):
                break
        else:
            raise SystemExit(f"{tag}: no seed meets the conditions")
        km = KMeans(n_clusters=k, init=x64[start], n_init=1, algorithm="lloyd", tol=TOL, max_iter=300).fit(x64)
        onehot = np.zeros((n, k))
        onehot[np.arange(n), km.labels_] = 1.0
        nk, means, covs = _estimate_gaussian_parameters(x64, onehot, REG, "diag")
        sk = {"rows_q": rows_q, "start": start.astype(np.int64), "centres": km.cluster_centers_, "labels": km.labels_.astype(np.int32), "n_iter": np.int64(km.n_iter_),
              "inertia": np.float64(km.inertia_), "stop": np.array(want_stop), "weights": nk / n, "means": means, "variances": covs}
        print(f"{tag}: seed {seed}, sklearn n_iter {km.n_iter_}, restatement n_iter {ref['n_iter']} stop {ref['stop']}; labels equal "
              f"{np.array_equal(ref['labels'], km.labels_)}, centres {np.abs(ref['centres'] - km.cluster_centers_).max():.1e}, inertia (rel) "
              f"{abs(ref['inertia'] / km.inertia_ - 1):.1e}, weights {np.abs(ref['weights'] - sk['weights']).max():.1e}, means "
              f"{np.abs(ref['means'] - means).max():.1e}, variances (rel) {np.abs(ref['variances'] / covs - 1).max():.1e}")
        if tag == "strict":
            gm = GaussianMixture(n_components=k, covariance_type="diag", reg_covar=REG, weights_init=sk["weights"], means_init=means, precisions_init=1.0 / covs,
                                 max_iter=10, tol=0.0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                gm.fit(x64)
            sk.update(em_weights=gm.weights_, em_means=gm.means_, em_variances=gm.covariances_, em_lower_bound=np.float64(gm.lower_bound_), em_n_iter=np.int64(gm.n_iter_))
        out.update({f"{tag}__{key}": v for key, v in sk.items()})
    path = os.path.join(HERE, "kmeans_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
