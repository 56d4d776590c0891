#!/usr/bin/env python3
"""Writes tests/golden/ubm_train_ref.npz: the UBM training fixture of tests/test_ubm_cpu.py and tests/test_gpu_ubm.py.

    python tests/golden/make_golden_ubm.py

The rows are drawn here from the reference's float UBM (ubm_*_d of speaker_enroll_ref.npz; tests/ubm_ref.py draw_population) and stored
as int16 at 1 / 4096, so that float32 holds them exactly.  The start is the library's deterministic one (tests/ubm_ref.py init_rows, in
float64).  The answers are sklearn's own: GaussianMixture(n_components=32, covariance_type="diag", reg_covar=1e-6, weights_init,
means_init, precisions_init) for max_iter 1 and 10 at tol = 0 and for a run that stops on tol = 1e-3.  Needs scikit-learn; the tests
read the file and never import it."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import ubm_ref as U  # noqa: E402

N_ROWS, K, REG = 6000, 32, 1e-6
RUNS = {"iter1": dict(max_iter=1, tol=0.0), "iter10": dict(max_iter=10, tol=0.0), "tol": dict(max_iter=300, tol=1e-3)}


def main():
    from sklearn.mixture import GaussianMixture
    z = np.load(os.path.join(HERE, "speaker_enroll_ref.npz"))
    ubm = {key: z[f"ubm_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
    rng = np.random.default_rng(20261017)
    rows_q = np.clip(np.rint(U.draw_population(rng, ubm, N_ROWS).astype(np.float64) * 4096.0), -32767, 32767).astype(np.int16)
    x = rows_q.astype(np.float32) / np.float32(4096.0)
    assert np.array_equal(x.astype(np.float64) * 4096.0, rows_q)
    init = U.init_rows(x, K, REG)
    out = {"rows_q": rows_q, "reg_covar": np.float64(REG)}
    out.update({f"init_{key}": v for key, v in init.items()})
    for tag, kw in RUNS.items():
        gm = GaussianMixture(n_components=K, covariance_type="diag", reg_covar=REG, weights_init=init["weights"], means_init=init["means"],
                             precisions_init=1.0 / init["variances"], **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                      # (tol = 0 never converges: sklearn says so)
            gm.fit(x.astype(np.float64))
        sk = {"weights": gm.weights_, "means": gm.means_, "variances": gm.covariances_, "lower_bound": np.float64(gm.lower_bound_),
              "n_iter": np.int64(gm.n_iter_), "converged": np.bool_(gm.converged_), "max_iter": np.int64(kw["max_iter"]), "tol": np.float64(kw["tol"])}
        out.update({f"{tag}__{key}": v for key, v in sk.items()})
        want = U.fit(x, init, reg_covar=REG, **kw)
        model = U.fit(x, init, reg_covar=REG, dtype=np.float32, **kw)
        rel = float((np.abs(want["variances"] - sk["variances"]) / sk["variances"]).max())
        print(f"{tag}: n_iter {int(gm.n_iter_)} converged {bool(gm.converged_)} lower bound {gm.lower_bound_:.9f}; restatement vs sklearn: weights "
              f"{np.abs(want['weights'] - sk['weights']).max():.1e}, means {np.abs(want['means'] - sk['means']).max():.1e}, variances (rel) {rel:.1e}, "
              f"lower bound {abs(want['lower_bounds'][-1] - sk['lower_bound']):.1e}, n_iter {want['n_iter']}")
        if want["n_iter"] == model["n_iter"]:
            print(f"{tag}: float32 model vs float64: " + ", ".join(f"{key} {v:.2e}" for key, v in U.deviations(model, want).items()))
        else:
            print(f"{tag}: the float32 model stops after {model['n_iter']} iterations")
    path = os.path.join(HERE, "ubm_train_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
