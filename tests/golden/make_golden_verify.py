#!/usr/bin/env python3
"""Writes tests/golden/speaker_verify_ref.npz: sklearn's scores of the verification fixture of tests/test_verify_cpu.py and
tests/test_gpu_verify.py.

    python tests/golden/make_golden_verify.py

Inputs: the twelve clips and the float UBM of tests/golden/speaker_enroll_ref.npz (rows through tests/enroll_ref.py fixture_feats), and
as the twelve speakers that fixture's relevance__means rounded to float32.  Stored: GaussianMixture.score of the UBM per clip,
ubm_score [12], and of each target per clip, target_score [12 clips][12 speakers] -- a target model being the UBM's weights_ and
covariances_ with means_ replaced.  sklearn and numpy only; nothing of tests/verify_ref.py goes into the file (it is checked against
it here: the float64 restatement reproduces sklearn's UBM score of clip 0 to one unit in the last place -- 1.42e-14 at that score, 72.28,
the all-zero row under the component at the variance floor; against an 80-bit evaluation the restatement is the correctly rounded
value and sklearn 1.7.2 the neighbouring double)."""
import os
import sys

import numpy as np
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import enroll_ref as E  # noqa: E402
from tests import verify_ref as V  # noqa: E402


def mixture(ubm, means):
    gm = GaussianMixture(n_components=means.shape[0], covariance_type="diag")
    gm.weights_, gm.means_, gm.covariances_ = E.weights_of(ubm), np.asarray(means, np.float64), 1.0 / ubm["inv_covs"]
    gm.precisions_cholesky_ = np.sqrt(ubm["inv_covs"])
    return gm


def main():
    z = np.load(os.path.join(HERE, "speaker_enroll_ref.npz"))
    ubm = {key: z[f"ubm_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
    feats = E.fixture_feats(z).astype(np.float64)
    fo = z["frame_offsets"]
    speakers = z["relevance__means"].astype(np.float32)
    clips = [feats[fo[c]:fo[c + 1]] for c in range(fo.size - 1)]
    gm = mixture(ubm, ubm["means"])
    ubm_score = np.array([gm.score(x) for x in clips])
    target_score = np.array([[mixture(ubm, m).score(x) for m in speakers] for x in clips])
    L_u, _ = V.clip_sums(clips[0], ubm, speakers[:1])
    dev = abs(L_u / clips[0].shape[0] - ubm_score[0])
    print(f"float64 restatement vs sklearn, UBM score of clip 0 ({ubm_score[0]:.2f}): {dev:.2e}, one ulp {np.spacing(abs(ubm_score[0])):.2e}")
    assert dev <= np.spacing(abs(ubm_score[0]))
    path = os.path.join(HERE, "speaker_verify_ref.npz")
    np.savez_compressed(path, ubm_score=ubm_score, target_score=target_score)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 4096


if __name__ == "__main__":
    main()
