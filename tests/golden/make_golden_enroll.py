#!/usr/bin/env python3
"""Writes tests/golden/speaker_enroll_ref.npz: the reference's float GMMs and the enrolment fixture of tests/test_enroll_cpu.py and
tests/test_gpu_enroll.py.

    python tests/golden/make_golden_enroll.py [path to the reference checkout, default /root/reference]

From the reference only the DOUBLE_GMM parameter arrays of 2fa/audio/pico-audio/src/gmm_params.inc are taken (ubm_*_d, target_*_d: the
numbers its trainer wrote).  The fixture speakers are made here: rows of the clipN__mfcc matrices of speaker_gmm_ref.npz tiled to the
speaker's length, plus per-speaker noise (sigma 3 .. 14) and a per-speaker offset (sigma 10), quantised to 1 / 32 so that they fit int16
(raw_q).  What the library is given is their sliding CMVN at window 300 (tests/enroll_ref.py fixture_feats: float64, rounded to float32);
the expected outputs are the float64 restatement's on those rows, in both MAP modes."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import enroll_ref as E  # noqa: E402

LENGTHS = [1, 2, 64, 97, 150, 299, 300, 301, 700, 1025, 1500, 4097]
MODES = {"relevance": dict(mode="relevance", relevance_factor=16.0), "fixed": dict(mode="fixed_alpha", fixed_alpha=0.7)}


def parse_double_arrays(text):
    out = {}
    for name, body in re.findall(r"double\s+(\w+_d)\s*(?:\[\w+\])+\s*=\s*\{(.*?)\};", text, re.S):
        out[name] = np.array([float(v) for v in re.findall(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?", body)], np.float64)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with open(os.path.join(ref, "2fa/audio/pico-audio/src/gmm_params.inc")) as f:
        text = f.read()
    k, d = int(re.search(r"#define K (\d+)", text).group(1)), int(re.search(r"#define D (\d+)", text).group(1))
    arrays = parse_double_arrays(text)
    models = {}
    for who in ("ubm", "target"):
        models[who] = {"log_consts": arrays[f"{who}_log_consts_d"], "means": arrays[f"{who}_means_d"].reshape(k, d),
                       "inv_covs": arrays[f"{who}_inv_covs_d"].reshape(k, d)}
        assert models[who]["log_consts"].shape == (k,)
    ubm = models["ubm"]
    w = E.weights_of(ubm)
    assert abs(w.sum() - 1.0) < 1e-6, w.sum()                                    # the weights behind log_consts_d sum to 1
    assert np.array_equal(models["target"]["log_consts"], ubm["log_consts"]) and np.array_equal(models["target"]["inv_covs"], ubm["inv_covs"])
    assert np.isclose((1.0 / ubm["inv_covs"]).min(), 1e-6)                       # a component at the variance floor

    clips = np.load(os.path.join(HERE, "speaker_gmm_ref.npz"))
    rng = np.random.default_rng(20261017)
    raws = []
    for i, n in enumerate(LENGTHS):
        base = clips[f"clip{i % 4}__mfcc"].astype(np.float64)
        rows = np.tile(base, (n // base.shape[0] + 1, 1))[:n]
        sigma = 3.0 + 11.0 * i / (len(LENGTHS) - 1)
        rows = rows + rng.normal(0.0, sigma, rows.shape) + rng.normal(0.0, 10.0, (1, d))
        raws.append(np.clip(np.rint(rows * 32.0), -32767, 32767).astype(np.int16))
    fo = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    out = {"raw_q": np.concatenate(raws), "frame_offsets": fo}
    for who in models:
        for key, v in models[who].items():
            out[f"{who}_{key}_d"] = v
    feats = E.fixture_feats(out)
    for tag, kw in MODES.items():
        want = E.enroll_ragged(feats, fo, ubm, **kw)
        model = E.enroll_ragged(feats, fo, ubm, dtype=np.float32, **kw)
        dev = {key: float(np.abs(model[key].astype(np.float64) - want[key]).max()) for key in ("means", "ll_mean")}
        ties = E.tie_zone(want["means"], E.GATE_FACTOR * dev["means"])
        print(f"{tag}: float32 model vs float64: means {dev['means']:.2e}, ll_mean {dev['ll_mean']:.2e}; Q6 entries that differ "
              f"{int((model['means_q6'] != want['means_q6']).sum())} of {ties.size}, in the tie zone {ties.mean():.3%}; saturated {want['saturated'].tolist()}")
        assert ties.mean() < 0.01
        for key, v in want.items():
            out[f"{tag}__{key}"] = v
    cm = np.abs(E.cmvn_ragged(out["raw_q"].astype(np.float32) / np.float32(32.0), fo, 300, np.float32).astype(np.float64)
                - E.cmvn_ragged(out["raw_q"].astype(np.float64) / 32.0, fo, 300)).max()
    print(f"CMVN at window 300: float32 model vs float64 {cm:.2e}")
    path = os.path.join(HERE, "speaker_enroll_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
