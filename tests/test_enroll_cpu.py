"""CPU: sliding CMVN and MAP enrolment (include/dsp_amd.h dsp_cmvn_*, dsp_speaker_enroll*) -- the numpy restatement of their definitions
(tests/enroll_ref.py) against sklearn's GaussianMixture and against a literal per-row CMVN loop, the pinned fixture
(tests/golden/speaker_enroll_ref.npz) against the restatement, the exports, and the argument checks the entries make before they touch
a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from dsp_amd import lib as dl
from tests import enroll_ref as E
from tests.enroll_util import MODES, ROOT, build_main_enroll, fixture

ENROLL_SYMBOLS = ["dsp_cmvn_create", "dsp_cmvn_destroy", "dsp_cmvn_ragged_device",
                  "dsp_speaker_enroller_create", "dsp_speaker_enroller_destroy", "dsp_speaker_enroll_ragged_device"]


def test_fixture_holds_the_reference_gmms_and_its_own_preconditions(golden):
    z, ubm, feats = fixture(golden)
    assert ubm["means"].shape == (32, 13) and ubm["means"].dtype == np.float64
    assert abs(E.weights_of(ubm).sum() - 1.0) < 1e-6
    assert np.array_equal(z["target_log_consts_d"], z["ubm_log_consts_d"]) and np.array_equal(z["target_inv_covs_d"], z["ubm_inv_covs_d"])
    assert not np.array_equal(z["target_means_d"], z["ubm_means_d"])
    assert np.abs(ubm["means"]).max() < 2.0 and np.isclose((1.0 / ubm["inv_covs"]).min(), 1e-6)
    assert np.diff(z["frame_offsets"]).tolist() == [1, 2, 64, 97, 150, 299, 300, 301, 700, 1025, 1500, 4097]
    assert feats.shape == (int(z["frame_offsets"][-1]), 13) and feats.dtype == np.float32
    assert np.all(feats[0] == 0.0)                                           # the one-row speaker
    # the Q6 image of the double means is the firmware's int8 table (speaker_gmm_ref.npz): the format enrolment writes
    s = golden("speaker_gmm_ref.npz")
    for who in ("ubm", "target"):
        mq, sat = E.q6(z[f"{who}_means_d"][None])
        assert np.abs(mq[0].astype(int) - s[f"{who}_means"].astype(int)).max() <= 1 and int(sat[0]) == 0


@pytest.mark.parametrize("tag", list(MODES))
def test_fixture_expectations_are_the_restatements(golden, tag):
    z, ubm, feats = fixture(golden)
    got = E.enroll_ragged(feats, z["frame_offsets"], ubm, **MODES[tag])
    for key in ("means", "counts", "ll_mean"):
        assert np.abs(got[key] - z[f"{tag}__{key}"]).max() <= 1e-9, key
    assert np.array_equal(got["means_q6"], z[f"{tag}__means_q6"]) and np.array_equal(got["saturated"], z[f"{tag}__saturated"])
    model = E.enroll_ragged(feats, z["frame_offsets"], ubm, dtype=np.float32, **MODES[tag])
    dev = float(np.abs(model["means"].astype(np.float64) - got["means"]).max())
    ties = E.tie_zone(got["means"], E.GATE_FACTOR * dev)
    print(f"{tag}: float32 model vs float64 means {dev:.2e}, tie zone {ties.mean():.3%}, saturated {got['saturated'].tolist()}")
    assert ties.mean() < 0.01
    assert np.array_equal(model["means_q6"][~ties], got["means_q6"][~ties])
    assert np.allclose(got["counts"].sum(axis=1), np.diff(z["frame_offsets"]), rtol=1e-12)


def test_restatement_is_sklearns_gaussian_mixture(golden):
    """An independent pin: predict_proba / score_samples of a diagonal GaussianMixture given the fixture's weights, means, covariances and
    precisions_cholesky_ = sqrt(inv_covs), and both reference scripts' map_adapt_gmm written with its posteriors.  Float64 against
    float64: rounding only.  Measured here with sklearn 1.7.2: 5e-15 (posteriors), 1.4e-14 (log-likelihoods), 9e-15 (means); the bounds below are 1e-12 and 1e-11."""
    GaussianMixture = pytest.importorskip("sklearn.mixture").GaussianMixture
    z, ubm, feats = fixture(golden)
    gm = GaussianMixture(n_components=32, covariance_type="diag")
    gm.weights_, gm.means_, gm.covariances_ = E.weights_of(ubm), ubm["means"], 1.0 / ubm["inv_covs"]
    gm.precisions_cholesky_ = np.sqrt(ubm["inv_covs"])
    fo = z["frame_offsets"]
    worst = {"p": 0.0, "ll": 0.0, "means": 0.0}
    for s in (1, 3, 8, 11):
        x = feats[fo[s]:fo[s + 1]].astype(np.float64)
        p, ll = E.posteriors(x, ubm)
        post = gm.predict_proba(x)
        worst["p"] = max(worst["p"], float(np.abs(p - post).max()))
        worst["ll"] = max(worst["ll"], float(np.abs(ll - gm.score_samples(x)).max()))
        n_k, f_k = post.sum(0) + 1e-8, post.T @ x                                  # adapt_ubm.py, both scripts
        for kw, alpha in ((MODES["relevance"], (n_k / (n_k + 16.0))[:, None]), (MODES["fixed"], 0.7)):
            want = alpha * (f_k / n_k[:, None]) + (1 - alpha) * gm.means_
            got = E.enroll(x, ubm, **kw)
            worst["means"] = max(worst["means"], float(np.abs(got["means"] - want).max()))
            assert abs(got["ll_mean"] - gm.score(x)) <= 1e-11
            assert np.abs(got["counts"] + 1e-8 - n_k).max() <= 1e-10
    print("restatement vs sklearn:", worst)
    assert worst["p"] <= 1e-12 and worst["ll"] <= 1e-11 and worst["means"] <= 1e-11


def _cmvn_literal(x, window):
    """sliding_cmvn as the reference writes it: one row at a time, numpy's own mean and std"""
    n, half = x.shape[0], window // 2
    y = np.zeros_like(x)
    for t in range(n):
        seg = x[max(0, t - half):min(n, t + half)]
        y[t] = (x[t] - seg.mean(axis=0)) / (seg.std(axis=0) + 1e-8)
    return y


@pytest.mark.parametrize("window", [2, 3, 10, 300])
def test_restatements_cmvn_on_the_edge_lengths(window):
    half = window // 2
    rng = np.random.default_rng(window)
    for n in sorted({1, 2, half, half + 1, window - 1, window, window + 1}):
        x = rng.normal(0.0, 30.0, (n, 5)) + np.array([-400.0, 60.0, 0.0, 5.0, -20.0])
        got, want = E.cmvn(x, window), _cmvn_literal(x, window)
        assert np.abs(got - want).max() <= 1e-9, (window, n)
        if n == 1:
            assert np.all(got == 0.0)
    # the window is asymmetric: row t reads t - half .. t + half - 1, and nothing of the next recording
    x = rng.normal(0.0, 1.0, (3 * window + 7, 2))
    y = E.cmvn_ragged(x, [0, window + 3, window + 3, 3 * window + 7], window)
    assert np.array_equal(y[:window + 3], E.cmvn(x[:window + 3], window)) and np.array_equal(y[window + 3:], E.cmvn(x[window + 3:], window))
    t = window + 1
    moved = x[window + 3:].copy()
    moved[t + half] += 100.0                                                     # one past the window's last row
    assert np.array_equal(E.cmvn(moved, window)[t], y[window + 3 + t])
    moved[t + half - 1] += 100.0                                                 # the window's last row
    assert not np.array_equal(E.cmvn(moved, window)[t], y[window + 3 + t])
    assert np.all(E.cmvn(np.zeros((40, 3)), window) == 0.0) and np.all(E.cmvn(np.zeros((40, 3), np.float32), window, np.float32) == 0.0)


def test_enroll_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in ENROLL_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_cmvn") or n.startswith("dsp_speaker_enroll")) == sorted(ENROLL_SYMBOLS)
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "enroll_kernels.hpp")) as f:
        hpp = f.read()
    for name, value in (("kEnrollChunkRows", E.CHUNK_ROWS), ("kCmvnTileRows", E.CMVN_TILE_ROWS), ("kCmvnMaxWindow", E.CMVN_MAX_WINDOW)):
        assert re.search(r"constexpr int " + name + r" = " + str(value) + r";", hpp), name


def _einval(rc):
    assert rc == -1 and dl.last_error() != "", (rc, dl.last_error())


def test_bad_arguments_are_einval_before_any_device_work():
    L = dl.load()
    h = C.c_void_p()
    for d, window in ((0, 300), (17, 300), (13, 1), (13, 0), (13, -4), (13, E.CMVN_MAX_WINDOW + 1)):
        _einval(L.dsp_cmvn_create(0, d, window, C.byref(h)))
        assert not h.value
    assert str(E.CMVN_MAX_WINDOW) in dl.last_error()                             # the refusal names the limit
    _einval(L.dsp_cmvn_create(0, 13, 300, None))
    off = (C.c_long * 2)(0, 4)
    _einval(L.dsp_cmvn_ragged_device(None, None, 1, off, None, None))
    arr = np.zeros(65 * 17)
    for k, d in ((65, 13), (0, 13), (32, 17), (32, 0)):
        p = dl.GmmFloatParams(k, d, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)
        _einval(L.dsp_speaker_enroller_create(C.byref(p), 0, C.byref(h)))
        assert not h.value and ("64" in dl.last_error() or "16" in dl.last_error())
    _einval(L.dsp_speaker_enroller_create(None, 0, C.byref(h)))
    _einval(L.dsp_speaker_enroller_create(C.byref(dl.GmmFloatParams(4, 4, None, arr.ctypes.data, arr.ctypes.data)), 0, C.byref(h)))
    bad = arr.copy()
    bad[3] = np.inf
    _einval(L.dsp_speaker_enroller_create(C.byref(dl.GmmFloatParams(4, 4, arr.ctypes.data, bad.ctypes.data, arr.ctypes.data)), 0, C.byref(h)))
    cfg = dl.EnrollConfig(dl.MAP_RELEVANCE, 16.0, 0.7)
    _einval(L.dsp_speaker_enroll_ragged_device(None, None, 1, off, C.byref(cfg), None, None, None, None, None, None))


def test_enroll_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
ubm = {"log_consts": np.zeros(4), "means": np.zeros((4, 3)), "inv_covs": np.ones((4, 3))}
for f, args in ((dsp_amd.Cmvn, (0,)), (dsp_amd.Cmvn, (17,)), (dsp_amd.Cmvn, (13, 1)),
                (dsp_amd.SpeakerEnroller, (dict(ubm, means=np.zeros(4)),)), (dsp_amd.SpeakerEnroller, (dict(ubm, log_consts=np.zeros(5)),)),
                (dsp_amd.SpeakerEnroller, ({k: np.zeros((65, 3)) if k != "log_consts" else np.zeros(65) for k in ubm},)),
                (dsp_amd.SpeakerEnroller.speaker_model, (np.zeros((4, 3), np.float32), {"means": np.zeros((4, 3), np.int8)})),
                (dsp_amd.SpeakerEnroller.speaker_model, (np.zeros((4, 2), np.int8), {"means": np.zeros((4, 3), np.int8)}))):
    try:
        f(*args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for {f.__name__}{args}")
c = object.__new__(dsp_amd.Cmvn)
c.d, c.window, c.device, c._h = 3, 300, 0, None
e = object.__new__(dsp_amd.SpeakerEnroller)
e.k, e.d, e.device, e._h = 4, 3, 0, None
x = torch.zeros(8, 3)
for call in (lambda: c.apply(x, [0, 8]), lambda: c.apply(np.zeros((8, 3), np.float32), [0, 8]), lambda: e.enroll(x, [0, 8]),
             lambda: e.enroll(x, [0, 8], mode="both"), lambda: e.enroll(x, [0, 8], relevance_factor=0.0),
             lambda: e.enroll(x, [0, 8], mode="fixed_alpha", fixed_alpha=1.5), lambda: e.enroll(x, [0, 8, 4]), lambda: e.enroll(x, [])):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for a bad enrolment argument")
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_example_main_enroll_links_and_refuses_bad_arguments(tmp_path):
    exe = build_main_enroll(str(tmp_path / "main_enroll"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, str(tmp_path / "missing.txt"), str(tmp_path / "missing.wav")], capture_output=True, text=True)
    assert r.returncode == 1 and "expected k d" in r.stderr
