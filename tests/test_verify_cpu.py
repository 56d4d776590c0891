"""CPU: float speaker verification (include/dsp_amd.h dsp_speaker_verif*) -- the numpy restatement of its definition (tests/verify_ref.py)
against sklearn's GaussianMixture.score (tests/golden/speaker_verify_ref.npz), what the float32 model of the GPU arithmetic deviates by,
the inputs of the GPU shape sweep (that `best` is decided on most clips by the restatement alone), the exports, and the argument checks
the entries make before they touch a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dsp_amd import lib as dl
from tests import verify_ref as V
from tests.enroll_util import ROOT
from tests.verify_util import SWEEP_KD, SWEEP_SPEAKERS, decided, fixture_case, subset, sweep_case

VERIFY_SYMBOLS = ["dsp_speaker_verifier_create", "dsp_speaker_verifier_destroy", "dsp_speaker_verify_ragged_device"]
LP = C.POINTER(C.c_long)


def test_restatement_is_sklearns_score_on_the_fixture(golden):
    case = fixture_case(golden)
    want, sk = case["want"], case["sklearn"]
    assert sk["ll_ubm"].shape == (12,) and sk["ll_target"].shape == (12, 12) and want["llr"].dtype == np.float64
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "speaker_verify_ref.npz")) < 4096
    err = {key: float(np.abs(want[key] - sk[key]).max()) for key in ("ll_ubm", "ll_target", "llr")}
    print("\nrestatement vs sklearn:", err)
    assert all(e <= 1e-11 for e in err.values()), err
    assert np.array_equal(want["best"], np.argmax(sk["llr"], axis=1))
    # the fixture's clips are noisy tilings of four recordings (clip i of recording i % 4): a clip of more than a handful of rows scores
    # highest against a speaker enrolled from its own recording
    assert np.array_equal(want["best"][2:] % 4, np.arange(2, 12) % 4)


def test_float32_model_deviation_on_the_fixture(golden):
    case = fixture_case(golden)
    want, model = case["want"], case["model"]
    assert model["llr"].dtype == np.float32 and model["best"].dtype == np.int32
    dev = {key: float(np.abs(model[key].astype(np.float64) - want[key]).max()) for key in ("llr", "ll_ubm", "ll_target", "best_llr")}
    gates = V.gates(want, model)
    print("\nfloat32 model vs float64:", {k: f"{v:.2e}" for k, v in dev.items()}, "gates", {k: f"{v:.2e}" for k, v in gates.items()},
          "ll_ubm range", float(want["ll_ubm"].min()), float(want["ll_ubm"].max()))
    assert all(0.0 < dev[key] < 1e-4 for key in dev)                             # float32 rounding of scores of tens, no more
    sure = decided(want["llr"], gates["llr"])
    assert sure.sum() * 2 >= sure.size and np.array_equal(model["best"][sure], want["best"][sure])


def test_row_tree_and_tiles_of_the_restatement():
    """the clip sum is the definition's: inside a tile ((a0 + a1) + (a2 + a3)) + ..., absent rows 0, then the tiles in ascending order"""
    rng = np.random.default_rng(3)
    ll = rng.normal(-20.0, 5.0, 64 * 2 + 5).astype(np.float32)

    def tree(v):
        v = list(v) + [0.0] * (64 - len(v))
        while len(v) > 1:
            v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
        return v[0]

    tiles = [tree(ll[i:i + 64].astype(np.float64)) for i in range(0, ll.size, 64)]
    assert V.clip_sum(ll) == (tiles[0] + tiles[1]) + tiles[2]
    assert V.clip_sum(ll[:1]) == float(ll[0]) and V.clip_sum(ll[:64]) == tiles[0]
    # a speaker whose centres are the UBM's has the UBM's sums exactly, in both arithmetics
    ubm = {"log_consts": np.log([0.3, 0.7]), "means": rng.normal(size=(2, 3)), "inv_covs": rng.uniform(0.5, 2.0, (2, 3))}
    x = rng.normal(size=(70, 3)).astype(np.float32)
    for dtype in (np.float64, np.float32):
        out = V.verify(x, [0, 70], ubm, ubm["means"][None].astype(dtype), dtype)
        assert out["llr"][0, 0] == 0.0 and out["ll_target"][0, 0] == out["ll_ubm"][0]


@pytest.mark.parametrize("k,d", SWEEP_KD)
def test_sweep_inputs_decide_best_by_the_restatement_alone(k, d):
    """the GPU shape sweep's inputs: for every speaker count the float64 runner-up is more than 2 gates below the maximum on at least
    half of the clips, and there the float32 model names the float64 argmax"""
    case = sweep_case(k, d)
    assert np.isclose((1.0 / case["ubm"]["inv_covs"]).min(), 1e-6)
    for n_spk in SWEEP_SPEAKERS:
        want, model = subset(case["want"], n_spk), subset(case["model"], n_spk)
        gates = V.gates(want, model)
        sure = decided(want["llr"], gates["llr"])
        print(f"\nk {k} d {d} S {n_spk}: llr gate {gates['llr']:.3e}, decided {int(sure.sum())} of {sure.size}")
        assert np.isfinite(want["llr"]).all() and np.isfinite(model["llr"]).all()
        assert sure.sum() * 2 >= sure.size, (k, d, n_spk)
        assert np.array_equal(model["best"][sure], want["best"][sure])


def test_verify_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in VERIFY_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_speaker_verif")) == sorted(VERIFY_SYMBOLS)
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "verify_kernels.hpp")) as f:
        hpp = f.read()
    for name, value in (("kVerifySpeakerTile", V.SPEAKER_TILE), ("kVerifyTileRows", V.TILE_ROWS)):
        assert re.search(r"constexpr int " + name + r" = " + str(value) + r";", hpp), name
    assert "a float log-sum-exp scorer" not in header


def _einval(rc, *words):
    assert rc == -1 and dl.last_error() != "" and all(w in dl.last_error() for w in words), (rc, dl.last_error())


def _verifier(L, k=4, d=3):
    arr = np.ones(k * d)
    h = C.c_void_p()
    p = dl.GmmFloatParams(k, d, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)
    assert L.dsp_speaker_verifier_create(C.byref(p), 0, C.byref(h)) == 0 and h.value, dl.last_error()      # no device is needed
    return h


def test_bad_arguments_are_einval_before_any_device_work():
    L = dl.load()
    h = C.c_void_p()
    arr = np.zeros(65 * 17)
    for k, d, word in ((65, 13, "64"), (0, 13, "64"), (32, 17, "16"), (32, 0, "16")):
        p = dl.GmmFloatParams(k, d, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)
        _einval(L.dsp_speaker_verifier_create(C.byref(p), 0, C.byref(h)), word)
        assert not h.value
    _einval(L.dsp_speaker_verifier_create(None, 0, C.byref(h)), "NULL")
    _einval(L.dsp_speaker_verifier_create(C.byref(dl.GmmFloatParams(4, 3, None, arr.ctypes.data, arr.ctypes.data)), 0, C.byref(h)), "NULL")
    _einval(L.dsp_speaker_verifier_create(C.byref(dl.GmmFloatParams(4, 3, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)), 0, None), "out")
    _einval(L.dsp_speaker_verifier_create(C.byref(dl.GmmFloatParams(4, 3, arr.ctypes.data, arr.ctypes.data, arr.ctypes.data)), -1, C.byref(h)), "device")
    bad = arr.copy()
    bad[3] = np.inf
    _einval(L.dsp_speaker_verifier_create(C.byref(dl.GmmFloatParams(4, 3, arr.ctypes.data, bad.ctypes.data, arr.ctypes.data)), 0, C.byref(h)), "finite")

    v = _verifier(L)
    off = lambda *a: (C.c_long * len(a))(*a)                                    # noqa: E731
    X, M, O = 0x1000, 0x2000, 0x3000                                             # never dereferenced: every call below is refused first

    def call(n_clips=2, offsets=off(0, 5, 9), n_spk=3, ver=v, feats=X, means=M, outs=(O, None, None, None, None)):
        return L.dsp_speaker_verify_ragged_device(ver, feats, n_clips, offsets, means, n_spk, *outs, None)

    _einval(call(ver=None), "verifier")
    _einval(call(feats=None), "d_feats")
    _einval(call(means=None), "d_means")
    _einval(call(offsets=None), "frame_offsets")
    _einval(call(outs=(None,) * 5), "every output", "NULL")
    _einval(call(offsets=off(0, 9, 5)), "decrease", "clip 1")
    _einval(call(offsets=off(-1, 5, 9)), "non-negative")
    _einval(call(n_clips=3, offsets=off(0, 5, 5, 9)), "clip 1", "no rows")
    _einval(call(n_clips=1, offsets=off(4, 4)), "clip 0", "no rows")
    _einval(call(n_clips=-1), ">= 0")
    _einval(call(n_spk=-2), ">= 0")
    _einval(call(n_spk=(1 << 19) + 1), "speakers")
    # zero clips or zero speakers: DSP_OK, no launch, no device -- whatever else is passed
    assert call(n_clips=0, offsets=None) == 0 and call(n_spk=0) == 0 and call(n_clips=0, offsets=None, feats=None, means=None, outs=(None,) * 5) == 0
    for out in range(5):                                                         # any single output will do: the next refusal is the device's
        outs = tuple(O if i == out else None for i in range(5))
        if L.dsp_device_count() <= 0:
            assert call(outs=outs) == -2 and "no HIP device" in dl.last_error()      # DSP_ENODEV, after every argument check
    L.dsp_speaker_verifier_destroy(v)
    L.dsp_speaker_verifier_destroy(None)


def test_verify_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
ubm = {"log_consts": np.zeros(4), "means": np.zeros((4, 3)), "inv_covs": np.ones((4, 3))}
for args in ((dict(ubm, means=np.zeros(4)),), (dict(ubm, log_consts=np.zeros(5)),),
             ({k: np.zeros((65, 3)) if k != "log_consts" else np.zeros(65) for k in ubm},)):
    try:
        dsp_amd.SpeakerVerifier(*args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for SpeakerVerifier{args}")
v = dsp_amd.SpeakerVerifier(ubm)                       # touches no device
assert (v.k, v.d) == (4, 3)
x, m = torch.zeros(8, 3), torch.zeros(2, 4, 3)
for call in (lambda: v.verify(x, [0, 8], m), lambda: v.verify(np.zeros((8, 3), np.float32), [0, 8], m), lambda: v.verify(x, [0, 8, 4], m),
             lambda: v.verify(x, [], m), lambda: v.verify(x, [0, 8], m, want=()), lambda: v.verify(x, [0, 8], m, want=("llr", "score"))):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for a bad verification argument")
v.close()
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
