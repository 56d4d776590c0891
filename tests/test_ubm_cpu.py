"""CPU: UBM training and the GMM quantiser (include/dsp_amd.h dsp_ubm_*, dsp_gmm_quantize) -- the numpy restatement of their definitions
(tests/ubm_ref.py) against sklearn's own GaussianMixture answers recorded in tests/golden/ubm_train_ref.npz, the deterministic start, the
host quantiser against the restatement and against the reference's integer tables, the exports, and every argument check the entries
make before they touch a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dsp_amd import lib as dl
from tests import enroll_ref as E
from tests import ubm_ref as U
from tests.ubm_util import ROOT, RUNS, fixture, fixture_fit

UBM_SYMBOLS = ["dsp_ubm_trainer_create", "dsp_ubm_trainer_destroy", "dsp_ubm_init_rows_device", "dsp_ubm_train_device", "dsp_gmm_quantize"]


def test_fixture_rows_are_exact_in_float32_and_the_start_is_the_librarys(golden):
    z, x, init = fixture(golden)
    assert x.dtype == np.float32 and x.shape == (6000, 13) and np.array_equal(x.astype(np.float64) * 4096.0, z["rows_q"])
    mine = U.init_rows(x, 32, float(z["reg_covar"]))
    for key in ("weights", "means", "variances"):
        assert np.array_equal(mine[key], init[key]), key
    assert [int(z[f"{tag}__n_iter"]) for tag in RUNS] == [1, 10, 32] and [bool(z[f"{tag}__converged"]) for tag in RUNS] == [False, False, True]


@pytest.mark.parametrize("tag", list(RUNS))
def test_restatement_reproduces_sklearns_recorded_answers(golden, tag):
    """float64 against float64: measured 4e-15 (weights), 2e-13 (means), 6e-13 relative (variances), 2e-15 (lower bound) when the fixture was
    made; the bounds are 1e-10 and 1e-9 relative, with room for another BLAS"""
    z, _, _ = fixture(golden)
    got = fixture_fit(golden)                                                    # one run to the tol stop: its first iterations are the other two
    i = int(z[f"{tag}__n_iter"])
    assert got["n_iter"] == 32 and got["converged"] and i <= got["n_iter"]
    w, mu, var = got["models"][i - 1]
    assert np.abs(w - z[f"{tag}__weights"]).max() <= 1e-10 and np.abs(mu - z[f"{tag}__means"]).max() <= 1e-10
    assert (np.abs(var - z[f"{tag}__variances"]) / z[f"{tag}__variances"]).max() <= 1e-9
    assert abs(got["lower_bounds"][i - 1] - float(z[f"{tag}__lower_bound"])) <= 1e-10
    if float(z[f"{tag}__tol"]) == 0.0:                                            # a tol of 0 never stops before max_iter
        assert not bool(z[f"{tag}__converged"]) and i == int(z[f"{tag}__max_iter"])
        assert np.all(np.abs(np.diff(np.concatenate([[-np.inf], got["lower_bounds"][:i]]))) > 0.0)
    else:                                                                         # the stop: the first change below tol, and none before
        change = np.abs(np.diff(np.concatenate([[-np.inf], got["lower_bounds"]])))
        assert change[-1] < float(z[f"{tag}__tol"]) and np.all(change[:-1] >= float(z[f"{tag}__tol"]))


def test_start_indices_variances_and_the_single_component():
    rng = np.random.default_rng(3)
    for n, k in ((5, 5), (7, 3), (1000, 32), (257, 64), (6, 1)):
        idx = U.init_row_indices(n, k)
        assert np.array_equal(idx, np.floor((np.arange(k) + 0.5) * n / k).astype(np.int64)) and idx.min() >= 0 and idx.max() < n
        assert np.all(np.diff(idx) >= 1) if k > 1 else True
    x = (rng.normal(0.3, 1.0, (700, 5)) * np.array([1.0, 0.1, 3.0, 0.01, 1.0])).astype(np.float32)
    init = U.init_rows(x, 6, 1e-6)
    x64 = x.astype(np.float64)
    assert np.array_equal(init["means"], x64[U.init_row_indices(700, 6)]) and np.array_equal(init["weights"], np.full(6, 1.0 / 6))
    assert np.abs(init["variances"] / (x64.var(axis=0) + 1e-6)[None] - 1.0).max() <= 1e-12
    one = U.fit(x, U.init_rows(x, 1, 0.0), max_iter=1, tol=0.0, reg_covar=0.0)    # k = 1: the global mean and variance in one iteration
    assert np.abs(one["means"][0] - x64.mean(axis=0)).max() <= 1e-12 and np.abs(one["variances"][0] / x64.var(axis=0) - 1.0).max() <= 1e-10
    assert abs(one["weights"][0] - 1.0) <= 1e-15 and one["n_iter"] == 1
    # centred moments in the float32 model keep a floor component's variance positive, where E[x^2] - mean^2 in float32 does not
    tight = (0.8 + 1e-3 * rng.normal(size=(512, 1))).astype(np.float32)
    m32 = U.fit(tight, {"weights": np.ones(1), "means": np.full((1, 1), 0.8), "variances": np.full((1, 1), 1e-6)}, 1, 0.0, 0.0, np.float32)
    assert m32["variances"][0, 0] > 0.0 and abs(m32["variances"][0, 0] / tight.astype(np.float64).var() - 1.0) < 1e-4


def _quantize_c(params):
    L = dl.load()
    keep = {key: np.ascontiguousarray(params[key], np.float64) for key in ("log_consts", "means", "inv_covs")}
    k, d = keep["means"].shape
    p = dl.GmmFloatParams(k, d, keep["log_consts"].ctypes.data, keep["means"].ctypes.data, keep["inv_covs"].ctypes.data)
    out = {"means": np.zeros((k, d), np.int8), "inv_covs": np.zeros((k, d), np.int32), "log_consts": np.zeros(k, np.int16)}
    sat = (C.c_int * 3)()
    rc = L.dsp_gmm_quantize(C.byref(p), out["means"].ctypes.data, out["inv_covs"].ctypes.data, out["log_consts"].ctypes.data, sat)
    assert rc == 0, dl.last_error()
    return out, dict(zip(("means", "inv_covs", "log_consts"), sat))


def test_quantiser_gives_the_references_integer_tables(golden):
    """the reference's float arrays (gmm_params.inc *_d, in speaker_enroll_ref.npz) quantise to its own integer tables
    (speaker_gmm_ref.npz), entry for entry, in all three formats -- by the restatement, by dsp_gmm_quantize and by dsp_amd.quantize_gmm"""
    import dsp_amd
    z, s = golden("speaker_enroll_ref.npz"), golden("speaker_gmm_ref.npz")
    for who in ("ubm", "target"):
        params = {key: z[f"{who}_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
        for q, sat in (U.quantize(params), _quantize_c(params), dsp_amd.quantize_gmm(params)):
            for key in ("means", "inv_covs", "log_consts"):
                assert q[key].dtype == s[f"{who}_{key}"].dtype and np.array_equal(q[key], s[f"{who}_{key}"]), (who, key)
            assert sat == {"means": 0, "inv_covs": 0, "log_consts": 0}


@pytest.mark.parametrize("k,d", [(1, 1), (5, 3), (32, 13), (64, 16)])
def test_quantiser_is_the_restatement_on_random_and_saturating_models(k, d):
    rng = np.random.default_rng(100 * k + d)
    for spread in (1.0, 40.0):                                                    # 40: means past +-2, inv_covs past 2^31 / 2048, log_consts past +-128
        params = E.random_ubm(rng, k, d)
        params["means"] = params["means"] * spread
        params["inv_covs"] = params["inv_covs"] * (spread if spread > 1.0 else 1.0)
        params["log_consts"] = params["log_consts"] * spread
        want, want_sat = U.quantize(params)
        got, got_sat = _quantize_c(params)
        for key in want:
            assert np.array_equal(got[key], want[key]), (k, d, spread, key)
        assert got_sat == want_sat
        if spread > 1.0 and k * d >= 15:
            assert want_sat["means"] > 0 and want_sat["inv_covs"] > 0
    # ties go to even, in all three formats; the limits themselves are not clamped, one past them is
    ties = {"means": np.array([[0.5, 1.5, 2.5, -0.5, -1.5, 127.0, -128.0, 127.5, -128.5, 128.0]]) / 64.0,
            "inv_covs": np.array([[0.5, 1.5, 2.5, 3.5, 4.5, 2147483647.0, 2147483647.5, 2147483648.0, 1e300, 6.5]]) / 2048.0,
            "log_consts": np.array([-32768.5 / 256.0])}
    got, sat = _quantize_c(ties)
    assert got["means"].tolist() == [[0, 2, 2, 0, -2, 127, -128, 127, -128, 127]] and sat["means"] == 2          # 127.5 -> 128 and 128 clamp; -128.5 -> -128
    assert got["inv_covs"].tolist() == [[0, 2, 2, 4, 4, 2147483647, 2147483647, 2147483647, 2147483647, 6]] and sat["inv_covs"] == 3
    assert got["log_consts"].tolist() == [-32768] and sat["log_consts"] == 0
    assert U.quantize(ties)[1] == sat
    got, sat = _quantize_c({"means": np.zeros((1, 1)), "inv_covs": np.array([[1.0 / 1e-6]]), "log_consts": np.array([-32769.0 / 256.0])})
    assert got["inv_covs"][0, 0] == 2048000000 and got["log_consts"][0] == -32768 and sat == {"means": 0, "inv_covs": 0, "log_consts": 1}
    assert int(np.rint(2048.0 / 1e-6)) < 2**31 - 1                                # reg_covar = 1e-6 still fits the Q11 table


def test_ubm_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in UBM_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_ubm_") or n.startswith("dsp_gmm_")) == sorted(UBM_SYMBOLS)
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "ubm_kernels.hpp")) as f:
        hpp = f.read()
    for name, value in (("kUbmChunkRows", U.CHUNK_ROWS), ("kUbmGroupChunks", U.GROUP_CHUNKS), ("kUbmSuperGroups", U.SUPER_GROUPS)):
        assert re.search(r"constexpr int " + name + r" = " + str(value) + r";", hpp), name
    assert "Not covered: UBM training" not in header


def _einval(rc, *words):
    assert rc == -1 and all(w in dl.last_error() for w in words), (rc, dl.last_error(), words)


def test_bad_arguments_are_einval_before_any_device_work():
    """every refusal of the trainer and of the quantiser, with the argument it names -- none of them needs a device (a trainer is made
    without one: its workspace is allocated by the first call that trains)"""
    L = dl.load()
    h = C.c_void_p()
    for k, d, word in ((0, 13, "k must"), (65, 13, "k must"), (32, 0, "d must"), (32, 17, "d must")):
        _einval(L.dsp_ubm_trainer_create(0, k, d, C.byref(h)), word)
        assert not h.value
    _einval(L.dsp_ubm_trainer_create(-1, 4, 3, C.byref(h)), "device")
    _einval(L.dsp_ubm_trainer_create(0, 4, 3, None), "out")
    assert L.dsp_ubm_trainer_create(0, 4, 3, C.byref(h)) == 0 and h.value
    k, d = 4, 3
    arrays = {key: np.zeros(shape) for key, shape in (("weights", k), ("means", (k, d)), ("variances", (k, d)), ("log_consts", k), ("inv_covs", (k, d)),
                                                       ("lower_bounds", 5))}
    res = dl.UbmResult()
    res.gmm.log_consts, res.gmm.means, res.gmm.inv_covs = (arrays[key].ctypes.data for key in ("log_consts", "means", "inv_covs"))
    res.weights, res.variances, res.lower_bounds = (arrays[key].ctypes.data for key in ("weights", "variances", "lower_bounds"))
    rows = C.c_void_p(4096)                                                        # never read: every call below is refused first
    good = {"weights": np.full(k, 0.25), "means": np.zeros((k, d)), "variances": np.ones((k, d))}

    def train(t=h, feats=rows, n=100, init=good, cfg=(5, 1e-3, 1e-6), result=res):
        keep = None if init is None else {key: np.ascontiguousarray(v, np.float64) for key, v in init.items()}
        start = None if init is None else dl.UbmInit(*[keep[key].ctypes.data for key in ("weights", "means", "variances")])
        return L.dsp_ubm_train_device(t, feats, n, C.byref(start) if start is not None else None, C.byref(dl.UbmConfig(*cfg)) if cfg else None,
                                      C.byref(result) if result is not None else None, None)

    _einval(train(t=None), "trainer")
    _einval(train(feats=None), "d_feats")
    _einval(train(n=3), "n must be at least k = 4")
    _einval(train(n=-1), "n must be at least k")
    _einval(train(init=None, n=2), "n must be at least k")
    _einval(train(cfg=None), "dsp_ubm_config")
    for max_iter in (0, -3):
        _einval(train(cfg=(max_iter, 1e-3, 1e-6)), "max_iter")
    for tol in (-1e-9, float("nan")):
        _einval(train(cfg=(5, tol, 1e-6)), "tol")
    for reg in (-1e-9, float("nan"), float("inf")):
        _einval(train(cfg=(5, 1e-3, reg)), "reg_covar")
    for w, word in (([0.5, 0.5, 0.0, 0.0], "weights must be > 0"), ([0.5, 0.7, -0.1, -0.1], "weights must be > 0"), ([0.25, 0.25, 0.25, 0.2], "sum to 1"),
                    ([0.3, 0.3, 0.3, 0.3], "sum to 1"), ([0.25, 0.25, float("nan"), 0.25], "finite"), ([0.25, float("inf"), 0.25, 0.25], "finite")):
        _einval(train(init=dict(good, weights=np.array(w))), "weights", word)
    for v in (0.0, -1.0):
        bad = np.ones((k, d))
        bad[2, 1] = v
        _einval(train(init=dict(good, variances=bad)), "variances must be > 0", "component 2")
    for key in ("means", "variances"):
        for v in (float("nan"), float("inf")):
            bad = np.ones((k, d))
            bad[1, 2] = v
            _einval(train(init=dict(good, **{key: bad})), "finite")
    _einval(L.dsp_ubm_train_device(h, rows, 100, C.byref(dl.UbmInit(None, good["means"].ctypes.data, good["variances"].ctypes.data)),
                                   C.byref(dl.UbmConfig(5, 1e-3, 1e-6)), C.byref(res), None), "dsp_ubm_init")
    _einval(train(result=None), "dsp_ubm_result")
    empty = dl.UbmResult()
    _einval(train(result=empty), "dsp_ubm_result")
    out = [np.zeros(k), np.zeros((k, d)), np.zeros((k, d))]
    ptrs = [a.ctypes.data for a in out]
    _einval(L.dsp_ubm_init_rows_device(None, rows, 100, 1e-6, *ptrs, None), "trainer")
    _einval(L.dsp_ubm_init_rows_device(h, None, 100, 1e-6, *ptrs, None), "d_feats")
    _einval(L.dsp_ubm_init_rows_device(h, rows, 3, 1e-6, *ptrs, None), "n must be at least k")
    _einval(L.dsp_ubm_init_rows_device(h, rows, 100, -1.0, *ptrs, None), "reg_covar")
    _einval(L.dsp_ubm_init_rows_device(h, rows, 100, float("nan"), *ptrs, None), "reg_covar")
    _einval(L.dsp_ubm_init_rows_device(h, rows, 100, 1e-6, None, ptrs[1], ptrs[2], None), "NULL")
    L.dsp_ubm_trainer_destroy(h)
    L.dsp_ubm_trainer_destroy(None)
    assert all(np.all(a == 0.0) for a in arrays.values()) and all(np.all(a == 0.0) for a in out)       # no refused call wrote anything
    # the quantiser
    z = np.zeros(65 * 17)
    i8, i32, i16, sat = np.zeros(65 * 17, np.int8), np.zeros(65 * 17, np.int32), np.zeros(65, np.int16), (C.c_int * 3)()
    for kk, dd, word in ((65, 13, "64"), (0, 13, "64"), (32, 17, "16"), (32, 0, "16")):
        _einval(L.dsp_gmm_quantize(C.byref(dl.GmmFloatParams(kk, dd, z.ctypes.data, z.ctypes.data, z.ctypes.data)), i8.ctypes.data, i32.ctypes.data,
                                   i16.ctypes.data, sat), word)
    _einval(L.dsp_gmm_quantize(None, i8.ctypes.data, i32.ctypes.data, i16.ctypes.data, sat), "NULL")
    _einval(L.dsp_gmm_quantize(C.byref(dl.GmmFloatParams(4, 3, None, z.ctypes.data, z.ctypes.data)), i8.ctypes.data, i32.ctypes.data, i16.ctypes.data, sat), "NULL")
    _einval(L.dsp_gmm_quantize(C.byref(dl.GmmFloatParams(4, 3, z.ctypes.data, z.ctypes.data, z.ctypes.data)), None, i32.ctypes.data, i16.ctypes.data, sat), "NULL")
    _einval(L.dsp_gmm_quantize(C.byref(dl.GmmFloatParams(4, 3, z.ctypes.data, z.ctypes.data, z.ctypes.data)), i8.ctypes.data, i32.ctypes.data, i16.ctypes.data, None), "NULL")
    nan = z.copy()
    nan[5] = np.nan
    _einval(L.dsp_gmm_quantize(C.byref(dl.GmmFloatParams(4, 3, z.ctypes.data, nan.ctypes.data, z.ctypes.data)), i8.ctypes.data, i32.ctypes.data, i16.ctypes.data, sat), "NaN")


def test_ubm_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
for f, args in ((dsp_amd.UbmTrainer, (0, 13)), (dsp_amd.UbmTrainer, (65, 13)), (dsp_amd.UbmTrainer, (32, 17)), (dsp_amd.UbmTrainer, (32, 0)),
                (dsp_amd.quantize_gmm, ({"log_consts": np.zeros(4), "means": np.zeros(4), "inv_covs": np.zeros(4)},)),
                (dsp_amd.quantize_gmm, ({"log_consts": np.zeros(5), "means": np.zeros((4, 3)), "inv_covs": np.zeros((4, 3))},)),
                (dsp_amd.quantize_gmm, ({"log_consts": np.zeros(65), "means": np.zeros((65, 3)), "inv_covs": np.zeros((65, 3))},))):
    try:
        f(*args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for {f.__name__}{args}")
t = dsp_amd.UbmTrainer(4, 3)
x = torch.zeros(8, 3)
good = {"weights": np.full(4, 0.25), "means": np.zeros((4, 3)), "variances": np.ones((4, 3))}
for call in (lambda: t.fit(x), lambda: t.init_rows(x), lambda: t.fit(np.zeros((8, 3), np.float32)), lambda: t.fit(x, max_iter=0),
             lambda: t.fit(x, tol=-1.0), lambda: t.fit(x, tol=float("nan")), lambda: t.fit(x, reg_covar=-1.0), lambda: t.init_rows(x, reg_covar=float("nan")),
             lambda: t.fit(x, init=dict(good, weights=np.full(3, 1 / 3))), lambda: t.fit(x, init=dict(good, weights=np.array([0.5, 0.5, 0.0, 0.0]))),
             lambda: t.fit(x, init=dict(good, variances=np.zeros((4, 3)))), lambda: t.fit(x, init=dict(good, means=np.full((4, 3), np.nan)))):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for a bad training argument")
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
