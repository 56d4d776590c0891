"""CPU: the k-means start of UBM training (include/dsp_amd.h dsp_kmeans_*) -- the numpy restatement of its definitions
(tests/kmeans_ref.py) against sklearn's own KMeans answers recorded in tests/golden/kmeans_ref.npz, what the fixture must be for a float32
kernel to owe every label, the draws, the seeding's validity rule, the exports, and every argument check made before a device is touched."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dsp_amd import lib as dl
from tests import kmeans_ref as K
from tests.kmeans_util import CASES, fixture, fixture_lloyd
from tests.ubm_util import ROOT

KMEANS_SYMBOLS = ["dsp_kmeans_seed_device", "dsp_kmeans_fit_device", "dsp_kmeans_train_ubm_device"]


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_sklearns_recorded_answers(golden, tag):
    """float64 against float64.  Measured when the fixture was made: n_iter and every label equal; centres 3e-15, inertia 7e-16 relative,
    weights 0, means 9e-16, variances 4e-14 relative.  The bounds are 1e-12 and 1e-11 relative, with room for another BLAS."""
    z, x, sk = fixture(golden, tag)
    assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64) * 4096.0, sk["rows_q"])
    got = fixture_lloyd(golden, tag)
    assert got["n_iter"] == int(sk["n_iter"]) and got["stop"] == str(sk["stop"]) and np.array_equal(got["labels"], sk["labels"])
    assert np.abs(got["centres"] - sk["centres"]).max() <= 1e-12 and abs(got["inertia"] / float(sk["inertia"]) - 1.0) <= 1e-12
    assert np.abs(got["weights"] - sk["weights"]).max() <= 1e-12 and np.abs(got["means"] - sk["means"]).max() <= 1e-12
    assert np.abs(got["variances"] / sk["variances"] - 1.0).max() <= 1e-11
    assert np.array_equal(got["counts"], np.bincount(sk["labels"], minlength=got["centres"].shape[0]))


@pytest.mark.parametrize("tag", CASES)
def test_fixture_has_no_empty_cluster_and_a_margin_float32_cannot_cross(golden, tag):
    """at every iteration and in the final labelling: every cluster has rows, and every row's relative label margin against the
    float32-rounded centres is at least 16 x 2 (d + 3) 2^-24 -- 2 (d + 3) 2^-24 bounds the rounding of a d-term float32 sum of squares, so
    a correct float32 kernel reproduces every label; a tol stop has no shift within 1e-3 of the limit"""
    z, x, sk = fixture(golden, tag)
    ref = fixture_lloyd(golden, tag)
    k, d = ref["centres"].shape
    limit = K.shift_limit(x, float(z["tol"]))
    against = [t[0] for t in ref["trace"]] + [ref["centres"]]
    assert len(ref["trace"]) == ref["n_iter"] and ref["n_empty"] == 0
    for centres in against:
        s = K.sq_dists(x, centres.astype(np.float32).astype(np.float64))
        assert np.bincount(np.argmin(s, axis=1), minlength=k).min() > 0
        assert K.margins(s).min() >= 16.0 * K.rounding_bound(d)
    shifts = np.array([t[3] for t in ref["trace"]])
    if str(sk["stop"]) == "tol":
        assert np.all(np.abs(shifts - limit) > 1e-3 * limit) and np.all(shifts[:-1] > limit) and shifts[-1] <= limit
    else:
        assert np.all(shifts[:-1] > limit)                            # the strict stop came first, not by a hair
    model = fixture_lloyd(golden, tag, np.float32)                     # so the float32 model walks the same path
    assert model["n_iter"] == ref["n_iter"] and model["stop"] == ref["stop"] and np.array_equal(model["labels"], ref["labels"])


def test_draws_are_splitmix64():
    """u(0, 0, t) are the first outputs of splitmix64 seeded with 0 (its published test vector), top 53 bits; every draw is in [0, 1)"""
    first = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for t, word in enumerate(first):
        assert K.mix((t + 1) * K.GOLDEN) == word and K.draw(0, 0, t) == (word >> 11) * 2.0 ** -53
    assert K.draw(0, 0, 0) == 0.8833108082136426
    u = np.array([K.draw(seed, j, t) for seed in (0, 1, 42, 2 ** 64 - 1) for j in range(64) for t in range(K.MAX_TRIALS)])
    assert u.min() >= 0.0 and u.max() < 1.0 and np.unique(u).size == u.size and abs(u.mean() - 0.5) < 0.05
    assert K.draw(2 ** 64 - 1, 63, 5) == K.draw(-1 % 2 ** 64, 63, 5)   # wrap-around, not overflow
    assert [K.trials(k) for k in (1, 2, 3, 7, 8, 20, 21, 32, 54, 55, 64)] == [2, 2, 3, 3, 4, 4, 5, 5, 5, 6, 6]
    assert len({K.restart_seed(7, r) for r in range(8)} | {7}) == 9


@pytest.mark.parametrize("n,k,d", [(64, 64, 3), (700, 5, 1), (1500, 8, 13), (1025, 32, 13), (4097, 64, 16)])
def test_float32_seedings_are_valid_against_float64(n, k, d):
    """the validity rule the GPU's seeding is held to accepts the float32 model's, and refuses a seeding that is not greedy"""
    rng = np.random.default_rng(1000 * n + k)
    x = (rng.normal(0.0, 2.0, (k, d))[rng.integers(0, k, n)] + rng.normal(0.0, 0.7, (n, d))).astype(np.float32)
    for seed in (0, 1, 42):
        rows = K.seed_rows(x, k, seed, np.float32)
        assert K.seeding_is_valid(x, rows, seed) is None
        assert K.seeding_is_valid(x, K.seed_rows(x, k, seed), seed) is None
    if k < n:
        bad = rows.copy()
        bad[-1] = bad[0]
        assert "distinct" in K.seeding_is_valid(x, bad, 42)
        bad[0] = (rows[0] + 1) % n
        assert K.seeding_is_valid(x, bad, 42) is not None
    with pytest.raises(K.TooFewDistinctRows):
        K.seed_rows(np.repeat(x[:max(k - 1, 1)], 3, axis=0)[:max(n, k)] if k > 1 else x, k + (k == 1), 3)


def test_kmeans_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in KMEANS_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert sorted(n for n in dl.SYMBOLS if n.startswith("dsp_kmeans_")) == sorted(KMEANS_SYMBOLS)
    assert "kmeans_kernels.hip" in dl._build.SOURCES and "kmeans_kernels.hpp" in dl._build.HEADERS
    assert "initialisation and its n_init restarts are not built" not in header and "Not covered: k-means" not in header
    for size, mirror in ((24, dl.KmeansConfig), (72, dl.KmeansResult), (56, dl.KmeansUbmConfig), (64 * 8 + 32, dl.KmeansRestart), (16, dl.KmeansUbmReport)):
        assert C.sizeof(mirror) == size, mirror.__name__


def _einval(rc, *words):
    assert rc == -1 and all(w in dl.last_error() for w in words), (rc, dl.last_error(), words)


def test_bad_arguments_are_einval_before_any_device_work():
    L = dl.load()
    h = C.c_void_p()
    assert L.dsp_ubm_trainer_create(0, 4, 3, C.byref(h)) == 0 and h.value
    k, d = 4, 3
    rows = C.c_void_p(4096)                                                        # never read: every call below is refused first
    picked = np.zeros(k, np.int64)
    _einval(L.dsp_kmeans_seed_device(None, rows, 100, 1, picked.ctypes.data, None), "trainer")
    _einval(L.dsp_kmeans_seed_device(h, None, 100, 1, picked.ctypes.data, None), "d_feats")
    _einval(L.dsp_kmeans_seed_device(h, rows, 3, 1, picked.ctypes.data, None), "n must be at least k = 4")
    _einval(L.dsp_kmeans_seed_device(h, rows, 100, 1, None, None), "rows")
    arrays = {key: np.zeros(shape, t) for key, shape, t in (("centres", (k, d), np.float64), ("counts", k, np.int64), ("weights", k, np.float64),
                                                            ("means", (k, d), np.float64), ("variances", (k, d), np.float64))}
    res = dl.KmeansResult(*[arrays[key].ctypes.data for key in ("centres", "counts", "weights", "means", "variances")], None)
    good = np.zeros((k, d))

    def fit(t=h, feats=rows, n=100, centres=good, cfg=(5, 1e-4, 1e-6), result=res):
        return L.dsp_kmeans_fit_device(t, feats, n, centres.ctypes.data if centres is not None else None, C.byref(dl.KmeansConfig(*cfg)) if cfg else None,
                                       C.byref(result) if result is not None else None, None)

    _einval(fit(t=None), "trainer")
    _einval(fit(feats=None), "d_feats")
    _einval(fit(n=3), "n must be at least k = 4")
    _einval(fit(centres=None), "centres0")
    _einval(fit(cfg=None), "dsp_kmeans_config")
    for max_iter in (0, -3):
        _einval(fit(cfg=(max_iter, 1e-4, 1e-6)), "max_iter")
    for tol in (-1e-9, float("nan"), float("inf")):
        _einval(fit(cfg=(5, tol, 1e-6)), "tol")
    for reg in (-1e-9, float("nan"), float("inf")):
        _einval(fit(cfg=(5, 1e-4, reg)), "reg_covar")
    for v in (float("nan"), float("inf"), -float("inf"), 1e39):
        bad = good.copy()
        bad[2, 1] = v
        _einval(fit(centres=bad), "centres0 must be finite", "centre 2")
    _einval(fit(result=None), "dsp_kmeans_result")
    _einval(fit(result=dl.KmeansResult()), "dsp_kmeans_result")
    ubm = {key: np.zeros(shape) for key, shape in (("weights", k), ("means", (k, d)), ("variances", (k, d)), ("log_consts", k), ("inv_covs", (k, d)),
                                                   ("lower_bounds", 5))}
    ures = dl.UbmResult()
    ures.gmm.log_consts, ures.gmm.means, ures.gmm.inv_covs = (ubm[key].ctypes.data for key in ("log_consts", "means", "inv_covs"))
    ures.weights, ures.variances, ures.lower_bounds = (ubm[key].ctypes.data for key in ("weights", "variances", "lower_bounds"))
    restarts = (dl.KmeansRestart * 3)()
    report = dl.KmeansUbmReport(restarts, -7)

    def train(t=h, feats=rows, n=100, cfg=(2, 42, 300, 1e-4, (5, 1e-3, 1e-6)), result=ures, rep=report):
        c = dl.KmeansUbmConfig(cfg[0], cfg[1], cfg[2], cfg[3], dl.UbmConfig(*cfg[4])) if cfg else None
        return L.dsp_kmeans_train_ubm_device(t, feats, n, C.byref(c) if c is not None else None, C.byref(result) if result is not None else None,
                                             C.byref(rep) if rep is not None else None, None)

    _einval(train(t=None), "trainer")
    _einval(train(feats=None), "d_feats")
    _einval(train(n=-1), "n must be at least k")
    _einval(train(cfg=None), "dsp_kmeans_ubm_config")
    for n_init in (0, -1):
        _einval(train(cfg=(n_init, 42, 300, 1e-4, (5, 1e-3, 1e-6))), "n_init")
    _einval(train(cfg=(2, 42, 0, 1e-4, (5, 1e-3, 1e-6))), "kmeans_max_iter")
    for tol in (-1.0, float("nan"), float("inf")):
        _einval(train(cfg=(2, 42, 300, tol, (5, 1e-3, 1e-6))), "kmeans_tol")
    _einval(train(cfg=(2, 42, 300, 1e-4, (0, 1e-3, 1e-6))), "em.max_iter")
    _einval(train(cfg=(2, 42, 300, 1e-4, (5, -1.0, 1e-6))), "em.tol")
    for reg in (-1.0, float("nan"), float("inf")):
        _einval(train(cfg=(2, 42, 300, 1e-4, (5, 1e-3, reg))), "reg_covar")
    _einval(train(result=None), "dsp_ubm_result")
    _einval(train(result=dl.UbmResult()), "dsp_ubm_result")
    _einval(train(rep=None), "dsp_kmeans_ubm_report")
    _einval(train(rep=dl.KmeansUbmReport(None, 0)), "dsp_kmeans_ubm_report")
    L.dsp_ubm_trainer_destroy(h)
    assert all(np.all(a == 0) for a in arrays.values()) and all(np.all(a == 0.0) for a in ubm.values()) and np.all(picked == 0)
    assert report.winner == -7                                                     # no refused call wrote anything


def test_kmeans_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
assert not __debug__
t = dsp_amd.UbmTrainer(4, 3)
x = torch.zeros(8, 3)
good = np.zeros((4, 3))
for call in (lambda: t.kmeans_seed(x), lambda: t.kmeans_seed(np.zeros((8, 3), np.float32)), lambda: t.kmeans_seed(x, seed=-1), lambda: t.kmeans_seed(x, seed=2 ** 64),
             lambda: t.kmeans(x, good), lambda: t.kmeans(x, np.zeros((3, 3))), lambda: t.kmeans(x, np.full((4, 3), np.nan)),
             lambda: t.kmeans(x, good, max_iter=0), lambda: t.kmeans(x, good, tol=-1.0), lambda: t.kmeans(x, good, tol=float("nan")),
             lambda: t.kmeans(x, good, tol=float("inf")), lambda: t.kmeans(x, good, reg_covar=-1.0),
             lambda: t.fit(x, init="kmeans"), lambda: t.fit(x, init="random"), lambda: t.fit(x, init="kmeans", n_init=0), lambda: t.fit(x, n_init=2),
             lambda: t.fit(x, init="kmeans", seed=-1), lambda: t.fit(x, init="kmeans", kmeans_max_iter=0), lambda: t.fit(x, init="kmeans", kmeans_tol=-1.0),
             lambda: t.fit(x, init="kmeans", max_iter=0), lambda: t.fit(x, init="kmeans", reg_covar=float("nan"))):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for a bad k-means argument")
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_restarts_keep_the_largest_last_lower_bound():
    """section 3 of the restatement: n_init = 1 is restart 0 alone, more restarts never end lower, the winner is the first argmax, and
    the float32 model seeds the same rows on rows this well separated"""
    rng = np.random.default_rng(12)
    x = (rng.normal(0.0, 3.0, (4, 3))[rng.integers(0, 4, 600)] + rng.normal(0.0, 0.5, (600, 3))).astype(np.float32)
    one, rep1 = K.train_ubm(x, 4, 42, n_init=1, max_iter=5)
    three, rep3 = K.train_ubm(x, 4, 42, n_init=3, max_iter=5)
    assert rep1["winner"] == 0 and np.array_equal(rep1["restarts"][0]["rows"], K.seed_rows(x, 4, K.restart_seed(42, 0)))
    assert np.array_equal(rep3["restarts"][0]["rows"], rep1["restarts"][0]["rows"]) and rep3["restarts"][0]["lower_bound"] == rep1["restarts"][0]["lower_bound"]
    bounds = [r["lower_bound"] for r in rep3["restarts"]]
    assert rep3["winner"] == int(np.argmax(bounds)) and three["lower_bounds"][-1] == max(bounds) >= one["lower_bounds"][-1]
    for r in range(3):
        assert K.seeding_is_valid(x, K.seed_rows(x, 4, K.restart_seed(42, r), np.float32), K.restart_seed(42, r)) is None
