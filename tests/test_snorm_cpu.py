"""No GPU: the restatement of cohort normalisation (tests/snorm_ref.py) against an independent form written here with numpy's own
sort, mean and std; its edge cases; every refusal of dsp_cohort_stats_device and dsp_score_normalize_device through the built library,
in the header's order and with no device present; the prototypes and the record's 32 bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import snorm_ref as R
from tests import snorm_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNORM_SYMBOLS = ["dsp_cohort_stats_device", "dsp_score_normalize_device"]


# ---- the restatement --------------------------------------------------------------------------------------------------------------------

def test_keys_grow_with_the_float_and_put_minus_zero_first():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], np.float32)
    k = R.keys(v)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(R.float_of(k).view(np.uint32), v.view(np.uint32))
    assert R.keys(np.array([np.nan], np.float32))[0] > k[-1]                        # (a positive NaN lies above +inf: only finite values take part)


def test_the_tree_is_fixed_by_the_length_alone():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 64, 65, 4095, 4096, 4097, 9000):
        x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 8, n)
        want = 0.0
        for c0 in range(0, n, R.CHUNK):                                             # the definition, leaf by leaf
            level = list(x[c0:c0 + R.CHUNK]) + [0.0] * (R.CHUNK - len(x[c0:c0 + R.CHUNK]))
            while len(level) > 1:
                level = [level[i] + level[i + 1] for i in range(0, len(level), 2)]
            want = level[0] if c0 == 0 else want + level[0]
        assert R.tree_sum(x) == want, n
    assert R.tree_sum(np.array([1e16, 1.0, -1e16, 1.0])) == 0.0                     # ((1e16 + 1) + (-1e16 + 1)): pairwise, not sequential
    assert not np.signbit(R.tree_sum(np.array([-0.0])))                             # (-0 + the absent leaf's +0)


def test_the_record_of_hand_made_vectors():
    r = R.stat(np.array([1.0, 3.0, np.nan, 2.0, np.inf, 3.0, -np.inf], np.float32), 2)
    assert (r["n_finite"], r["n_selected"], r["n_above"], r["threshold"], r["mean"], r["std"]) == (4, 2, 0, 3.0, 3.0, 0.0)
    r = R.stat(np.array([1.0, 3.0, np.nan, 2.0, np.inf, 3.0, -np.inf], np.float32), 3)
    assert (r["n_finite"], r["n_selected"], r["n_above"], r["threshold"]) == (4, 3, 2, 2.0) and r["mean"] == 8.0 / 3.0
    assert r["std"] == np.array([3.0, 3.0, 2.0]).std()
    for k in (0, 4, 5, 1 << 22):
        r = R.stat(np.array([1.0, 3.0, np.nan, 2.0, np.inf, 3.0, -np.inf], np.float32), k)
        assert (r["n_selected"], r["n_above"], r["threshold"], r["mean"]) == (4, 3, 1.0, 2.25)
    r = R.stat(np.array([0.0, -0.0, 0.0, -0.0], np.float32), 2)                     # -0 before +0: the two +0 are the largest
    assert (r["n_above"], r["n_selected"]) == (0, 2) and not np.signbit(r["threshold"]) and r["mean"] == 0.0 and r["std"] == 0.0
    r = R.stat(np.array([0.0, -0.0, 0.0, -0.0], np.float32), 3)
    assert (r["n_above"], r["n_selected"]) == (2, 3) and np.signbit(r["threshold"])
    r = R.stat(np.array([np.nan, np.inf, -np.inf], np.float32), 1)
    assert np.isnan([r["mean"], r["std"], r["threshold"]]).all() and (r["n_finite"], r["n_selected"], r["n_above"]) == (0, 0, 0)
    assert R.STAT_DTYPE.itemsize == 32 and np.dtype(dl.COHORT_STAT_DTYPE) == R.STAT_DTYPE


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 100, 1000, 4095, 4096, 4097])
def test_restatement_against_the_independent_form(n):
    """Records of the restatement against np.sort(finite values as float64)[-K':] with numpy's mean and std: the threshold and the three
    counts exactly, the outputs of all three modes within the gate (tests/snorm_util.py gate_misses)."""
    vectors = 12
    x = U.special(n, vectors) if n >= 5 else U.cohort(n, vectors)
    sc = U.scores(vectors, vectors, n)
    for k in U.top_ks(n):
        rec = R.stats(x, R.PER_ROW, k)
        mean, std, theta, nf, ns, na = U.independent_records(x, k)
        assert np.array_equal(rec["threshold"].view(np.uint32), theta.view(np.uint32)), (n, k)
        assert np.array_equal(rec["n_finite"], nf) and np.array_equal(rec["n_selected"], ns) and np.array_equal(rec["n_above"], na), (n, k)
        for mode in (R.NORM_Z, R.NORM_T, R.NORM_S):
            got = R.apply(sc, mode, rec, rec, 1e-6)
            assert got.dtype == np.float32 and U.gate_misses(got, sc, mode, (mean, std), (mean, std), 1e-6) == 0, (n, k, mode)


def test_a_record_does_not_depend_on_the_axis_or_on_its_neighbours():
    x = U.special(300, 12)
    a, b = R.stats(x, R.PER_ROW, 7), R.stats(np.ascontiguousarray(x.T), R.PER_COLUMN, 7)
    assert U.same_bits(a, b) is None and U.same_bits(R.stats(x[3:5], R.PER_ROW, 7), a[3:5]) is None
    assert U.same_bits(a, R.stats(x, R.PER_ROW, 8)) is not None


def test_apply_floors_sigma_rounds_once_and_keeps_nan():
    st = np.zeros(2, R.STAT_DTYPE)
    st["mean"], st["std"], st["n_finite"] = [1.0, -2.0], [0.5, 0.0], [3, 3]
    x = np.array([[2.0, -2.0], [np.nan, 1.0]], np.float32)
    z = R.apply(x, R.NORM_Z, None, st, 1e-6)
    assert z[0, 0] == 2.0 and z[0, 1] == 0.0 and np.isnan(z[1, 0]) and z[1, 1] == np.float32(3.0 / 1e-6)
    z0 = R.apply(x, R.NORM_Z, None, st, 0.0)
    assert np.isnan(z0[0, 1]) and z0[1, 1] == np.inf                                 # sigma' = 0: 0 / 0 and 3 / 0, as IEEE has them
    t = R.apply(x, R.NORM_T, st, None, 1e-6)
    assert t[0, 0] == 2.0 and t[0, 1] == -6.0 and t[1, 1] == np.float32(3.0 / 1e-6)
    s = R.apply(x, R.NORM_S, st, st, 1e-6)
    assert s[0, 0] == 2.0 and s[0, 1] == -3.0
    empty = np.zeros(2, R.STAT_DTYPE)
    empty["mean"] = empty["std"] = np.nan
    assert np.isnan(R.apply(x, R.NORM_S, st, empty, 1e-6)).all() and np.isnan(R.apply(x, R.NORM_T, empty, None, 1e-6)).all()
    v = np.float32(1.0 + 2.0 ** -23)                                                # the quotient is rounded once, from float64
    st["mean"], st["std"] = [2.0 ** -30, 0.0], [1.0 + 2.0 ** -29, 1.0]
    assert R.apply(np.array([[v, v]], np.float32), R.NORM_Z, None, st, 0.0)[0, 0] == np.float32((np.float64(v) - 2.0 ** -30) / (1.0 + 2.0 ** -29))


# ---- the library's host code ---------------------------------------------------------------------------------------------------------------

def test_refusals_touch_no_device_and_come_in_the_header_s_order():
    L = dsp_amd.load()
    ptr = C.c_void_p(64)              # never dereferenced: every call below is refused before a device is touched

    def stats(device=0, d_cohort=ptr, R_=4, C_=6, axis=dl.COHORT_PER_ROW, top_k=0, d_stats=ptr):
        return L.dsp_cohort_stats_device(device, d_cohort, R_, C_, axis, top_k, d_stats, None)

    def norm(device=0, d_scores=ptr, T=4, S=2, row=ptr, col=ptr, mode=dl.NORM_S, floor=1e-6, cfg=True, d_out=ptr):
        c = dl.SnormConfig(mode, 0, floor)
        return L.dsp_score_normalize_device(device, d_scores, T, S, row, col, C.byref(c) if cfg else None, d_out, None)

    nan, inf = float("nan"), float("inf")
    stats_refused = [                                        # include/dsp_amd.h: "the first of"
        (dict(device=-1), "device index out of range"),
        (dict(axis=2), "axis"),
        (dict(top_k=-1), "top_k must be 0 .. 2^22, got -1"),
        (dict(R_=-1), "n_rows or n_cols < 0"),
        (dict(d_cohort=None), "d_cohort is NULL"),
        (dict(d_stats=None), "d_stats is NULL"),
    ]
    norm_refused = [
        (dict(device=-1), "device index out of range"),
        (dict(cfg=False), "dsp_snorm_config is NULL"),
        (dict(mode=3), "mode"),
        (dict(floor=-1e-9), "std_floor"),
        (dict(T=-1), "n_rows or n_cols < 0"),
        (dict(d_scores=None), "d_scores is NULL"),
        (dict(d_out=None), "d_out is NULL"),
        (dict(row=None), "d_row_stats is NULL"),
        (dict(col=None), "d_col_stats is NULL"),
    ]
    for call, refused in ((stats, stats_refused), (norm, norm_refused)):
        for kwargs, word in refused:
            assert call(**kwargs) == -1, kwargs
            assert word in dl.last_error(), (kwargs, dl.last_error())
        for i in range(len(refused) - 1):                    # the order: of two refusals the earlier one is reported
            for j in range(i + 1, len(refused)):
                if set(refused[i][0]) & set(refused[j][0]):
                    continue
                both = dict(refused[j][0], **refused[i][0])
                assert call(**both) == -1 and refused[i][1] in dl.last_error(), (refused[i], refused[j], dl.last_error())
    # the other values of every refusal
    for kwargs, word in [(dict(axis=-1), "axis"), (dict(top_k=(1 << 22) + 1), "top_k"), (dict(C_=-2), "n_rows or n_cols < 0"),
                         (dict(R_=(1 << 30) + 1), "2^30 vectors"), (dict(C_=(1 << 30) + 1, axis=dl.COHORT_PER_COLUMN), "2^30 vectors"),
                         (dict(C_=0), "cohort length must be 1 .. 2^22, got 0"), (dict(C_=(1 << 22) + 1), "cohort length"),
                         (dict(R_=0, axis=dl.COHORT_PER_COLUMN), "cohort length must be 1 .. 2^22, got 0"),
                         (dict(R_=(1 << 22) + 1, axis=dl.COHORT_PER_COLUMN), "cohort length"),
                         (dict(R_=(1 << 30) + 1, C_=0), "2^30 vectors"), (dict(C_=0, d_cohort=None), "cohort length")]:
        assert stats(**kwargs) == -1 and word in dl.last_error(), (kwargs, dl.last_error())
    assert stats(top_k=1 << 22, C_=1 << 22, d_cohort=None) == -1 and "d_cohort" in dl.last_error()      # (the limits themselves pass)
    for kwargs, word in [(dict(mode=-1), "mode"), (dict(floor=nan), "std_floor"), (dict(floor=inf), "std_floor"), (dict(S=-1), "n_rows or n_cols < 0"),
                         (dict(T=(1 << 30) + 1), "2^30 rows or columns"), (dict(S=(1 << 30) + 1), "2^30 rows or columns"),
                         (dict(mode=dl.NORM_T, row=None), "d_row_stats"), (dict(mode=dl.NORM_Z, col=None), "d_col_stats")]:
        assert norm(**kwargs) == -1 and word in dl.last_error(), (kwargs, dl.last_error())
    # what a mode does not need may be NULL, and a floor of 0 is allowed: the refusal is that of the scores, which comes later
    for kwargs in (dict(mode=dl.NORM_Z, row=None), dict(mode=dl.NORM_T, col=None), dict(floor=0.0)):
        rc = norm(d_scores=None, **kwargs)
        assert rc == -1 and "d_scores is NULL" in dl.last_error(), kwargs
    # nothing to do: DSP_OK, no launch, whatever the pointers
    assert stats(R_=0) == 0 and stats(R_=0, C_=0, d_cohort=None, d_stats=None) == 0 and stats(C_=0, axis=dl.COHORT_PER_COLUMN, d_cohort=None) == 0
    assert norm(T=0) == 0 and norm(S=0, d_scores=None, d_out=None, row=None, col=None) == 0
    assert stats(R_=0, top_k=-1) == -1 and norm(T=0, mode=7) == -1 and norm(T=0, floor=-1.0) == -1      # what comes before is still refused


def test_symbols_are_declared_exported_and_listed():
    L = dsp_amd.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dsp_amd.build.LIB], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    for name in SNORM_SYMBOLS:
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported and re.search(r"\b%s\(" % name, header), name
    assert [n for n in dl.SYMBOLS if "normaliz" in n or "cohort" in n] == SNORM_SYMBOLS
    assert "ScoreNormalizer" in dsp_amd.__all__ and issubclass(dsp_amd.ScoreNormalizer, dl.Closing)
    assert "capi_snorm.cpp" in dsp_amd.build.SOURCES and "snorm_kernels.hip" in dsp_amd.build.SOURCES and "snorm_kernels.hpp" in dsp_amd.build.HEADERS
    for name, value in (("COHORT_PER_ROW", 0), ("COHORT_PER_COLUMN", 1), ("NORM_Z", 0), ("NORM_T", 1), ("NORM_S", 2)):
        assert re.search(r"#define DSP_%s %d\b" % (name, value), header) and getattr(dl, name) == value
    assert (R.PER_ROW, R.PER_COLUMN, R.NORM_Z, R.NORM_T, R.NORM_S) == (0, 1, 0, 1, 2) and dl.NORM_MODES == R.MODES


def test_ctypes_mirrors_match_the_header_and_the_kernels_constants_the_restatement():
    assert C.sizeof(dl.CohortStat) == 32 and C.sizeof(dl.SnormConfig) == 16
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "capi_snorm.cpp")) as f:
        src = f.read()
    assert "static_assert(sizeof(dsp_cohort_stat) == 32" in src and "static_assert(sizeof(dsp_snorm_config) == 16" in src
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    for struct, mirror in (("dsp_cohort_stat", dl.CohortStat), ("dsp_snorm_config", dl.SnormConfig)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        names = [n for line in body.split(";") for n in re.sub(r"/\*.*?\*/", "", line, flags=re.S).replace(",", " ").split()[1:]]
        assert names == [f[0] for f in mirror._fields_], struct
    assert [f[0] for f in dl.CohortStat._fields_] == list(R.STAT_DTYPE.names) == [n for n, _ in dl.COHORT_STAT_DTYPE]
    assert [C.sizeof(f[1]) for f in dl.CohortStat._fields_] == [R.STAT_DTYPE[n].itemsize for n in R.STAT_DTYPE.names]
    with open(os.path.join(ROOT, "dsp_amd", "csrc", "snorm_kernels.hpp")) as f:
        hpp = f.read()

    def const(name):
        return eval(re.search(r"constexpr \w+ %s = ([^;]+);" % name, hpp).group(1).replace("L", ""), {})      # noqa: S307  (our own header: "1L << 22")

    assert (const("kSnormChunk"), const("kSnormMaxLength"), const("kSnormMaxVectors"), const("kSnormMaxTopK")) == (R.CHUNK, R.MAX_LENGTH, R.MAX_VECTORS, 1 << 22)
    assert dl.COHORT_MAX_LENGTH == R.MAX_LENGTH
    # the shared cases reach every form: resident and re-read vectors, the narrow and the tiled column form, a ragged last tile
    assert const("kSnormResident") == 32 * 1024 and max(U.LENGTHS) > const("kSnormResident") >= sorted(U.LENGTHS)[-2]
    assert min(U.VECTORS) < const("kSnormLanesAcrossColumns") <= 63 and const("kSnormTileColumns") == 64 and {63, 64, 65, 130} <= set(U.VECTORS)


def test_the_python_layer_refuses_before_any_call():
    import torch
    with dsp_amd.ScoreNormalizer() as n:
        x = torch.zeros((3, 2))
        for call in (lambda: n.stats(x, "row"), lambda: n.stats(x.double(), "row"), lambda: n.apply(x, "z", col_stats=torch.zeros((2, 4), dtype=torch.int64)),
                     lambda: n.normalize(x, mode="t", row_cohort=x)):
            with pytest.raises(ValueError, match="float32 CUDA tensor"):
                call()
        with pytest.raises(ValueError, match="axis"):
            n.stats(x, "both")
        with pytest.raises(ValueError, match="top_k"):
            n.stats(x, "row", -1)
        with pytest.raises(ValueError, match="mode"):
            n.apply(x, "q")
        with pytest.raises(ValueError, match="std_floor"):
            n.apply(x, "z", std_floor=float("nan"))
    assert n._L is None
    n.close()                                                                         # a second close does nothing; a closed object refuses
    for call in (lambda: n.stats(x, "row"), lambda: n.apply(x, "q"), lambda: n.normalize(x, mode="q")):      # closed comes before any argument
        with pytest.raises(dl.DspError, match="closed"):
            call()
    with pytest.raises(ValueError, match="device"):
        dsp_amd.ScoreNormalizer(-1)
