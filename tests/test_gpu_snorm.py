"""GPU: cohort normalisation (dsp_cohort_stats_device, dsp_score_normalize_device; dsp_amd.ScoreNormalizer) against the
float64 restatement tests/snorm_ref.py, bit for bit, and against the independent numpy form within the derived gate of
tests/snorm_util.py.  Every output buffer is pre-filled with a sentinel and followed by spare entries that must keep it.  The float64
sqrt and division of the device are correctly rounded: `std` is held to the same bits as `mean`."""
import numpy as np
import pytest

from tests import enroll_ref as E
from tests import snorm_ref as R
from tests import snorm_util as U
from tests import verify_util as VU

pytestmark = pytest.mark.gpu

SPARE = 3


@pytest.fixture(scope="module")
def norm():
    import torch
    import dsp_amd
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    with dsp_amd.ScoreNormalizer() as n:
        yield n


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C", copy=True)).cuda()                  # (the shared cases are read-only)


def _raw_stats(norm, x, axis, top_k):
    """dsp_cohort_stats_device into a sentinel-filled buffer with SPARE records behind the last -> the records on the host"""
    import torch
    from dsp_amd import lib as dl
    vectors = x.shape[0] if axis == R.PER_ROW else x.shape[1]
    buf = torch.full((vectors + SPARE, 4), U.SENTINEL, dtype=torch.int64, device=x.device)
    rc = norm._L.dsp_cohort_stats_device(norm.device, x.data_ptr(), x.shape[0], x.shape[1], axis, top_k, buf.data_ptr(), dl.current_stream(x))
    assert rc == 0, dl.last_error()
    host = buf.cpu().numpy()
    assert (host[vectors:] == U.SENTINEL).all(), "a record was written past the last vector"
    assert not (host[:vectors, 3] == U.SENTINEL).any(), "a record was not written"
    return host[:vectors].copy().view(R.STAT_DTYPE).reshape(-1)


def _records_dev(rec):
    """host records -> the int64 CUDA tensor [V][4] ScoreNormalizer.apply takes"""
    return _dev(np.ascontiguousarray(rec).view(np.int64).reshape(-1, 4))


def _raw_apply(norm, x, mode, row, col, floor):
    """dsp_score_normalize_device into a sentinel-filled flat buffer with SPARE floats behind the last -> the outputs on the host"""
    import ctypes as C
    import torch
    from dsp_amd import lib as dl
    T, S = x.shape
    buf = torch.full((T * S + SPARE,), -7.25, dtype=torch.float32, device=x.device)
    cfg = dl.SnormConfig(mode, 0, floor)
    rc = norm._L.dsp_score_normalize_device(norm.device, x.data_ptr(), T, S, row.data_ptr() if row is not None else None,
                                            col.data_ptr() if col is not None else None, C.byref(cfg), buf.data_ptr(), dl.current_stream(x))
    assert rc == 0, dl.last_error()
    host = buf.cpu().numpy()
    assert (host[T * S:] == -7.25).all(), "an output was written past the last trial"
    return host[:T * S].reshape(T, S)


def _same_outputs(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("n", U.LENGTHS)
def test_records_equal_the_restatement_on_both_axes(norm, n):
    """All six fields, bit for bit, for reduced lengths at the tile and chunk edges of the tree (and 33 000, the first form past the
    LDS-resident one), vector counts at the edges of the column tile and in the narrow form, and every top_k of snorm_util.top_ks."""
    x = U.cohort(n)
    rows = _dev(x)
    for vectors in U.VECTORS:
        by_row, by_col = rows[:vectors], rows[:vectors].T.contiguous()
        for k in U.top_ks(n):
            want = U.records(x, k, ("cohort", n))[:vectors]
            assert U.same_bits(_raw_stats(norm, by_row, R.PER_ROW, k), want) is None, (n, vectors, k, "row")
            assert U.same_bits(_raw_stats(norm, by_col, R.PER_COLUMN, k), want) is None, (n, vectors, k, "column")


@pytest.mark.parametrize("n", [5, 300, 4100])
def test_records_of_the_special_vectors(norm, n):
    """NaN, +inf, -inf, -0 / +0, an all-NaN vector, an all-equal one (sigma = 0), a plateau of ties wider than K, in the narrow and
    the tiled column form and per row"""
    x = U.special(n)
    rows = _dev(x)
    for vectors in (12, 70):
        by_row, by_col = rows[:vectors], rows[:vectors].T.contiguous()
        for k in sorted({0, 1, 3, n - 1, 300}):
            want = U.records(x, k, ("special", n))[:vectors]
            assert want["n_finite"][2] == 0 and want["std"][3] == 0.0 and want["n_selected"][4] - want["n_above"][4] >= 1
            assert U.same_bits(_raw_stats(norm, by_row, R.PER_ROW, k), want) is None, (n, vectors, k, "row")
            assert U.same_bits(_raw_stats(norm, by_col, R.PER_COLUMN, k), want) is None, (n, vectors, k, "column")


@pytest.mark.parametrize("shape", [(130, 65), (4097, 3)])
def test_per_column_equals_per_row_of_the_transpose(norm, shape):
    x = _dev(U.cohort(shape[1], shape[0], seed=5))                                   # [130][65] and [4097][3]
    for k in (0, 7):
        a, b = _raw_stats(norm, x, R.PER_COLUMN, k), _raw_stats(norm, x.T.contiguous(), R.PER_ROW, k)
        assert a.size == shape[1] and U.same_bits(a, b) is None, (shape, k)


def test_a_record_depends_on_its_vector_alone(norm):
    import torch
    n, at, k = 1000, 17, 300
    x = U.cohort(n, 65, seed=3)
    want = R.stats(x[at:at + 1], R.PER_ROW, k)
    others = U.cohort(n, 65, seed=4).copy()
    others[at] = x[at]                                                                # the vectors around it replaced
    moved = np.stack([x[at]] + [others[i] for i in range(64)])                        # and the vector at another position
    for axis, lay in ((R.PER_ROW, lambda m: _dev(m)), (R.PER_COLUMN, lambda m: _dev(m.T))):
        first = _raw_stats(norm, lay(x), axis, k)[at:at + 1]
        assert U.same_bits(first, want) is None
        assert U.same_bits(_raw_stats(norm, lay(others), axis, k)[at:at + 1], want) is None
        assert U.same_bits(_raw_stats(norm, lay(moved), axis, k)[:1], want) is None
        assert U.same_bits(_raw_stats(norm, lay(x[at:at + 1]), axis, k), want) is None
        _raw_stats(norm, lay(U.cohort(8193, 130)), axis, 0)                           # a larger call in between: guards a later workspace
        assert U.same_bits(_raw_stats(norm, lay(x), axis, k)[at:at + 1], want) is None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = _raw_stats(norm, lay(x), axis, k)[at:at + 1]
        assert U.same_bits(on_side, want) is None


@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (65, 130), (130, 65)])
def test_apply_equals_the_restatement(norm, shape):
    """all three modes, std_floor 0 and 1e-6, into `out` and in place; NaN scores and statistics with n_finite == 0 give NaN"""
    T, S = shape
    sc = U.scores(T, S).copy()
    sc[0, 0] = np.nan if T * S > 1 else sc[0, 0]
    row = R.stats(U.special(40, 130)[:T], R.PER_ROW, 5)
    col = R.stats(U.special(33, 130, seed=2)[:S], R.PER_ROW, 0)
    assert T <= 3 or (row["n_finite"][2] == 0 and row["std"][3] == 0.0)
    x, d_row, d_col = _dev(sc), _records_dev(row), _records_dev(col)
    for name, mode in R.MODES.items():
        for floor in (0.0, 1e-6):
            want = R.apply(sc, mode, row, col, floor)
            use_row, use_col = (d_row if mode != R.NORM_Z else None), (d_col if mode != R.NORM_T else None)
            assert _same_outputs(_raw_apply(norm, x, mode, use_row, use_col, floor), want), (shape, name, floor)
            assert _same_outputs(norm.apply(x, name, use_row, use_col, floor).cpu().numpy(), want), (shape, name, floor)
            inplace = x.clone()
            assert norm.apply(inplace, name, use_row, use_col, floor, out=inplace) is inplace
            assert _same_outputs(inplace.cpu().numpy(), want), (shape, name, floor, "in place")
            if T >= 3:
                assert np.isnan(want[2]).all() or mode == R.NORM_Z
    assert np.isnan(R.apply(sc, R.NORM_S, row, col, 1e-6)[0, 0]) or T * S == 1


@pytest.mark.parametrize("n", U.LENGTHS)
def test_against_the_independent_numpy_form(norm, n):
    """The device's records and outputs against np.sort(finite values as float64)[-K':], .mean() and .std(): the threshold and the
    counts exactly, every output of every mode within |got - ind| <= 1 float32 ulp of ind + 2^-40 (|x| + |mean|) / sigma'."""
    x = U.special(n, 130) if n >= 5 else U.cohort(n, 130)
    rows_of, cols_of = x[:65], x[65:]
    d_rows, d_cols = _dev(rows_of), _dev(cols_of.T)
    sc = U.scores(65, 65, n)
    d_sc = _dev(sc)
    for k in U.top_ks(n):
        row, col = norm.stats(d_rows, "row", k), norm.stats(d_cols, "column", k)
        ind = [U.independent_records(src, k) for src in (rows_of, cols_of)]
        for got, (mean, std, theta, nf, ns, na) in zip((norm.stats_to_numpy(row), norm.stats_to_numpy(col)), ind):
            assert np.array_equal(got["threshold"].view(np.uint32), theta.view(np.uint32)), (n, k)
            assert np.array_equal(got["n_finite"], nf) and np.array_equal(got["n_selected"], ns) and np.array_equal(got["n_above"], na), (n, k)
        ind_row, ind_col = ind[0][:2], ind[1][:2]
        for name, mode in R.MODES.items():
            out = norm.apply(d_sc, name, row if name != "z" else None, col if name != "t" else None, 1e-6).cpu().numpy()
            misses = U.gate_misses(out, sc, mode, ind_row, ind_col, 1e-6)
            print(n, k, name, "outputs outside the gate:", misses, "of", out.size)
            assert misses == 0, (n, k, name)


def test_end_to_end_on_the_verifier_s_scores(norm):
    """a random UBM (k = 4, d = 3), 3 enrolled and 5 cohort speakers, 6 trial and 7 cohort clips of 20 .. 90 rows: three verifier calls,
    normalize(mode="s", top_k=3) = the restatement on the verifier's own outputs, and the evaluator and the calibrator take it"""
    import dsp_amd
    rng = np.random.default_rng(4242)
    ubm = E.random_ubm(rng, 4, 3)
    speakers = [E.draw_speaker(rng, ubm, 200, 0.6) for _ in range(8)]
    means = _dev(np.stack([E.enroll(s, ubm)["means"] for s in speakers]).astype(np.float32))
    enrolled, cohort_speakers = means[:3].contiguous(), means[3:].contiguous()

    def clips(count, seed):
        r = np.random.default_rng(seed)
        lens = r.integers(20, 91, count)
        rows = [E.draw_speaker(r, ubm, int(m), 0.6) for m in lens]
        return _dev(np.concatenate(rows)), VU.offsets(lens)

    trial, trial_fo = clips(6, 1)
    cohort_clips, cohort_fo = clips(7, 2)
    with dsp_amd.SpeakerVerifier(ubm) as v:
        scores = v.verify(trial, trial_fo, enrolled, want=("llr",))["llr"]
        row_cohort = v.verify(trial, trial_fo, cohort_speakers, want=("llr",))["llr"]
        col_cohort = v.verify(cohort_clips, cohort_fo, enrolled, want=("llr",))["llr"]
    assert scores.shape == (6, 3) and row_cohort.shape == (6, 5) and col_cohort.shape == (7, 3)
    out = norm.normalize(scores, row_cohort, col_cohort, mode="s", top_k=3)
    want = R.apply(scores.cpu().numpy(), R.NORM_S, R.stats(row_cohort.cpu().numpy(), R.PER_ROW, 3), R.stats(col_cohort.cpu().numpy(), R.PER_COLUMN, 3), 1e-6)
    assert out.shape == (6, 3) and np.isfinite(want).all() and _same_outputs(out.cpu().numpy(), want)
    for mode, kwargs in (("z", dict(col_cohort=col_cohort)), ("t", dict(row_cohort=row_cohort))):
        assert norm.normalize(scores, mode=mode, **kwargs).shape == (6, 3)
    truth = [0, 1, 2, -1, 0, 1]
    with dsp_amd.TrialEvaluator() as ev:
        res = ev.evaluate(out, truth, n_thresholds=16, want=("columns",))
    assert int(res["columns"]["n_target"][-1]) == 5 and int(res["columns"]["n_nan"][-1]) == 0
    with dsp_amd.ScoreCalibrator() as cal:
        assert np.array_equal(cal.apply(out, (1.0, 0.0, 0.0)).cpu().numpy(), out.cpu().numpy() + np.float32(0.0))


def test_the_python_layer_refuses_before_any_launch_and_closes_once(norm):
    import torch
    import dsp_amd
    x = _dev(U.scores(4, 3))
    row, col = norm.stats(_dev(U.cohort(9, 4)), "row"), norm.stats(_dev(U.cohort(9, 3)).T.contiguous(), "column")
    assert row.shape == (4, 4) and col.shape == (3, 4) and row.dtype == torch.int64
    host = norm.stats_to_numpy(col)
    assert sorted(host) == sorted(R.STAT_DTYPE.names) and host["mean"].dtype == np.float64 and host["n_finite"].tolist() == [9, 9, 9]
    bad = [lambda: norm.apply(x.cpu(), "s", row, col), lambda: norm.apply(x.double(), "s", row, col), lambda: norm.apply(x[0], "s", row, col),
           lambda: norm.apply(x, "s", row_stats=row), lambda: norm.apply(x, "s", col_stats=col), lambda: norm.apply(x, "z", row_stats=row),
           lambda: norm.apply(x, "t", col_stats=col), lambda: norm.apply(x, "s", col, row), lambda: norm.apply(x, "s", row.cpu(), col),
           lambda: norm.apply(x, "s", row.float(), col), lambda: norm.apply(x, "s", row, col, out=torch.empty((3, 4), device="cuda")),
           lambda: norm.apply(x, "s", row, col, std_floor=-1.0), lambda: norm.apply(x, "both", row, col),
           lambda: norm.stats(x, "diagonal"), lambda: norm.stats(x, "row", top_k=(1 << 22) + 1), lambda: norm.stats(x.cpu(), "row"),
           lambda: norm.stats(torch.empty((3, 0), device="cuda"), "row"), lambda: norm.stats(x.reshape(-1), "row"),
           lambda: norm.normalize(x, mode="s", row_cohort=x), lambda: norm.normalize(x, mode="t"), lambda: norm.normalize(x, mode="z", row_cohort=x),
           lambda: norm.normalize(x, _dev(U.cohort(9, 5)), None, mode="t"), lambda: norm.normalize(x, None, _dev(U.cohort(4, 9)), mode="z")]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} was accepted")
    assert norm.stats(torch.empty((0, 5), device="cuda"), "row").shape == (0, 4)       # no vector: nothing launched
    assert norm.apply(torch.empty((0, 3), device="cuda"), "z", col_stats=col).shape == (0, 3)
    with dsp_amd.ScoreNormalizer() as fresh:                                          # `with` and close() twice, as tests/test_gpu_handles.py asks of the handle classes
        assert fresh._L is not None and fresh.device == 0
        assert fresh.stats(x, "row").shape == (4, 4)
    assert fresh._L is None
    fresh.close()
    fresh.__del__()
    assert fresh._L is None
    with pytest.raises(dsp_amd.DspError, match="closed"):
        fresh.apply(x, "z", col_stats=col)
