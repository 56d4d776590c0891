"""CPU: what tests/test_gpu_resample_shapes.py relies on, checked without a GPU -- every name of tests/resample_shapes.py in its pinned
class through dsp_resample_geometry, the geometry's invariants and the staging boundary over a sweep of ratios, every class of the sweep
under a name, the stream resampler's refusal of exactly the unstaged ratios, the numpy restatement against scipy.signal.resample_poly on
the names' own recordings, the impulse recordings against the restatement, and the tight gate against mutants of the float32 model."""
import ctypes as C
import math

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import resample_ref as R
from tests import resample_shapes as RS

SWEEP_UPS = [1, 2, 3, 4, 5, 7, 8, 16, 64, 160, 255, 441, 640, 1023, 1024]
LDS_BUDGET = 40 * 1024


@pytest.fixture(scope="module")
def sweep():
    """[(up, down, geometry)]: every up of SWEEP_UPS with every coprime down <= 1024, the copy left out"""
    out = []
    for up in SWEEP_UPS:
        for down in range(1, 1025):
            if math.gcd(up, down) == 1 and (up, down) != (1, 1):
                out.append((up, down, dsp_amd.resample_geometry(down, up)))
    return out


def test_geometry_query_counts_its_fields_and_refuses_what_the_ratio_refuses():
    L = dl.load()
    n = len(dsp_amd.resample.GEOMETRY_FIELDS)
    v = (C.c_int * n)()
    assert L.dsp_resample_geometry(48000, 16000, None, 0) == n == L.dsp_resample_geometry(48000, 16000, v, n)
    assert list(v) == [1, 3, 30, 61, 64, 2048, 512, 6205, 1, 33076]
    assert L.dsp_resample_geometry(48000, 16000, v, n - 1) == -1 and "fields" in dl.last_error()
    for ri, ro in ((0, 16000), (16000, -5), (1, 1025), (44101, 16000)):
        assert L.dsp_resample_geometry(ri, ro, None, 0) == -1 and dl.last_error() != ""
    g = dsp_amd.resample_geometry(44100, 16000)
    assert (g["up"], g["down"], g["half"]) == dsp_amd.resample_ratio(44100, 16000) == R.ratio(44100, 16000)
    with pytest.raises(ValueError):
        dsp_amd.resample_geometry(48000.0, 16000)


@pytest.mark.parametrize("name", RS.NAMES)
def test_every_name_is_in_its_class(name):
    rate_in, rate_out, want = RS.SHAPES[name]
    g = dsp_amd.resample_geometry(rate_in, rate_out)
    assert RS.class_of(g) == want, (name, g)
    assert (g["up"], g["down"], g["half"]) == R.ratio(rate_in, rate_out)


def test_sweep_geometry_invariants_and_the_staging_boundary(sweep):
    first_unstaged = {}
    for up, down, g in sweep:
        half = 10 * max(up, down)
        taps = (2 * half + up) // up
        row = (taps + 3) & ~3
        span_of = lambda tile: ((tile - 1) * down + up - 1) // up + row       # noqa: E731
        what = (up, down, g)
        assert (g["up"], g["down"], g["half"], g["taps"], g["row"]) == (up, down, half, taps, row), what
        assert g["tile"] == 4 * g["items"] and g["items"] % up == 0 and g["tile"] % 4 == 0 and 4 <= g["tile"] <= 4096, what
        assert g["span"] == span_of(g["tile"]), what
        assert g["lds_bytes"] <= LDS_BUDGET, what
        assert g["lds_bytes"] == ((g["tile"] + g["span"] + 16) * 4 if g["staged"] else g["tile"] * 4), what
        # unstaged exactly where one lane group (4 up outputs) with its span is already past the budget
        one_group = (4 * up + span_of(4 * up) + 16) * 4
        assert g["staged"] == (1 if one_group <= LDS_BUDGET else 0), what
        if not g["staged"]:
            first_unstaged.setdefault(up, down)
            assert first_unstaged[up] <= down                                 # (and every longer branch behind it)
            assert g["items"] == up * max(1, 1024 // (4 * up)), what
    assert first_unstaged == {1: 445, 2: 757, 3: 989}
    for up, down, g in sweep:
        assert g["staged"] == (0 if up in first_unstaged and down >= first_unstaged[up] else 1), (up, down)


def test_every_class_of_the_sweep_has_a_name(sweep):
    """(form x how the items fill the 256 lanes): a class no name stands for would never run on a GPU under test"""
    named = {(want[0], RS.items_class(want[2])) for _ri, _ro, want in RS.SHAPES.values()}
    seen = {}
    for up, down, g in sweep:
        seen.setdefault((RS.form_of(g), RS.items_class(g["items"])), (down, up))
    missing = {k: v for k, v in seen.items() if k not in named}
    assert not missing, f"classes without a name in tests/resample_shapes.py (class: first rate_in -> rate_out): {missing}"
    assert named <= set(seen)


def test_live_streams_refuse_exactly_the_unstaged_ratios(sweep):
    """before any device work: n_streams = -1 is the next refusal behind the branch-too-long one"""
    create = dl.load().dsp_stream_resampler_create
    h = C.c_void_p(1)
    for up, down, g in sweep:
        if not (up <= 3 or down % 97 == 0):              # every ratio at the ups that have a boundary, a sample of the others
            continue
        assert create(0, down, up, -1, 1, 0, 0, C.byref(h)) == -1
        msg = dl.last_error()
        if g["staged"]:
            assert "taps per output" not in msg and "n_streams" in msg, (up, down, msg)
        else:
            assert f"{g['taps']} taps per output" in msg and "not a live-feed ratio" in msg, (up, down, msg)
    assert create(0, 445, 1, -1, 1, 0, 0, C.byref(h)) == -1 and "8901 taps per output" in dl.last_error()
    assert create(0, 444, 1, -1, 1, 0, 0, C.byref(h)) == -1 and "taps per output" not in dl.last_error()
    assert h.value is None


@pytest.mark.parametrize("name", RS.NAMES)
def test_lengths_reach_the_tile_edges(name):
    rate_in, rate_out, (_form, tile, _items, taps) = RS.SHAPES[name]
    up, down, _half = R.ratio(rate_in, rate_out)
    ns = RS.lengths(name)
    outs = [R.out_len(n, up, down) for n in ns]
    assert ns[:3] == [0, 1, 7] and 7 < taps and len(set(ns)) == len(ns)
    assert max(outs) >= RS.GATE_MIN_OUTPUTS
    if name == "unstaged_longest":
        assert outs == [0, 1, 1, 3, 5, 67]                  # (one sample and seven are one output each)
        return
    wanted = (tile + 1, tile - 1) if name in RS.BUDGETED else (tile - 1, tile, tile + 1, 2 * tile + 3)
    for k in wanted:
        # the smallest reachable output length >= k is there (k itself wherever up <= down)
        reach = R.out_len(RS.n_for_outputs(k, up, down), up, down)
        assert reach in outs and reach >= k and R.out_len(RS.n_for_outputs(k, up, down) - 1, up, down) < k and (up > down or reach == k), (name, k)
    if name in RS.BUDGETED:
        assert sum(ns) <= RS.INPUT_BUDGET + 67 * down
    assert any(o > tile for o in outs) and any(0 < o < tile for o in outs)


@pytest.mark.parametrize("name", RS.NAMES)
def test_restatement_is_resample_poly_on_the_names_recordings(name):
    """as test_restatement_is_resample_poly of tests/test_resample_cpu.py, its gate unchanged (16 x 8.9e-16), on the recordings the GPU
    tests use.  Worst seen over the names: 8.9e-16 (16000 -> 44100)."""
    from scipy.signal import resample_poly
    rate_in, rate_out = RS.rates(name)
    up, down, _half = R.ratio(rate_in, rate_out)
    worst = 0.0
    for (_raw, x), (ref, _bound, _model) in zip(RS.recordings(name), RS.references(name)):
        want = resample_poly(x.astype(np.float64), up, down)
        assert ref.shape == want.shape == (R.out_len(x.size, up, down),)
        if x.size:
            worst = max(worst, float(np.abs(ref - want).max()))
    print(f"restatement on {name}: {worst:.2e}")
    assert worst <= 16 * 8.9e-16


@pytest.mark.parametrize("name", RS.NAMES)
def test_impulse_recordings_give_the_taps(name):
    """the expected impulse response is written from the library's float64 taps directly: held here, bit for bit, to the restatement
    run with those taps, and the taps to the restatement's own under the gate of test_taps_are_firwin_times_up (16 x 9.2e-16 of the
    largest tap)"""
    rate_in, rate_out = RS.rates(name)
    x, want, single, ref, bound = RS.impulses(name)
    h = dsp_amd.resample_taps(rate_in, rate_out)
    assert np.abs(h - R.taps(rate_in, rate_out)).max() <= 16 * 9.2e-16 * np.abs(h).max()
    model = R.resample(x, rate_in, rate_out, dtype=np.float32, h64=h)
    assert model.dtype == want.dtype == np.float32 and np.array_equal(model, want)
    assert np.array_equal(ref, R.resample(x, rate_in, rate_out, h64=h))
    assert np.all(np.abs(want.astype(np.float64) - ref) <= bound)
    _form, tile, _items, taps = RS.SHAPES[name][2]
    assert want.size > tile or name == "unstaged_longest"
    assert np.count_nonzero(want) >= 2
    # a recording longer than two branches keeps the impulses apart: most outputs are one tap (up1024's 9 samples are shorter than one)
    assert single.sum() >= 0.5 * want.size if x.size > 2 * taps else name == "up1024"
    h32 = h.astype(np.float32)
    assert set(np.unique(want[single])) <= set(np.unique(h32)) | {np.float32(0.0)}


@pytest.mark.parametrize("name", RS.NAMES)
def test_the_float32_model_passes_both_gates(name):
    gated = 0
    for (_raw, x), (ref, bound, model) in zip(RS.recordings(name), RS.references(name)):
        if model is None:
            assert ref.size < RS.GATE_MIN_OUTPUTS
            continue
        gated += 1
        assert np.all(np.abs(model.astype(np.float64) - ref) <= bound)
        assert RS.gate_ratio(model, ref, model) == 1.0 <= RS.MARGIN
        # the float64 reference's own error is nowhere near the float32 floor the gate is scaled by
        assert RS.gate_ratio(ref, ref, model) == 0.0
    assert gated >= 1


@pytest.mark.parametrize("name", RS.LONG_NAMES)
def test_the_tight_gate_rejects_mutants_of_the_model(name):
    """One defect each on the float32 model; every one must fail rms(err) <= MARGIN rms(model err), with room: the issue's sidelobe
    mutant measured 117 - 480 times the model's rms.  What the per-output bound alone makes of the same mutant is printed beside it."""
    assert RS.SHAPES[name][2][3] > 200
    refs = RS.references(name)
    idx = max((i for i, r in enumerate(refs) if r[2] is not None), key=lambda i: refs[i][0].size)
    x = RS.recordings(name)[idx][1]
    ref, bound, model = refs[idx]
    up = R.ratio(*RS.rates(name))[0]
    muts = RS.mutants(name, x)
    assert set(muts) == {"sidelobe_tap_zeroed", "one_sample_late"} | ({"next_branch"} if up > 1 else set())
    for what, y in muts.items():
        ratio = RS.gate_ratio(y, ref, model)
        of_bound = float((np.abs(y.astype(np.float64) - ref) / np.where(bound > 0, bound, np.inf)).max())
        print(f"{name} {what}: {ratio:.0f} x the model's rms error; worst output at {of_bound:.3f} of the per-output bound")
        assert ratio > 32, (name, what, ratio)          # 8 times past the largest margin the gate may ever take (4)
