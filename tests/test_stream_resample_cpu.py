"""CPU: the host side of the streaming resampler (include/dsp_amd.h dsp_stream_resample*) -- K(N) and the carry's length against a
brute-force loop, dsp_stream_resample_plan (no GPU call) against K(N), a numpy model of push / carry / finish held bit for bit to the
whole recording (tests/stream_resample_ref.py), the refusals made before any device work in the header's order, the exports, and the
Python wrappers' checks under python -O.  (What dsp_stream_session_attach_resampler refuses between two live objects needs a device to
create them: tests/test_gpu_stream_resample.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl
from tests import resample_ref as R
from tests import stream_resample_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dsp_stream_resample_plan", "dsp_stream_resampler_create", "dsp_stream_resampler_destroy", "dsp_stream_resampler_reset",
           "dsp_stream_resampler_counts", "dsp_stream_resample_push_device", "dsp_stream_resample_finish_device",
           "dsp_stream_session_attach_resampler"]
LP = C.POINTER(C.c_long)
EINVAL = -1
COUNTS = list(range(400)) + [1000, 1023, 1024, 4095, 4097, 5200, 44100, 48000, 96001]
# the pairs whose carry reaches T - 1 sample frames, and that T - 1
FULL_CARRY = {(10000, 16000): 20, (44100, 16000): 55, (48000, 16000): 60, (96000, 16000): 120}


def _c_plan(rate_in, rate_out, received, co):
    """the C planner, raw: (return value, out_offsets)"""
    co = np.ascontiguousarray(co, np.int64)
    n = co.size - 1
    rec = np.ascontiguousarray(received, np.int64) if received is not None else None
    oo = np.full(n + 1, -7, np.int64)
    rc = dl.load().dsp_stream_resample_plan(rate_in, rate_out, rec.ctypes.data_as(LP) if rec is not None else None, co.ctypes.data_as(LP), n,
                                            oo.ctypes.data_as(LP))
    return rc, oo


@pytest.mark.parametrize("rate_in,rate_out", R.RATE_PAIRS)
def test_emitted_and_carry_against_brute_force(rate_in, rate_out):
    up, down, half = R.ratio(rate_in, rate_out)
    T = S.taps_per_branch(up, half)
    longest = 0
    for n in COUNTS:
        k = S.emitted(n, up, down, half)
        if (up, down) == (1, 1):
            assert k == n and S.carry_start(n, up, down, half) == n
            continue
        assert k == S.emitted_brute(n, up, down, half), n
        # exactly the outputs whose last sample has arrived, and never more than a whole recording of n samples has
        assert k == 0 or S.i_max(k - 1, up, down, half) <= n - 1 < S.i_max(k, up, down, half)
        assert k <= R.out_len(n, up, down)
        carried = n - S.carry_start(n, up, down, half)
        assert 0 <= carried <= T - 1, (n, carried)
        longest = max(longest, carried)
        # the C planner agrees: one stream, nothing received, one chunk of n
        rc, oo = _c_plan(rate_in, rate_out, None, [3, 3 + n])
        assert rc == k and oo.tolist() == [0, k]
    if (rate_in, rate_out) in FULL_CARRY:
        assert longest == T - 1 == FULL_CARRY[(rate_in, rate_out)]


@pytest.mark.parametrize("rate_in,rate_out", R.RATE_PAIRS)
def test_planner_follows_k(rate_in, rate_out):
    up, down, half = R.ratio(rate_in, rate_out)
    rng = np.random.default_rng(rate_in)
    n = 23
    received = np.zeros(n, np.int64)
    for _push in range(40):
        lengths = rng.integers(0, 900, n)
        lengths[rng.integers(0, n, 6)] = 0
        lengths[rng.integers(0, n, 3)] = 1
        co = np.concatenate([[rng.integers(0, 9)], lengths]).cumsum()
        want = S.push_plan(received, lengths, up, down, half)
        rc, oo = _c_plan(rate_in, rate_out, received, co)
        assert rc == want[-1]
        np.testing.assert_array_equal(oo, want)
        np.testing.assert_array_equal(dsp_amd.stream_resample_plan(rate_in, rate_out, received, co), want)
        received = received + lengths
    # the pushes of a stream add up to K of what it received
    assert [S.emitted(int(r), up, down, half) for r in received] == [int(_c_plan(rate_in, rate_out, None, [0, int(r)])[0]) for r in received]
    # received = NULL is "nothing yet"; n = 0 needs no chunk_offsets
    rc, oo = _c_plan(rate_in, rate_out, None, [0, 400, 400, 1000])
    assert oo.tolist() == [0] + np.cumsum([S.emitted(400, up, down, half), 0, S.emitted(600, up, down, half)]).tolist() and rc == oo[-1]
    out = (C.c_long * 1)(-7)
    assert dl.load().dsp_stream_resample_plan(rate_in, rate_out, None, None, 0, out) == 0 and out[0] == 0


def test_planner_refusals():
    L = dl.load()
    good = [0, 100, 500]
    assert _c_plan(10000, 16000, [0, 0], good)[0] == S.emitted(100, 8, 5, 80) + S.emitted(400, 8, 5, 80)
    for ri, ro in ((0, 16000), (16000, 0), (1, 1025), (1025, 1), (44101, 16000)):
        assert _c_plan(ri, ro, None, good)[0] == EINVAL
    assert "1024" in dl.last_error()
    co = np.array(good, np.int64)
    oo = np.zeros(3, np.int64)
    assert L.dsp_stream_resample_plan(10000, 16000, None, None, 2, oo.ctypes.data_as(LP)) == EINVAL
    assert L.dsp_stream_resample_plan(10000, 16000, None, co.ctypes.data_as(LP), 2, None) == EINVAL
    assert L.dsp_stream_resample_plan(10000, 16000, None, co.ctypes.data_as(LP), -1, oo.ctypes.data_as(LP)) == EINVAL
    assert _c_plan(10000, 16000, [0, 0], [0, 500, 100])[0] == EINVAL and "stream 1" in dl.last_error()
    assert _c_plan(10000, 16000, [0, 0], [-1, 100, 500])[0] == EINVAL
    assert _c_plan(10000, 16000, [0, -1], good)[0] == EINVAL and "received" in dl.last_error()
    assert _c_plan(10000, 16000, [0, 0], [0, 100, 2**31 + 100])[0] == EINVAL
    assert _c_plan(10000, 16000, [0, 2**62], good)[0] == EINVAL and "overflow" in dl.last_error()


@pytest.mark.parametrize("rate_in,rate_out", R.RATE_PAIRS)
def test_model_chunked_is_whole_bit_for_bit(rate_in, rate_out):
    """any chunking: pushes give the first K(N) outputs of the whole recording, finish the rest -- chunks of 0, of 1 and of fewer
    frames than the carry included (T - 2, T - 1, T)"""
    up, down, half = R.ratio(rate_in, rate_out)
    T = S.taps_per_branch(up, half)
    rng = np.random.default_rng(99 + rate_in)
    for total in (0, 1, T - 1, 3 * T + 7, 2500):
        x = rng.uniform(-1, 1, total).astype(np.float32)
        whole = R.resample(x, rate_in, rate_out, dtype=np.float32)
        for _trial in range(2):
            m = S.StreamModel(rate_in, rate_out)
            got, seen = [], 0
            for c in S.chunking(total, rng, [max(T - 2, 0), T - 1, T]) + [0]:
                got.append(m.push(x[seen:seen + c]))
                seen += c
                emitted = sum(g.size for g in got)
                assert emitted == S.emitted(seen, up, down, half)
                assert np.array_equal(np.concatenate(got).view(np.uint32), whole[:emitted].view(np.uint32)), (total, seen)
            got.append(m.finish())
            assert np.array_equal(np.concatenate(got).view(np.uint32), whole.view(np.uint32)), total
            assert m.longest_carry <= max(T - 1, 0) and m.n == 0


def _refused(rc, *words):
    assert rc == EINVAL, (rc, dl.last_error())
    for w in words:
        assert w in dl.last_error(), (w, dl.last_error())


def test_entries_refuse_in_the_headers_order_before_any_device_work():
    L = dl.load()
    h = C.c_void_p(1)
    create = L.dsp_stream_resampler_create
    # out NULL, before everything else
    _refused(create(0, 0, 16000, -1, 3, 0, 1, None), "out is NULL")
    # a bad PCM layout, before the rates
    _refused(create(0, 0, 16000, 4, 3, 0, 1, C.byref(h)), "channels")
    assert h.value is None
    _refused(create(0, 0, 16000, 4, 2, 7, 1, C.byref(h)), "stereo_mode")
    _refused(create(0, 0, 16000, 4, 2, 0, 0, C.byref(h)), "float samples are mono")
    # the rates, before the shape
    _refused(create(0, 0, 16000, 4, 1, 0, 0, C.byref(h)), "rate_in")
    _refused(create(0, 1025, 1, -1, 1, 0, 0, C.byref(h)), "1024")
    _refused(create(0, 44101, 16000, 4, 1, 0, 1, C.byref(h)), "1024")
    # a branch no block can stage, before n_streams
    _refused(create(0, 500, 1, -1, 1, 0, 0, C.byref(h)), "taps per output")
    _refused(create(0, 1024, 1, 4, 1, 0, 1, C.byref(h)), "taps per output")
    # n_streams, before the device index
    _refused(create(10**6, 10000, 16000, -1, 1, 0, 0, C.byref(h)), "n_streams")
    _refused(create(10**6, 10000, 16000, 2**31, 1, 0, 0, C.byref(h)), "n_streams")
    assert h.value is None
    # NULL handles
    co = np.array([0, 100], np.int64)
    idx = np.array([0], np.int64)
    _refused(L.dsp_stream_resample_push_device(None, None, co.ctypes.data_as(LP), None, None, None), "NULL")
    _refused(L.dsp_stream_resample_finish_device(None, idx.ctypes.data_as(LP), 1, None, None, None), "NULL")
    _refused(L.dsp_stream_resampler_reset(None, None, 0, None), "NULL")
    _refused(L.dsp_stream_resampler_counts(None, None, None), "NULL")
    _refused(L.dsp_stream_session_attach_resampler(None, None), "session is NULL")
    _refused(L.dsp_stream_session_attach_resampler(None, C.c_void_p(8)), "session is NULL")
    L.dsp_stream_resampler_destroy(None)


def test_stream_resample_symbols_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "dsp_amd.h")) as f:
        header = f.read()
    L = dl.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", dl._build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", nm, re.M))
    for name in SYMBOLS:
        assert not name.startswith("dsp_resampl")
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in dl.SYMBOLS and hasattr(L, name) and name in exported, name
    assert "Not covered: a filter-history carry" not in header


def test_stream_resample_wrapper_checks_raise_under_python_O():
    code = """
import numpy as np
import torch
import dsp_amd
for args in ((0, 16000, None, [0, 4]), (10000, 16000.0, None, [0, 4]), (10000, 16000, None, []), (10000, 16000, None, [[0, 4]]),
             (10000, 16000, None, [0, 4, 3]), (10000, 16000, None, [-1, 4]), (10000, 16000, [0, 0], [0, 4]), (10000, 16000, [-1], [0, 4])):
    try:
        dsp_amd.stream_resample_plan(*args)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for stream_resample_plan{args}")
try:
    dsp_amd.stream_resample_plan(1025, 1, None, [0, 4])
    raise SystemExit("no DspError for 1025 -> 1")
except dsp_amd.DspError:
    pass
for args, kw in (((0, 16000, 4), {}), ((10000, 16000, -1), {}), ((10000, 16000, 4), dict(dtype=torch.float64)), ((10000, 16000, 4), dict(channels=3)),
                 ((10000, 16000, 4), dict(channels=2)), ((10000, 16000, 4), dict(dtype=torch.int16, channels=2, stereo_mode=2))):
    try:
        dsp_amd.StreamResampler(*args, **kw)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for StreamResampler{args}{kw}")
try:
    dsp_amd.StreamResampler(500, 1, 4)
    raise SystemExit("no DspError for a ratio no block can stage")
except dsp_amd.DspError:
    pass
r = object.__new__(dsp_amd.StreamResampler)
r.rate_in, r.rate_out, r.up, r.down, r.half, r.n_streams, r.dtype, r.channels, r.device, r._h = 10000, 16000, 8, 5, 80, 2, torch.float32, 1, 0, None
for chunks, co in ((torch.zeros(8), [0, 4, 8]), ([0.0] * 8, [0, 4, 8]), (np.zeros(8, np.float32), [0, 4, 8])):
    try:
        r.push(chunks, co)
    except ValueError:
        continue
    raise SystemExit("no ValueError for a push of something that is not a CUDA tensor")
for call in (lambda: r.reset([2]), lambda: r.reset([[0]]), lambda: r.finish([-1]), lambda: r.finish([0, 0]), lambda: r.plan([0, 4])):
    try:
        call()
    except ValueError:
        continue
    raise SystemExit("no ValueError for streams / offsets the object does not have")
class Plan:
    _h, device, cfg = None, 0, dsp_amd.default_config()
for kw in (dict(rate_in=0), dict(rate_in=10000.0), dict(rate_in=10000, channels=2), dict(rate_in=10000, dtype=torch.float64)):
    try:
        dsp_amd.StreamSession(Plan(), 4, **kw)
    except ValueError:
        continue
    raise SystemExit(f"no ValueError for StreamSession{kw}")
print("ok")
"""
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
