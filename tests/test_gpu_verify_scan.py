"""GPU: the float speaker scan (dsp_speaker_float_scan_device; dsp_amd.SpeakerVerifier.scan).

What must hold bit for bit: every output of every window is what dsp_speaker_verify_ragged_device gives for the window's rows handed over
as a clip of their own -- and stays the same bits whatever the batch of recordings, the other speakers, a speaker's position, the outputs
asked for, the stream, the split of the call over runs of windows and what the workspace held.  Against float64 (tests/verify_scan_ref.py)
the gate is tests/verify_ref.py's: 8 times what the restatement's own float32 model deviates on the same inputs, floored at 8 * 2^-23 *
max |value|, never computed from the library; `best` by tests/verify_util.py check_best with at least half the windows decided
(tests/test_verify_scan_cpu.py checks that on the inputs alone)."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import verify_ref as V
from tests import verify_scan_ref as VS
from tests.enroll_util import ROOT
from tests.verify_scan_util import SCAN_CONFIGS, SCAN_KD, SCAN_OTHER_D, SCAN_SPEAKERS, scan_case, scan_ref
from tests.verify_util import check_best, offsets, subset

pytestmark = pytest.mark.gpu
LP = C.POINTER(C.c_long)
FLOATS = ("llr", "ll_ubm", "ll_target", "best_llr")
SPARE = 5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _cuda(torch, a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")      # (a copy: the shared cases are read-only)


def _raw(torch, ver, feats, fo, means, scan=None, want=V.OUTPUTS, stream=None):
    """dsp_speaker_float_scan_device (scan = (window, hop)) or dsp_speaker_verify_ragged_device (scan = None) into NaN- (best: -7-) filled
    buffers with SPARE entries behind each -> numpy, the spare checked"""
    import dsp_amd
    fo = np.ascontiguousarray(fo, np.int64)
    n_spk = means.shape[0]
    n = fo.size - 1 if scan is None else int(dsp_amd.scan_window_offsets(fo, *scan)[-1])
    x, m = _cuda(torch, feats), _cuda(torch, means)
    size = {"llr": n * n_spk, "ll_ubm": n, "ll_target": n * n_spk, "best": n, "best_llr": n}
    bufs = {key: (torch.full((size[key] + SPARE,), -7, dtype=torch.int32, device="cuda") if key == "best" else
                  torch.full((size[key] + SPARE,), float("nan"), dtype=torch.float32, device="cuda")) for key in want}
    torch.cuda.synchronize()
    outs = [bufs[key].data_ptr() if key in bufs else None for key in V.OUTPUTS]
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    if scan is None:
        rc = ver._L.dsp_speaker_verify_ragged_device(ver._h, x.data_ptr(), fo.size - 1, fo.ctypes.data_as(LP), m.data_ptr(), n_spk, *outs, st)
    else:
        rc = ver._L.dsp_speaker_float_scan_device(ver._h, x.data_ptr(), fo.size - 1, fo.ctypes.data_as(LP), C.byref(dsp_amd.lib.ScanConfig(*scan)),
                                                  m.data_ptr(), n_spk, *outs, st)
    assert rc == 0, dsp_amd.lib.last_error()
    torch.cuda.synchronize()
    out = {}
    for key, buf in bufs.items():
        a = buf.cpu().numpy()
        assert (np.all(a[size[key]:] == -7) if key == "best" else np.isnan(a[size[key]:]).all()), f"{key}: wrote behind the output"
        out[key] = a[:size[key]].reshape((n, n_spk) if key in ("llr", "ll_target") else (n,))
    return out


def _cut(torch, x, fo, window, hop):
    """the windows gathered on the device into a ragged matrix of their own -> (rows, clip offsets)"""
    start, n = VS.window_spans(fo, window, hop)
    clip_fo = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    idx = np.repeat(start - clip_fo[:-1], n) + np.arange(clip_fo[-1])
    return x[torch.tensor(idx, device="cuda")], clip_fo


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), (what, key)      # bits, not values


@pytest.mark.parametrize("k,d", SCAN_KD)
def test_every_window_is_the_per_clip_entry_on_its_rows(torch_cuda, k, d):
    """the definition: all five outputs, every scan configuration, 1, 3, 16, 17 and 33 speakers"""
    import dsp_amd
    torch = torch_cuda
    case = scan_case(k, d)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    x = _cuda(torch, case["feats"])
    for window, hop in SCAN_CONFIGS:
        rows, clip_fo = _cut(torch, x, case["fo"], window, hop)
        for n_spk in SCAN_SPEAKERS:
            means = _cuda(torch, case["means"][:n_spk])
            got = _raw(torch, ver, x, case["fo"], means, (window, hop))
            clips = _raw(torch, ver, rows, clip_fo, means)
            _same(got, clips, (k, d, window, hop, n_spk))


def _check_parity(got, want, model, what):
    gates = V.gates(want, model)
    errs = {key: float(np.abs(got[key].astype(np.float64) - want[key]).max()) for key in FLOATS}
    print(f"\nscan {what}: deviation / gate " + ", ".join(f"{k} {errs[k]:.3e} / {gates[k]:.3e}" for k in FLOATS))
    for key in FLOATS:
        assert got[key].dtype == np.float32 and np.isfinite(got[key]).all() and gates[key] > 0.0, (what, key)
        assert errs[key] <= gates[key], (what, key, errs[key], gates[key])
    assert got["best"].dtype == np.int32
    sure = check_best(got["best"], want["llr"], gates["llr"])
    assert sure.sum() * 2 >= sure.size, (what, int(sure.sum()))
    rows = np.arange(got["llr"].shape[0])
    assert np.array_equal(got["best_llr"], got["llr"][rows, got["best"]])                   # that value, bit for bit
    assert np.array_equal(got["best"], np.argmax(got["llr"], axis=1))                       # the smallest s with the largest llr


@pytest.mark.parametrize("k,d", SCAN_KD)
def test_parity_with_float64(torch_cuda, k, d):
    import dsp_amd
    torch = torch_cuda
    case = scan_case(k, d)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    x = _cuda(torch, case["feats"])
    for window, hop in SCAN_CONFIGS:
        want, model = scan_ref(k, d, window, hop)
        for n_spk in SCAN_SPEAKERS:
            got = _raw(torch, ver, x, case["fo"], case["means"][:n_spk], (window, hop))
            _check_parity(got, subset(want, n_spk), subset(model, n_spk), f"k {k} d {d} window {window} hop {hop} S {n_spk}")


@pytest.mark.parametrize("d", SCAN_OTHER_D)
def test_other_d_of_the_dispatch(torch_cuda, d):
    """further instantiations of the row-score kernel, at k = 5 and (98, 10): through the wrapper, which returns what was asked for"""
    import dsp_amd
    torch = torch_cuda
    case = scan_case(5, d)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    x, m = _cuda(torch, case["feats"]), _cuda(torch, case["means"])
    out = ver.scan(x, case["fo"], m, 98, 10, want=V.OUTPUTS)
    nw = int(dsp_amd.scan_window_offsets(case["fo"], 98, 10)[-1])
    assert out["llr"].shape == (nw, 33) and out["best"].dtype == torch.int32 and out["ll_ubm"].shape == (nw,) and out["ll_target"].shape == (nw, 33)
    _check_parity({key: out[key].cpu().numpy() for key in V.OUTPUTS}, *scan_ref(5, d, 98, 10), f"k 5 d {d} wrapper")
    default = ver.scan(x, case["fo"], m, 98, 10)
    assert sorted(default) == ["best", "best_llr", "ll_ubm", "llr"] and all(torch.equal(default[key], out[key]) for key in default)
    rows, clip_fo = _cut(torch, x, case["fo"], 98, 10)
    clips = ver.verify(rows, clip_fo, m, want=V.OUTPUTS)
    assert all(torch.equal(clips[key], out[key]) for key in V.OUTPUTS)


@pytest.mark.parametrize("which,window,hop", [("k32_d13", 98, 10), ("k5_d13", 30, 45), ("k64_d16", 257, 100), ("k1_d1", 65, 64)])
def test_a_window_does_not_see_its_surroundings(torch_cuda, which, window, hop):
    """every (window, speaker) pair gives the same bits: each recording alone, in the batch and in the reversed batch; each of 17 speakers
    alone and in the reversed set (positions cross speaker tiles); each single output and each output left out; after a larger call has
    grown the workspace; on a stream of its own; after a per-clip call on the same verifier, which shares the workspace -- and that
    per-clip call gives its own bits after a scan"""
    import dsp_amd
    torch = torch_cuda
    case = scan_case(*{"k32_d13": (32, 13), "k5_d13": (5, 13), "k64_d16": (64, 16), "k1_d1": (1, 1)}[which])
    feats, fo, scan = case["feats"], case["fo"], (window, hop)
    means = case["means"][:V.SPEAKER_TILE + 1]
    n, n_spk = fo.size - 1, means.shape[0]
    wo = dsp_amd.scan_window_offsets(fo, window, hop)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])                                   # a fresh workspace: the calls below grow it
    parts = [feats[fo[r]:fo[r + 1]] for r in range(n)]
    alone = [_raw(torch, ver, parts[r], [0, parts[r].shape[0]], means, scan) for r in range(n)]
    batch = _raw(torch, ver, feats, fo, means, scan)
    rev_fo = offsets([p.shape[0] for p in parts[::-1]])
    rev = _raw(torch, ver, np.concatenate(parts[::-1]), rev_fo, means, scan)
    rev_wo = dsp_amd.scan_window_offsets(rev_fo, window, hop)
    for r in range(n):
        for key in V.OUTPUTS:
            mine = batch[key][wo[r]:wo[r + 1]]
            assert np.array_equal(alone[r][key].view(np.int32), mine.view(np.int32)), (which, "alone", r, key)
            assert np.array_equal(rev[key][rev_wo[n - 1 - r]:rev_wo[n - r]].view(np.int32), mine.view(np.int32)), (which, "reversed", r, key)
    for s in range(n_spk):
        one = _raw(torch, ver, feats, fo, means[s:s + 1], scan, want=["llr", "ll_target", "ll_ubm"])
        assert np.array_equal(one["llr"][:, 0], batch["llr"][:, s]) and np.array_equal(one["ll_target"][:, 0], batch["ll_target"][:, s]), (which, s)
        assert np.array_equal(one["ll_ubm"], batch["ll_ubm"])
    back = _raw(torch, ver, feats, fo, means[::-1], scan)
    assert np.array_equal(back["llr"][:, ::-1], batch["llr"]) and np.array_equal(back["ll_target"][:, ::-1], batch["ll_target"])
    assert np.array_equal(back["ll_ubm"], batch["ll_ubm"]) and np.array_equal(back["best_llr"], batch["best_llr"])
    for key in V.OUTPUTS:
        _same(_raw(torch, ver, feats, fo, means, scan, want=[key]), {key: batch[key]}, (which, "only", key))
        rest = [other for other in V.OUTPUTS if other != key]
        _same(_raw(torch, ver, feats, fo, means, scan, want=rest), {other: batch[other] for other in rest}, (which, "without", key))
    _raw(torch, ver, np.concatenate([feats[fo[0]:]] * 3), offsets(list(np.diff(fo)) * 3), case["means"], scan)      # three times the rows, more models
    _same(_raw(torch, ver, feats, fo, means, scan), batch, (which, "after a larger call"))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _same(_raw(torch, ver, feats, fo, means, scan, stream=side), batch, (which, "side stream"))
    fresh = _raw(torch, dsp_amd.SpeakerVerifier(case["ubm"]), feats, fo, means)
    _same(_raw(torch, ver, feats, fo, means), fresh, (which, "verify after a scan"))
    _same(_raw(torch, ver, feats, fo, means, scan), batch, (which, "scan after verify"))


def test_a_split_scan_gives_the_same_bits(torch_cuda):
    """a scan whose per-row ll would pass the workspace bound is cut into runs of consecutive windows: with the bound brought down
    (DSP_AMD_VERIFY_SCAN_RUN_FLOATS, read when a verifier is made) to one float -- every window a run of its own -- and to runs of a few
    windows, every output is what the unsplit call gives.  In a child process: the variable is the child's alone."""
    code = """
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
import dsp_amd
from tests.verify_scan_util import scan_case
case = scan_case(5, 13)
x, m = torch.tensor(case["feats"], device="cuda"), torch.tensor(case["means"], device="cuda")
want = ("llr", "ll_ubm", "ll_target", "best", "best_llr")
for window, hop in ((98, 10), (64, 1)):
    whole = dsp_amd.SpeakerVerifier(case["ubm"]).scan(x, case["fo"], m, window, hop, want=want)
    for floats in (1, 34 * (window + 2 * hop), 34 * (window + 7 * hop + 3)):     # every window a run; runs of about 3 and of about 8 windows
        os.environ["DSP_AMD_VERIFY_SCAN_RUN_FLOATS"] = str(floats)
        split = dsp_amd.SpeakerVerifier(case["ubm"]).scan(x, case["fo"], m, window, hop, want=want)
        torch.cuda.synchronize()
        assert all(torch.equal(split[key], whole[key]) for key in want), (window, hop, floats)
    del os.environ["DSP_AMD_VERIFY_SCAN_RUN_FLOATS"]
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_exact_identities(torch_cuda):
    """a speaker whose means are the UBM's float32 means: llr == +0.0 exactly and ll_target == ll_ubm bitwise on every window -- beside the
    UBM in its block (0, 15) and in the next speaker tile (16)"""
    import dsp_amd
    torch = torch_cuda
    for k, d in ((5, 13), (64, 16)):
        case = scan_case(k, d)
        ver = dsp_amd.SpeakerVerifier(case["ubm"])
        means = case["means"][:V.SPEAKER_TILE + 1].copy()
        for at in (0, V.SPEAKER_TILE - 1, V.SPEAKER_TILE):
            means[at] = np.asarray(case["ubm"]["means"], np.float64).astype(np.float32)
        for scan in ((98, 10), (1, 1), (257, 100)):
            full = _raw(torch, ver, case["feats"], case["fo"], means, scan)
            for at in (0, V.SPEAKER_TILE - 1, V.SPEAKER_TILE):
                assert np.all(full["llr"][:, at] == 0.0) and not np.signbit(full["llr"][:, at]).any()
                assert np.array_equal(full["ll_target"][:, at].view(np.int32), full["ll_ubm"].view(np.int32))


def test_audio_to_windows_on_the_device(torch_cuda, golden):
    """SpeakerFrontEnd.features -> SpeakerEnroller.enroll -> scan, no host trip in between: three recordings of 0.5 s, 1 s + 1 sample and
    3.2 s at 16 kHz; the result is verify on the cut-out rows, bit for bit, and the window count is scan_window_offsets'"""
    import dsp_amd
    from tests.enroll_util import fixture
    torch = torch_cuda
    _, ubm, _ = fixture(golden)
    rng = np.random.default_rng(4116)
    lens = [8000, 16001, 51200]
    audio = torch.tensor(np.concatenate([0.1 * rng.standard_normal(n) for n in lens]).astype(np.float32), device="cuda")
    with dsp_amd.SpeakerFrontEnd() as fe:
        feats, fo = fe.features(audio, offsets(lens))
    assert np.diff(fo).tolist() == [1 + n // 160 for n in lens]
    en, ver = dsp_amd.SpeakerEnroller(ubm), dsp_amd.SpeakerVerifier(ubm)
    means = en.enroll(feats, fo)["means"]
    out = ver.scan(feats, fo, means, 98, 10, want=V.OUTPUTS)
    wo = dsp_amd.scan_window_offsets(fo, 98, 10)
    assert np.diff(wo).tolist() == [1, 1, 1 + (321 - 98) // 10] and out["llr"].shape == (wo[-1], 3)
    rows, clip_fo = _cut(torch, feats, fo, 98, 10)
    clips = ver.verify(rows, clip_fo, means, want=V.OUTPUTS)
    assert all(torch.equal(clips[key], out[key]) for key in V.OUTPUTS)
    assert bool(torch.isfinite(out["llr"]).all())


def test_refusals_reach_no_kernel(torch_cuda):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    case = scan_case(5, 13)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    x, m = _cuda(torch, case["feats"]), _cuda(torch, case["means"][:3])
    llr = torch.full((64, 3), 5.0, device="cuda")
    off = lambda *a: (C.c_long * len(a))(*a)                                    # noqa: E731

    def call(n, offsets_, n_spk=3, out=llr, cfg=dl.ScanConfig(98, 10)):
        return ver._L.dsp_speaker_float_scan_device(ver._h, x.data_ptr(), n, offsets_, C.byref(cfg) if cfg is not None else None, m.data_ptr(), n_spk,
                                                    out.data_ptr() if out is not None else None, None, None, None, None, None)

    def einval(rc, *words):
        assert rc == -1 and all(w in dl.last_error() for w in words), (rc, dl.last_error())

    einval(call(3, off(0, 10, 10, 20)), "recording 1", "no rows")
    einval(call(2, off(0, 10, 5)), "decrease")
    einval(call(1, off(0, 10), out=None), "NULL")
    einval(call(1, off(0, 10), cfg=None), "dsp_scan_config")
    einval(call(1, off(0, 10), cfg=dl.ScanConfig(98, 0)), "hop_frames")
    assert call(0, None) == 0 and call(1, off(0, 10), n_spk=0) == 0
    torch.cuda.synchronize()
    assert bool((llr == 5.0).all())                                              # no refused or empty call wrote anything
    with pytest.raises(ValueError):
        ver.scan(x, [0, 10, 10, 20], m, 98, 10)
    with pytest.raises(ValueError):
        ver.scan(x, [0, 10], m, 0, 10)
    with pytest.raises(ValueError):
        ver.scan(x, [0, 10], m[:, :4], 98, 10)                                   # means of another k
    with pytest.raises(ValueError):
        ver.scan(x, [0, 10], m.double(), 98, 10)
