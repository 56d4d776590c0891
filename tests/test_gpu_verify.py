"""GPU: float speaker verification (dsp_speaker_verif*; dsp_amd.SpeakerVerifier) against the float64 restatement of its definition
(tests/verify_ref.py) and against sklearn's scores (tests/golden/speaker_verify_ref.npz).

The gate, per output: a GPU value may deviate from float64 by GATE_FACTOR = 8 times what the restatement's own float32 model deviates on
the same inputs, floored at 8 * 2^-23 * max |value| (computed from tests/verify_ref.py, never from the library; 8 covers the fused
multiply-add, the hardware's expf and logf at equal precision).  `best` must lie within 2 gates of the float64 maximum and be the float64
argmax wherever the runner-up is more than 2 gates below it -- at least half of the clips of every case (tests/test_verify_cpu.py checks
that on the inputs alone).  Then what must hold bit for bit: a (clip, speaker) pair gives the same outputs whatever the batch, the other
speakers, the speaker's position, the outputs asked for, the stream, the split of the call and what the workspace held."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import enroll_ref as E
from tests import verify_ref as V
from tests.enroll_util import ROOT
from tests.verify_util import SWEEP_KD, SWEEP_SPEAKERS, check_best, fixture_case, offsets, subset, sweep_case

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
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")            # (a copy: the shared cases are read-only)


def _raw(torch, ver, feats, fo, means, want=V.OUTPUTS, stream=None):
    """dsp_speaker_verify_ragged_device into NaN- (best: -7-) filled buffers with SPARE entries behind each -> numpy, the spare checked"""
    import dsp_amd
    fo = np.ascontiguousarray(fo, np.int64)
    n, n_spk = fo.size - 1, means.shape[0]
    x, m = _cuda(torch, feats), _cuda(torch, means)
    size = {"llr": n * n_spk, "ll_ubm": n, "ll_target": n * n_spk, "best": n, "best_llr": n}
    bufs = {key: (torch.full((size[key] + SPARE,), -7, dtype=torch.int32, device="cuda") if key == "best" else
                  torch.full((size[key] + SPARE,), float("nan"), dtype=torch.float32, device="cuda")) for key in want}
    torch.cuda.synchronize()
    rc = ver._L.dsp_speaker_verify_ragged_device(ver._h, x.data_ptr(), n, fo.ctypes.data_as(LP), m.data_ptr(), n_spk,
                                                 *[bufs[key].data_ptr() if key in bufs else None for key in V.OUTPUTS],
                                                 C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, dsp_amd.lib.last_error()
    torch.cuda.synchronize()
    out = {}
    for key, buf in bufs.items():
        a = buf.cpu().numpy()
        assert (np.all(a[size[key]:] == -7) if key == "best" else np.isnan(a[size[key]:]).all()), f"{key}: wrote behind the output"
        out[key] = a[:size[key]].reshape((n, n_spk) if key in ("llr", "ll_target") else (n,))
    return out


def _check_parity(got, want, model, what, others=()):
    """the five outputs against float64 (and against `others`, further references of the float64 kind) under the 8 x rule -> the gates"""
    gates = V.gates(want, model)
    errs = {key: float(np.abs(got[key].astype(np.float64) - want[key]).max()) for key in FLOATS}
    print(f"\nverify {what}: gates " + ", ".join(f"{k} {v:.3e}" for k, v in gates.items()) + "; GPU vs float64 " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for key in FLOATS:
        assert got[key].dtype == np.float32 and np.isfinite(got[key]).all() and gates[key] > 0.0, (what, key)
        assert errs[key] <= gates[key], (what, key, errs[key], gates[key])
        for other in others:
            if key in other:
                assert float(np.abs(got[key].astype(np.float64) - other[key]).max()) <= gates[key], (what, key, "sklearn")
    assert got["best"].dtype == np.int32
    sure = check_best(got["best"], want["llr"], gates["llr"])
    assert sure.sum() * 2 >= sure.size, (what, int(sure.sum()))
    rows = np.arange(got["llr"].shape[0])
    assert np.array_equal(got["best_llr"], got["llr"][rows, got["best"]])                   # that value, bit for bit
    assert np.array_equal(got["best"], np.argmax(got["llr"], axis=1))                       # the smallest s with the largest llr
    return gates


def test_fixture_parity_with_float64_and_sklearn(torch_cuda, golden):
    import dsp_amd
    case = fixture_case(golden)
    assert np.diff(case["fo"]).tolist() == [1, 2, 64, 97, 150, 299, 300, 301, 700, 1025, 1500, 4097] and case["means"].shape == (12, 32, 13)
    got = _raw(torch_cuda, dsp_amd.SpeakerVerifier(case["ubm"]), case["feats"], case["fo"], case["means"])
    _check_parity(got, case["want"], case["model"], "fixture", others=(case["sklearn"],))


@pytest.mark.parametrize("k,d", SWEEP_KD)
def test_shape_sweep(torch_cuda, k, d):
    """k x d at the edges of what is accepted; clips of 1 .. 700 rows in one batch -- every edge of the 64-row tile and the 256-row chunk --
    with 3 rows of no clip in front; 1, 3, T, T + 1 and 2 T + 1 speakers (T = the kernel's speaker tile); a UBM with a component at the
    1e-6 variance floor"""
    import dsp_amd
    case = sweep_case(k, d)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    for n_spk in SWEEP_SPEAKERS:
        got = _raw(torch_cuda, ver, case["feats"], case["fo"], case["means"][:n_spk])
        _check_parity(got, subset(case["want"], n_spk), subset(case["model"], n_spk), f"k {k} d {d} S {n_spk}")


@pytest.mark.parametrize("d", [2, 7, 12])
def test_other_d_of_the_dispatch(torch_cuda, d):
    """further instantiations of the scoring kernel, at k = 5: through the wrapper, which returns what was asked for"""
    import dsp_amd
    torch = torch_cuda
    case = sweep_case(5, d)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    out = ver.verify(_cuda(torch, case["feats"]), case["fo"], _cuda(torch, case["means"]), want=V.OUTPUTS)
    assert out["llr"].shape == (9, 33) and out["best"].dtype == torch.int32 and out["ll_ubm"].shape == (9,)
    _check_parity({key: out[key].cpu().numpy() for key in V.OUTPUTS}, case["want"], case["model"], f"k 5 d {d} wrapper")
    default = ver.verify(_cuda(torch, case["feats"]), case["fo"], _cuda(torch, case["means"]))
    assert sorted(default) == ["best", "best_llr", "ll_ubm", "llr"] and all(torch.equal(default[key], out[key]) for key in default)


def test_exact_identities(torch_cuda, golden):
    """a speaker whose means are the UBM's float32 means: llr == 0.0 exactly and ll_target == ll_ubm bitwise, for every clip; and each
    output that may be NULL, left out, leaves the others the same bits"""
    import dsp_amd
    torch = torch_cuda
    for case in (fixture_case(golden), sweep_case(64, 16), sweep_case(5, 13)):
        ver = dsp_amd.SpeakerVerifier(case["ubm"])
        means = np.concatenate([case["means"]] * 2)[:V.SPEAKER_TILE + 1].copy()
        for at in (0, V.SPEAKER_TILE - 1, V.SPEAKER_TILE):                       # beside the UBM in its block, and in the next speaker tile
            means[at] = np.asarray(case["ubm"]["means"], np.float64).astype(np.float32)
        full = _raw(torch, ver, case["feats"], case["fo"], means)
        for at in (0, V.SPEAKER_TILE - 1, V.SPEAKER_TILE):
            assert np.all(full["llr"][:, at] == 0.0) and not np.signbit(full["llr"][:, at]).any()
            assert np.array_equal(full["ll_target"][:, at], full["ll_ubm"])
        for left_out in V.OUTPUTS:
            part = _raw(torch, ver, case["feats"], case["fo"], means, want=[key for key in V.OUTPUTS if key != left_out])
            assert left_out not in part and all(np.array_equal(part[key], full[key]) for key in part), left_out
        only = _raw(torch, ver, case["feats"], case["fo"], means, want=["best"])
        assert np.array_equal(only["best"], full["best"])


@pytest.mark.parametrize("which", ["fixture", "k32_d13", "k64_d16", "k1_d1"])
def test_a_trial_does_not_see_its_surroundings(torch_cuda, golden, which):
    """every (clip, speaker) pair gives the same bits: each clip alone, in the batch and in the reversed batch; each speaker alone, in the
    full set and in the reversed set (positions across T and T + 1 change speaker tiles); after a larger call has grown the workspace;
    on a stream of its own"""
    import dsp_amd
    torch = torch_cuda
    case = fixture_case(golden) if which == "fixture" else sweep_case(*{"k32_d13": (32, 13), "k64_d16": (64, 16), "k1_d1": (1, 1)}[which])
    feats, fo = case["feats"], case["fo"]
    means = case["means"][:V.SPEAKER_TILE + 1]
    n, n_spk = fo.size - 1, means.shape[0]
    ver = dsp_amd.SpeakerVerifier(case["ubm"])                                   # a fresh workspace: the calls below grow it
    parts = [feats[fo[c]:fo[c + 1]] for c in range(n)]
    alone = [_raw(torch, ver, parts[c], [0, parts[c].shape[0]], means) for c in range(n)]
    batch = _raw(torch, ver, feats, fo, means)
    rev = _raw(torch, ver, np.concatenate(parts[::-1]), offsets([p.shape[0] for p in parts[::-1]]), means)
    for c in range(n):
        for key in V.OUTPUTS:
            assert np.array_equal(alone[c][key][0], batch[key][c]), (which, "alone", c, key)
            assert np.array_equal(rev[key][n - 1 - c], batch[key][c]), (which, "reversed", c, key)
    for s in range(n_spk):
        one = _raw(torch, ver, feats, fo, means[s:s + 1], want=["llr", "ll_target", "ll_ubm"])
        assert np.array_equal(one["llr"][:, 0], batch["llr"][:, s]) and np.array_equal(one["ll_target"][:, 0], batch["ll_target"][:, s]), (which, s)
        assert np.array_equal(one["ll_ubm"], batch["ll_ubm"])
    back = _raw(torch, ver, feats, fo, means[::-1])
    assert np.array_equal(back["llr"][:, ::-1], batch["llr"]) and np.array_equal(back["ll_target"][:, ::-1], batch["ll_target"])
    assert np.array_equal(back["ll_ubm"], batch["ll_ubm"]) and np.array_equal(back["best_llr"], batch["best_llr"])
    more = case["means"] if case["means"].shape[0] > n_spk else np.concatenate([means, means])
    _raw(torch, ver, np.concatenate([feats[fo[0]:]] * 3), offsets(list(np.diff(fo)) * 3), more)          # three times the tiles, more models
    again = _raw(torch, ver, feats, fo, means)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        streamed = _raw(torch, ver, feats, fo, means, stream=side)
    for key in V.OUTPUTS:
        assert np.array_equal(again[key], batch[key]) and np.array_equal(streamed[key], batch[key]), (which, key)


def test_a_split_call_gives_the_same_bits(torch_cuda):
    """a call whose tile sums would pass the workspace bound is split over runs of clips: with the bound brought down to a few chunks
    (DSP_AMD_VERIFY_RUN_DOUBLES, read when a verifier is made) every output is what the unsplit call gives.  In a child process: the
    variable is the child's alone."""
    code = """
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
import dsp_amd
from tests.verify_util import sweep_case
case = sweep_case(5, 13)
x, m = torch.tensor(case["feats"], device="cuda"), torch.tensor(case["means"], device="cuda")
want = ("llr", "ll_ubm", "ll_target", "best", "best_llr")
whole = dsp_amd.SpeakerVerifier(case["ubm"]).verify(x, case["fo"], m, want=want)
for doubles in (1, 4 * 34 * 2, 4 * 34 * 5):                 # every clip a run of its own; runs of at most 2 and of at most 5 chunks
    os.environ["DSP_AMD_VERIFY_RUN_DOUBLES"] = str(doubles)
    split = dsp_amd.SpeakerVerifier(case["ubm"]).verify(x, case["fo"], m, want=want)
    torch.cuda.synchronize()
    assert all(torch.equal(split[key], whole[key]) for key in want), doubles
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_enrolled_means_go_straight_to_the_verifier(torch_cuda, golden):
    """enrol -> verify on the device: SpeakerEnroller.enroll(...)["means"] is `means` as it is; clip i, held-out rows of the synthetic
    speaker i was enrolled from, has llr > 0 against speaker i and is identified as i; and ll_ubm is the enroller's ll_mean of the same
    rows within the sum of both gates (the component sum differs in order by definition, so not bit for bit)"""
    import dsp_amd
    torch = torch_cuda
    ubm = fixture_case(golden)["ubm"]
    rng = np.random.default_rng(4103)
    lens = [700, 1500, 257, 1024, 300]
    draws = [E.draw_speaker(rng, ubm, n + 400) for n in lens]
    train, fo_train = np.concatenate([x[:n] for x, n in zip(draws, lens)]), offsets(lens)
    held, fo_held = np.concatenate([x[n:] for x, n in zip(draws, lens)]), offsets([400] * len(lens))
    en, ver = dsp_amd.SpeakerEnroller(ubm), dsp_amd.SpeakerVerifier(ubm)
    x_train = _cuda(torch, train)
    enrolled = en.enroll(x_train, fo_train)
    out = ver.verify(_cuda(torch, held), fo_held, enrolled["means"], want=V.OUTPUTS)          # no host trip in between
    llr = out["llr"].cpu().numpy()
    print("\nown llr", np.diag(llr).tolist(), "largest impostor llr", float((llr - np.diag(np.full(len(lens), np.inf))).max()))
    assert np.all(np.diag(llr) > 0.0) and np.array_equal(out["best"].cpu().numpy(), np.arange(len(lens)))
    means = enrolled["means"].cpu().numpy()
    want, model = V.verify(held, fo_held, ubm, means), V.verify(held, fo_held, ubm, means, np.float32)
    _check_parity({key: out[key].cpu().numpy() for key in V.OUTPUTS}, want, model, "enrolled on the device")
    # the training rows through both: the enroller's mean of ll and the verifier's ll_ubm
    same = ver.verify(x_train, fo_train, enrolled["means"], want=("ll_ubm",))["ll_ubm"].cpu().numpy().astype(np.float64)
    ll_mean = enrolled["ll_mean"].cpu().numpy().astype(np.float64)
    w_en, m_en = E.enroll_ragged(train, fo_train, ubm), E.enroll_ragged(train, fo_train, ubm, dtype=np.float32)
    gate_en = E.GATE_FACTOR * float(np.abs(m_en["ll_mean"].astype(np.float64) - w_en["ll_mean"]).max())
    gate_ver = V.gates(V.verify(train, fo_train, ubm, means[:1]), V.verify(train, fo_train, ubm, means[:1], np.float32))["ll_ubm"]
    err = float(np.abs(same - ll_mean).max())
    print(f"ll_ubm vs the enroller's ll_mean: {err:.3e}, gates {gate_ver:.3e} + {gate_en:.3e}")
    assert gate_en > 0.0 and err <= gate_ver + gate_en


def test_refusals_reach_no_kernel(torch_cuda, golden):
    import dsp_amd
    from dsp_amd import lib as dl
    torch = torch_cuda
    case = sweep_case(5, 13)
    ver = dsp_amd.SpeakerVerifier(case["ubm"])
    x, m = _cuda(torch, case["feats"]), _cuda(torch, case["means"][:3])
    llr = torch.full((9, 3), 5.0, device="cuda")
    off = lambda *a: (C.c_long * len(a))(*a)                                    # noqa: E731

    def call(n, offsets_, n_spk=3, out=llr):
        return ver._L.dsp_speaker_verify_ragged_device(ver._h, x.data_ptr(), n, offsets_, m.data_ptr(), n_spk, out.data_ptr() if out is not None else None,
                                                       None, None, None, None, None)

    def einval(rc, *words):
        assert rc == -1 and all(w in dl.last_error() for w in words), (rc, dl.last_error())

    einval(call(3, off(0, 10, 10, 20)), "clip 1", "no rows")
    einval(call(2, off(0, 10, 5)), "decrease")
    einval(call(1, off(0, 10), out=None), "NULL")
    assert call(0, None) == 0 and call(1, off(0, 10), n_spk=0) == 0
    torch.cuda.synchronize()
    assert bool((llr == 5.0).all())                                              # no refused or empty call wrote anything
    with pytest.raises(ValueError):
        ver.verify(x, [0, 10, 10, 20], m)
    with pytest.raises(ValueError):
        ver.verify(x, [0, 10], m[:, :4])                                         # means of another k
    with pytest.raises(ValueError):
        ver.verify(x, [0, 10], m.double())
