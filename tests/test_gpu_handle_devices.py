"""GPU: the handles' lifetime and the caller's current device (tests/test_gpu_handles.py has the `with` protocol and the borrowers).
Every handle class of the Python layer: create, close, close again, with torch's current device the same before and after each step;
one smallest ragged call per module that sends spans through a ring (dsp_amd/csrc/capi_util.hpp SpanRing) between create and close,
so that a ring with a used slot and a recorded event is destroyed; and, where a second GPU is visible, all of it again with the handle
on device 1 while device 0 stays current, the results equal to device 0's bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, D = 2, 2
UBM = {"log_consts": np.log([0.4, 0.6]) - 0.5 * D * np.log(2 * np.pi), "means": np.array([[-1.0, 0.5], [1.0, -0.25]]), "inv_covs": np.ones((K, D))}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _device(torch, dev):
    if dev >= torch.cuda.device_count():
        pytest.skip(f"needs {dev + 1} visible GPUs")
    torch.cuda.set_device(0)
    return dev


def _models(golden):
    s = golden("speaker_gmm_ref.npz")
    t = {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")}
    u = {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}
    m = golden("scrubjay_svm.npz")
    return dict(golden("stop_model.npz")), t, u, {k: m[k] for k in m.files}


def _all_handle_classes():
    """the package's own subclasses of lib.Handle (a test elsewhere may have made one of its own)"""
    from dsp_amd import lib
    found, todo = set(), [lib.Handle]
    while todo:
        for c in todo.pop().__subclasses__():
            if c.__module__.startswith("dsp_amd."):
                found.add(c.__name__)
            todo.append(c)
    return found


@pytest.mark.parametrize("dev", [0, 1])
def test_create_close_close_leaves_the_current_device_alone(torch_cuda, golden, dev):
    import dsp_amd
    from dsp_amd import scrubjay
    torch = torch_cuda
    dev = _device(torch, dev)
    stop_p, t, u, svm_p = _models(golden)
    # what the scanners and the session borrow (closed last)
    plan, stop, spk = dsp_amd.MfccPlan(dsp_amd.default_config(), dev), dsp_amd.StopModel(stop_p, dev), dsp_amd.SpeakerModel(t, u, dev)
    sj = scrubjay.ScrubJay(svm_p, dev)
    makers = {
        "MfccPlan": lambda: dsp_amd.MfccPlan(dsp_amd.default_config(), dev),
        "SvmModel": lambda: scrubjay.SvmModel(svm_p, dev),
        "StopModel": lambda: dsp_amd.StopModel(stop_p, dev),
        "SpeakerModel": lambda: dsp_amd.SpeakerModel(t, u, dev),
        "Scanner": lambda: dsp_amd.Scanner(plan, stop, spk),
        "ScrubJayScanner": lambda: scrubjay.ScrubJayScanner(sj),
        "StreamSession": lambda: dsp_amd.StreamSession(plan, 1, stop, spk),
        "Resampler": lambda: dsp_amd.Resampler(8000, 16000, dev),
        "StreamResampler": lambda: dsp_amd.StreamResampler(8000, 16000, 1, device=dev),
        "Augmenter": lambda: dsp_amd.Augmenter(dev),
        "Cmvn": lambda: dsp_amd.Cmvn(D, 2, dev),
        "SpeakerEnroller": lambda: dsp_amd.SpeakerEnroller(UBM, dev),
        "SpeakerVerifier": lambda: dsp_amd.SpeakerVerifier(UBM, dev),
        "UbmTrainer": lambda: dsp_amd.UbmTrainer(K, D, dev),
        "SvmTrainer": lambda: scrubjay.SvmTrainer(4, dev),
        "StopTrainer": lambda: dsp_amd.StopTrainer(device=dev),
        "Segmenter": lambda: dsp_amd.Segmenter(dev),
        "TrialEvaluator": lambda: dsp_amd.TrialEvaluator(dev),
        "ScoreCalibrator": lambda: dsp_amd.ScoreCalibrator(dev),
    }
    assert set(makers) == _all_handle_classes()
    try:
        for name, make in makers.items():
            assert torch.cuda.current_device() == 0, name
            h = make()
            assert h._h and torch.cuda.current_device() == 0, name
            h.close()
            assert h._h is None and torch.cuda.current_device() == 0, name
            h.close()      # nothing left to do
            assert h._h is None and torch.cuda.current_device() == 0, name
    finally:
        for h in (sj.svm, sj.plan, spk, stop, plan):
            h.close()
    assert torch.cuda.current_device() == 0


def _ring_calls(torch, dev):
    """One smallest ragged call per module with a ring, on GPU `dev` with GPU 0 current: two clips of the minimum length each (the session:
    one stream, one push that completes one row).  Each handle is closed behind its call, before the results are read.
    -> {name: [numpy arrays]}"""
    import dsp_amd
    where = f"cuda:{dev}"
    rng = np.random.default_rng(77)
    feats = torch.from_numpy(rng.standard_normal((2, D)).astype(np.float32)).to(where)      # two clips of one row
    means = torch.from_numpy(rng.standard_normal((1, K, D)).astype(np.float32)).to(where)
    two = torch.from_numpy(rng.uniform(-1, 1, 2).astype(np.float32)).to(where)              # two recordings of one sample
    chunk = torch.from_numpy(rng.uniform(-1, 1, 400).astype(np.float32)).to(where)          # one frame of the default plan
    fo = [0, 1, 2]
    out = {}

    def call(name, make, run):
        assert torch.cuda.current_device() == 0, name
        h = make()
        assert torch.cuda.current_device() == 0, name
        got = run(h)
        assert torch.cuda.current_device() == 0, name
        h.close()
        assert h._h is None and torch.cuda.current_device() == 0, name
        h.close()
        assert torch.cuda.current_device() == 0, name
        out[name] = [g.cpu().numpy() for g in got]

    call("Cmvn", lambda: dsp_amd.Cmvn(D, 2, dev), lambda h: [h.apply(feats, fo)])
    call("SpeakerEnroller", lambda: dsp_amd.SpeakerEnroller(UBM, dev),
         lambda h: [v for _, v in sorted(h.enroll(feats, fo).items())])
    call("SpeakerVerifier", lambda: dsp_amd.SpeakerVerifier(UBM, dev),
         lambda h: [v for _, v in sorted(h.verify(feats, fo, means, want=dsp_amd.SpeakerVerifier.OUTPUTS).items())])
    call("Resampler", lambda: dsp_amd.Resampler(8000, 16000, dev), lambda h: [h.ragged(two, fo)[0]])
    plan = dsp_amd.MfccPlan(dsp_amd.default_config(), dev)
    try:
        call("StreamSession", lambda: dsp_amd.StreamSession(plan, 1), lambda h: [h.push(chunk, [0, 400])[1]])
    finally:
        plan.close()
    assert torch.cuda.current_device() == 0
    return out


@pytest.fixture(scope="module")
def on_device_0(torch_cuda):
    torch_cuda.cuda.set_device(0)
    return _ring_calls(torch_cuda, 0)


def test_a_used_ring_is_destroyed_with_its_handle(on_device_0):
    got = on_device_0
    assert [a.shape for a in got["Cmvn"]] == [(2, D)] and got["Resampler"][0].shape == (4,) and got["StreamSession"][0].shape == (1, 13)
    assert len(got["SpeakerEnroller"]) == 5 and len(got["SpeakerVerifier"]) == 5
    for name, arrays in got.items():
        for a in arrays:
            assert np.isfinite(a.astype(np.float64)).all(), name


def test_a_handle_on_device_1_computes_what_device_0_computes(torch_cuda, on_device_0):
    dev = _device(torch_cuda, 1)
    got = _ring_calls(torch_cuda, dev)
    assert got.keys() == on_device_0.keys()
    for name, arrays in got.items():
        for a, b in zip(arrays, on_device_0[name]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
