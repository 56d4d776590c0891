"""GPU: the lifecycle of every class that owns native handles (lib.Handle, and SpeakerFrontEnd with its two), each made with the
smallest parameters its create function accepts: `with` closes it, closing again does nothing, and what it borrowed stays open.
Nothing is computed here: no method that launches a kernel is called."""
import contextlib
import operator

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GMM_1x1 = {"log_consts": np.zeros(1), "means": np.zeros((1, 1)), "inv_covs": np.ones((1, 1))}      # one component, one dimension


@pytest.fixture(scope="module")
def models(golden):
    """the parameter dicts of the models the golden fixtures provide"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    s = golden("speaker_gmm_ref.npz")
    svm = golden("scrubjay_svm.npz")
    return {"stop": dict(golden("stop_model.npz")), "svm": {k: svm[k] for k in svm.files},
            "target": {k: s[f"target_{k}"] for k in ("means", "inv_covs", "log_consts")},
            "ubm": {k: s[f"ubm_{k}"] for k in ("means", "inv_covs", "log_consts")}}


def _lent(stack, models):
    """a plan, a stop model and a speaker model for the borrowers, closed by `stack` after them"""
    import dsp_amd
    return (stack.enter_context(dsp_amd.MfccPlan()), stack.enter_context(dsp_amd.StopModel(models["stop"])),
            stack.enter_context(dsp_amd.SpeakerModel(models["target"], models["ubm"])))


def _scrubjay_scanner(stack, models):
    from dsp_amd import scrubjay
    sj = scrubjay.ScrubJay(models["svm"])
    stack.enter_context(sj.plan)
    stack.enter_context(sj.svm)
    return scrubjay.ScrubJayScanner(sj)


def _makers():
    import dsp_amd
    from dsp_amd import scrubjay
    return {
        "MfccPlan": lambda stack, m: dsp_amd.MfccPlan(),
        "SvmModel": lambda stack, m: scrubjay.SvmModel(m["svm"]),
        "SvmTrainer": lambda stack, m: scrubjay.SvmTrainer(1),
        "ScrubJayScanner": _scrubjay_scanner,
        "Resampler": lambda stack, m: dsp_amd.Resampler(8000, 16000),
        "StreamResampler": lambda stack, m: dsp_amd.StreamResampler(8000, 16000, 1),
        "Augmenter": lambda stack, m: dsp_amd.Augmenter(pad="zero", max_term=1),
        "StopModel": lambda stack, m: dsp_amd.StopModel(m["stop"]),
        "StopTrainer": lambda stack, m: dsp_amd.StopTrainer(1, 1, (1, 1, 1, 1)),
        "SpeakerModel": lambda stack, m: dsp_amd.SpeakerModel(m["target"], m["ubm"]),
        "Scanner": lambda stack, m: dsp_amd.Scanner(*_lent(stack, m)),
        "StreamSession": lambda stack, m: dsp_amd.StreamSession(_lent(stack, m)[0], 1),
        "Cmvn": lambda stack, m: dsp_amd.Cmvn(1, 2),
        "SpeakerEnroller": lambda stack, m: dsp_amd.SpeakerEnroller(GMM_1x1),
        "SpeakerVerifier": lambda stack, m: dsp_amd.SpeakerVerifier(GMM_1x1),
        "Segmenter": lambda stack, m: dsp_amd.Segmenter(),
        "TrialEvaluator": lambda stack, m: dsp_amd.TrialEvaluator(),
        "ScoreCalibrator": lambda stack, m: dsp_amd.ScoreCalibrator(),
        "UbmTrainer": lambda stack, m: dsp_amd.UbmTrainer(1, 1),
    }


HANDLE_CLASSES = ["MfccPlan", "SvmModel", "SvmTrainer", "ScrubJayScanner", "Resampler", "StreamResampler", "Augmenter", "StopModel", "StopTrainer",
                  "SpeakerModel", "Scanner", "StreamSession", "Cmvn", "SpeakerEnroller", "SpeakerVerifier", "Segmenter", "TrialEvaluator",
                  "ScoreCalibrator", "UbmTrainer"]
BORROWS = {"Scanner": ("plan", "stop", "speaker"), "StreamSession": ("plan",), "ScrubJayScanner": ("scrubjay.plan", "scrubjay.svm")}


def test_the_cases_are_the_package_s_handle_classes():
    import dsp_amd
    from dsp_amd import lib, scrubjay
    assert sorted(_makers()) == sorted(HANDLE_CLASSES) and len(HANDLE_CLASSES) == 19
    for name in HANDLE_CLASSES:
        assert issubclass(getattr(dsp_amd, name, None) or getattr(scrubjay, name), lib.Handle), name


@pytest.mark.parametrize("name", HANDLE_CLASSES)
def test_with_closes_the_handle_and_a_second_close_does_nothing(name, models):
    with contextlib.ExitStack() as stack:
        with _makers()[name](stack, models) as obj:
            assert type(obj).__name__ == name and obj._h and obj._h.value
        assert obj._h is None
        obj.close()
        obj.__del__()
        assert obj._h is None
        for lender in BORROWS.get(name, ()):                           # a borrower closes nothing it was lent
            assert operator.attrgetter(lender)(obj)._h, lender


def test_speaker_front_end_closes_both_of_its_handles():
    import dsp_amd
    with dsp_amd.SpeakerFrontEnd() as fe:
        plan, cmvn = fe.plan, fe.cmvn
        assert plan._h and cmvn._h
    assert fe.plan is None and fe.cmvn is None and plan._h is None and cmvn._h is None
    fe.close()
    fe.__del__()


def test_a_session_with_a_resampler_in_front_closes_both():
    import dsp_amd
    with dsp_amd.MfccPlan() as plan:
        with dsp_amd.StreamSession(plan, 1, rate_in=8000) as sess:
            rs = sess.resampler
            assert sess._h and rs._h and (rs.rate_in, rs.rate_out) == (8000, plan.cfg.sample_rate)
        assert sess._h is None and sess.resampler is None and rs._h is None
        sess.close()
        assert plan._h
    assert plan._h is None
