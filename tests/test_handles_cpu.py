"""CPU: every dsp_*_create / dsp_*_destroy pair of include/dsp_amd.h, called through ctypes with the smallest arguments each takes.
What a create refuses, in which order, what it answers without a GPU and what it leaves in *out are pinned here for the handles' one
create / destroy path (dsp_amd/csrc/capi_util.hpp); nothing is launched."""
import ctypes as C
import os
import re

import pytest

import dsp_amd
from dsp_amd import lib as dl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV = 0, -1, -2

# the arrays the rows point into (kept alive here: the rows hold their addresses)
_F = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
_D = (C.c_double * 1)(1.0)
_NAN = (C.c_double * 1)(float("nan"))
_I8, _I16, _I32 = (C.c_int8 * 1)(1), (C.c_int16 * 1)(1), (C.c_int32 * 1)(1)
_UNITS = (C.c_int * 4)(1, 1, 1, 1)
_DEVS = (C.c_int * 1)(0)
_SCAN = dl.ScanConfig(2, 1)


def _addr(a):
    return C.cast(a, C.c_void_p)


def _stop_params(last_units=1):
    p = dl.StopModelParams()
    p.n_coef, p.max_frames = 1, 1
    p.units[:] = [1, 1, 1, last_units]
    p.scaler_mean = p.scaler_scale = C.addressof(_F)
    for l in range(4):
        p.kernel[l] = p.bias[l] = C.addressof(_F)
    return p


def _gmm(k=1):
    return dl.GmmParams(k, 1, _addr(_I8), _addr(_I32), _addr(_I16))


def _fgmm(k=1, log_consts=_D):
    return dl.GmmFloatParams(k, 1, _addr(log_consts), _addr(_D), _addr(_D))


_CFG = dsp_amd.default_config()
_BAD_CFG = dsp_amd.default_config(n_fft=256)
_STOP, _STOP_BAD = _stop_params(), _stop_params(last_units=2)
_GMM, _GMM2 = _gmm(), _gmm(2)
_FGMM, _FGMM0, _FGMM_NAN = _fgmm(), _fgmm(0), _fgmm(log_consts=_NAN)
ref = C.byref

# name -> (arguments in front of `out`, or None where none are valid without a handle only a GPU gives;
#          the code without a GPU; the text for out == NULL;
#          [(arguments, text)]: refused for the argument, before any device is asked -- where two are wrong, the first in the order kept)
HANDLES = {
    "mfcc_plan": ((ref(_CFG), 0), ENODEV, "cfg/out is NULL", [((ref(_BAD_CFG), 0), "n_fft")]),
    "svm": ((0, 2, 1, _addr(_F), _addr(_F), _addr(_F), _addr(_F), 1.0, 0.0, 0.0, 0.0), ENODEV, "bad argument",
            [((0, 0, 1, _addr(_F), _addr(_F), _addr(_F), _addr(_F), 1.0, 0.0, 0.0, 0.0), "bad argument")]),
    "stop_model": ((ref(_STOP), 0), ENODEV, "out is NULL", [((ref(_STOP_BAD), 0), "the last layer must have one unit"), ((None, 0), "bad stop-model parameters")]),
    "speaker_model": ((ref(_GMM), ref(_GMM), 0), ENODEV, "out is NULL",
                      [((ref(_GMM), ref(_GMM2), 0), "target and UBM must have the same shape"), ((None, ref(_GMM), 0), "bad GMM parameters")]),
    "scanner": (None, None, "out is NULL", [((None, None, None, ref(_SCAN)), "plan is NULL")]),
    "scrubjay_scanner": (None, None, "out is NULL", [((None, None, ref(_SCAN)), "plan and SVM must not be NULL")]),
    "stream_session": (None, None, "out is NULL", [((None, None, None, ref(_SCAN), 1, 1, 0, 0), "plan is NULL")]),
    "resampler": ((0, 8000, 16000), ENODEV, "out is NULL", [((0, 0, 16000), "rate_in and rate_out must be >= 1")]),
    "stream_resampler": ((0, 8000, 16000, 1, 1, 0, 0), ENODEV, "out is NULL",
                         [((0, 8000, 16000, 1, 2, 0, 0), "float samples are mono"), ((0, 8000, 16000, -1, 1, 0, 0), "n_streams must be in [0, 2^31)")]),
    "augmenter": ((0, dl.PAD_REFLECT, 256), ENODEV, "out is NULL", [((0, 7, 256), "pad_mode must be"), ((0, dl.PAD_ZERO, 0), "max_term must be 1 .. 1024")]),
    "cmvn": ((0, 1, 2), ENODEV, "out is NULL", [((0, 0, 2), "d must be 1 .. 16"), ((0, 1, 1), "window must be 2 ..")]),
    "speaker_enroller": ((ref(_FGMM), 0), ENODEV, "out is NULL",
                         [((ref(_FGMM0), 0), "ubm: k must be 1 .. 64, got 0"), ((ref(_FGMM_NAN), 0), "must be finite in float32"),
                          ((None, 0), "ubm and its arrays must not be NULL")]),
    "speaker_verifier": ((ref(_FGMM), 0), OK, "out is NULL",
                         [((ref(_FGMM0), -1), "ubm: k must be 1 .. 64, got 0"), ((ref(_FGMM_NAN), -1), "device index out of range"),
                          ((ref(_FGMM_NAN), 0), "must be finite in float32")]),
    "ubm_trainer": ((0, 1, 1), OK, "out is NULL", [((-1, 0, 1), "k must be 1 .. 64, got 0"), ((-1, 1, 0), "d must be 1 .. 16, got 0"),
                                                    ((-1, 1, 1), "device index out of range")]),
    "svm_trainer": ((0, 1), OK, "out is NULL", [((-1, 0), "device index out of range"), ((0, 0), "n_features must be >= 1, got 0")]),
    "stop_trainer": ((0, 1, 1, _UNITS), OK, "out is NULL", [((-1, 0, 1, _UNITS), "device index out of range"), ((0, 0, 1, _UNITS), "n_coef must be >= 1, got 0"),
                                                            ((0, 1, 1, None), "units is NULL")]),
    "segmenter": ((0,), OK, "out is NULL", [((-1,), "device index out of range")]),
    "trial_evaluator": ((0,), OK, "out is NULL", [((-1,), "device index out of range")]),
    "calibrator": ((0,), OK, "out is NULL", [((-1,), "device index out of range")]),
    # not handles of one GPU, but pairs of the header all the same
    "gather": ((_DEVS, 1), ENODEV, "bad argument", [((_DEVS, 0), "1 .. 64 devices"), ((None, 1), "1 .. 64 devices")]),
    "classify_ctx": ((0,), ENODEV, "bad argument", []),
}
NAMES = sorted(HANDLES)


def _pair(name):
    L = dl.load()
    return getattr(L, f"dsp_{name}_create"), getattr(L, f"dsp_{name}_destroy")


def test_the_table_holds_every_pair_of_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsp_amd.h")).read(), flags=re.S)
    created = set(re.findall(r"\bdsp_(\w+)_create\s*\(", text))
    assert created == set(re.findall(r"\bdsp_(\w+)_destroy\s*\(", text)) == set(HANDLES)
    assert len(HANDLES) == 19 + 2


@pytest.mark.parametrize("name", NAMES)
def test_out_null_is_refused_by_name(name):
    create, _ = _pair(name)
    valid, _, text, bad = HANDLES[name]
    args = valid if valid is not None else bad[0][0]
    assert create(*args, None) == EINVAL
    assert dl.last_error() == text


@pytest.mark.parametrize("name", NAMES)
def test_destroy_of_null_is_a_no_op(name):
    _, destroy = _pair(name)
    destroy(None)
    destroy(None)


@pytest.mark.parametrize("name,args,text", [(n, a, t) for n in NAMES for a, t in HANDLES[n][3]])
def test_a_bad_argument_is_refused_before_the_device_is_asked(name, args, text):
    create, _ = _pair(name)
    h = C.c_void_p(0xDEAD)
    assert create(*args, ref(h)) == EINVAL
    assert text in dl.last_error() and "no HIP device" not in dl.last_error()
    # *out is NULL after a failure -- but for dsp_svm_create, which refuses its arguments, out among them, in one check in front of its
    # first store to *out
    assert h.value == (0xDEAD if name == "svm" else None)


@pytest.mark.parametrize("name", [n for n in NAMES if HANDLES[n][0] is not None])
def test_valid_arguments_without_a_gpu(name):
    """DSP_ENODEV and *out == NULL from a create that touches a device, "no HIP device" in the text; DSP_OK from one that does not -- the
    verifier, the three trainers and the three score-matrix stages, which report a missing device in the first call that launches --
    and its destroy then works without a device.  With a GPU the second kind is checked all the same; the first kind is
    tests/test_gpu_handles.py's."""
    create, destroy = _pair(name)
    valid, code, _, _ = HANDLES[name]
    no_gpu = dl.load().dsp_device_count() <= 0
    if code == ENODEV and not no_gpu:
        return
    h = C.c_void_p(0xDEAD)
    assert create(*valid, ref(h)) == code
    if code == OK:
        assert h.value
        destroy(h)
    else:
        assert h.value is None and "no HIP device" in dl.last_error()
