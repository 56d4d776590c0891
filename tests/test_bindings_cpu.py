"""CPU: the Python binding layer itself -- every prototype of lib.PROTOTYPES against include/dsp_amd.h, the lifecycle of lib.Handle on
a stub library, and that every handle class names a destroy function the header declares.  No compute call is made here."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import dsp_amd
from dsp_amd import lib as dl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RETURNS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "void": None, "const char *": C.c_char_p}
SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "uint64_t": C.c_uint64,
           "unsigned long long": C.c_uint64}
POINTER = "a pointer"


def _declarations():
    """include/dsp_amd.h without comments and preprocessor lines -> {name: (return type, [parameter class])}, a parameter's class
    being POINTER for any pointer or array and the ctypes type of SCALARS otherwise."""
    text = open(os.path.join(ROOT, "include", "dsp_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(compute_mfcc|fft_real_forward|classify\w*|dsp_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, f"{name} is declared twice"
        classes = []
        for p in (" ".join(p.split()) for p in params.split(",")):
            if p in ("void", ""):
                assert params.strip() in ("void", ""), (name, params)
            elif "*" in p or "[" in p:
                classes.append(POINTER)
            else:
                classes.append(SCALARS[p.rsplit(" ", 1)[0]])      # (KeyError: a scalar type this test does not know yet)
        out[name] = (RETURNS[" ".join(ret.replace("*", " * ").split())], classes)
    return out


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def _mismatches(name, prototype, declared):
    """what is wrong with one entry of PROTOTYPES against the header's declaration of `name` (nothing: [])"""
    (restype, argtypes), (ret, classes) = prototype, declared
    bad = []
    if len(argtypes) != len(classes):
        return [f"{name}: {len(argtypes)} argtypes, the header declares {len(classes)} parameters"]
    if restype is not ret:
        bad.append(f"{name}: restype {restype}, the header returns {ret}")
    for i, (got, want) in enumerate(zip(argtypes, classes)):
        if not (_is_pointer(got) if want is POINTER else got is want):
            bad.append(f"{name}: argument {i} is {got}, the header declares {want}")
    return bad


def test_every_prototype_agrees_with_the_header():
    declared = _declarations()
    assert set(dl.PROTOTYPES) == set(declared) and dl.SYMBOLS == list(dl.PROTOTYPES)
    assert list(dl.PROTOTYPES) == list(declared), "PROTOTYPES is kept in the header's order"
    bad, checked = [], 0
    for name, prototype in dl.PROTOTYPES.items():
        bad += _mismatches(name, prototype, declared[name])
        checked += 1
    assert not bad, "\n".join(bad)
    assert checked == len(declared) >= 198
    L = dsp_amd.load()                                   # and load() has applied the table to the library as it stands
    for name, (restype, argtypes) in dl.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_a_wrong_prototype_is_found():
    declared = _declarations()
    name = "dsp_mfcc_frames_device"
    restype, argtypes = dl.PROTOTYPES[name]
    assert not _mismatches(name, (restype, argtypes), declared[name])
    at = argtypes.index(C.c_long)
    wrong = argtypes[:at] + [C.c_int] + argtypes[at + 1:]                   # one c_long turned into c_int
    assert _mismatches(name, (restype, wrong), declared[name]) == [f"{name}: argument {at} is {C.c_int}, the header declares {C.c_long}"]
    assert _mismatches(name, (restype, argtypes[:-1]), declared[name])      # a missing argument
    assert _mismatches(name, (C.c_long, argtypes), declared[name])          # another return type
    assert _mismatches(name, (restype, [C.c_long] + argtypes[1:]), declared[name])      # a scalar where the header has a pointer


class _StubLibrary:
    """stands in for the loaded library: stub_create hands out a token (or fails), stub_destroy records its calls"""

    TOKEN = 0x5151

    def __init__(self, create_rc=0, destroy_raises=False):
        self.create_rc, self.destroy_raises, self.created, self.destroyed = create_rc, destroy_raises, [], []

    def stub_create(self, *args):
        *given, out = args
        self.created.append(given)
        if self.create_rc >= 0:
            out._obj.value = self.TOKEN
        return self.create_rc

    def stub_destroy(self, h):
        self.destroyed.append(h.value)
        if self.destroy_raises:
            raise RuntimeError("destroy failed")

    def dsp_last_error(self):
        return b"the stub refuses"


class _Thing(dl.Handle):
    _destroy = "stub_destroy"

    def __init__(self, *args):
        self.device = 0
        self._create("stub_create", *args)


@pytest.fixture
def stub(monkeypatch):
    def install(**how):
        s = _StubLibrary(**how)
        monkeypatch.setattr(dl, "load", lambda: s)
        return s
    return install


def test_handle_creates_once_and_destroys_once(stub):
    s = stub()
    t = _Thing(3, "x")
    assert s.created == [[3, "x"]] and t._L is s and t._h.value == s.TOKEN      # the out-handle went last, the arguments as given
    t.close()
    assert s.destroyed == [s.TOKEN] and t._h is None
    t.close()
    t.__del__()
    assert s.destroyed == [s.TOKEN]                       # a second close and the collection do nothing


def test_handle_closes_when_a_with_block_ends_or_raises(stub):
    s = stub()
    with _Thing() as t:
        assert t._h.value == s.TOKEN and s.destroyed == []
    assert t._h is None and s.destroyed == [s.TOKEN]
    with pytest.raises(KeyError):
        with _Thing() as u:
            raise KeyError("inside")
    assert u._h is None and s.destroyed == [s.TOKEN] * 2


def test_a_failed_create_leaves_a_closable_object(stub):
    s = stub(create_rc=-1)
    t = _Thing.__new__(_Thing)
    with pytest.raises(dl.DspError, match=r"stub_create failed \(-1\): the stub refuses"):
        t.__init__()
    assert t._h is None
    t.close()
    t.__del__()
    assert s.destroyed == []
    bare = _Thing.__new__(_Thing)                         # a constructor that raised before it reached _create
    bare.close()
    bare.__del__()
    assert bare._h is None and bare._L is None


def test_del_swallows_a_destroy_that_raises(stub):
    s = stub(destroy_raises=True)
    t = _Thing()
    with pytest.raises(RuntimeError, match="destroy failed"):
        t.close()
    t.__del__()                                           # the same failure, swallowed
    assert s.destroyed == [s.TOKEN] * 2


def test_current_stream_takes_a_tensor_or_a_device_index(monkeypatch):
    import torch

    class Stream:
        cuda_stream = 0x77

    asked = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: asked.append(device) or Stream())
    t = torch.zeros(1)
    assert dl.current_stream(t).value == 0x77 and dl.current_stream(3).value == 0x77 and asked == [t.device, 3]
    thing = _Thing.__new__(_Thing)
    thing.device = 2
    assert isinstance(thing._stream(), C.c_void_p) and asked[-1] == 2


def _package_classes():
    """every class defined in a module of the package, by its qualified name"""
    seen = {}
    sources = sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, "dsp_amd")) if f.endswith(".py") and f != "__init__.py")
    assert "consumers" in sources and "scrubjay" in sources
    for module in [importlib.import_module(f"dsp_amd.{name}") for name in sources]:
        for _, cls in inspect.getmembers(module, inspect.isclass):
            if cls.__module__.startswith("dsp_amd."):
                seen[f"{cls.__module__}.{cls.__qualname__}"] = cls
    return seen


# the destroy functions of include/dsp_amd.h whose handles have no Python class: dsp_amd.dist gathers through torch.distributed, and
# the classifier's contexts are made by the C callers of dsp_classify_batch_device_ctx
DESTROYS_WITHOUT_A_CLASS = {"dsp_gather_destroy", "dsp_classify_ctx_destroy"}


def test_every_handle_class_names_a_destroy_of_its_own():
    classes = _package_classes()
    handles = {name: cls for name, cls in classes.items() if issubclass(cls, dl.Handle) and cls is not dl.Handle}
    assert len(handles) == 19 and issubclass(dsp_amd.SpeakerFrontEnd, dl.Closing) and not issubclass(dsp_amd.SpeakerFrontEnd, dl.Handle)
    named = {}
    for name, cls in handles.items():
        assert dl.PROTOTYPES.get(cls._destroy) == (None, [C.c_void_p]), f"{name}._destroy = {cls._destroy!r}"
        assert cls._destroy not in named, f"{name} and {named.get(cls._destroy)} both name {cls._destroy}"
        named[cls._destroy] = name
    destroys = {name for name in dl.PROTOTYPES if name.endswith("_destroy")}
    assert destroys - set(named) == DESTROYS_WITHOUT_A_CLASS and set(named) <= destroys
    for name, cls in classes.items():                     # and the lifecycle is written once
        assert ("__del__" in vars(cls)) == (cls is dl.Closing), name
        if cls is not dl.Closing:
            assert "__enter__" not in vars(cls) and "__exit__" not in vars(cls), name


def test_a_real_handle_on_the_cpu():
    """SpeakerVerifier touches no device when it is created (tests/test_verify_cpu.py relies on the same)."""
    ubm = {"log_consts": np.zeros(1), "means": np.zeros((1, 1)), "inv_covs": np.ones((1, 1))}
    with dsp_amd.SpeakerVerifier(ubm) as v:
        assert v._h and v._L is dsp_amd.load() and (v.k, v.d, v.device) == (1, 1, 0)
    assert v._h is None
    v.close()
    assert v._h is None
    with pytest.raises(ValueError, match="k must be 1 .. 64"):
        dsp_amd.SpeakerVerifier({"log_consts": np.zeros(65), "means": np.zeros((65, 1)), "inv_covs": np.ones((65, 1))})


def test_offsets_array_words_its_two_nouns():
    for what, unit in (("frame_offsets", "rows"), ("window_offsets", "windows")):
        assert dl.offsets_array([0, 3, 3, 9], what, unit).tolist() == [0, 3, 3, 9] and dl.offsets_array([4], what, unit).dtype == np.int64
        for bad in ([], [[0, 1]]):
            with pytest.raises(ValueError, match=f"^{what} must hold n_recordings \\+ 1 {unit}$"):
                dl.offsets_array(bad, what, unit)
        for bad in ([-1, 2], [0, 5, 4]):
            with pytest.raises(ValueError, match=f"^{what} must be non-negative and non-decreasing$"):
                dl.offsets_array(bad, what, unit)
