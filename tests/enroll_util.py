"""What tests/test_enroll_cpu.py and tests/test_gpu_enroll.py share: the two MAP modes, the golden fixture with the rows the library is
given (computed once per session), and the build of examples/main_enroll.c."""
import os
import subprocess
import wave

import numpy as np

from tests import enroll_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dsp_amd")
MODES = {"relevance": dict(mode="relevance", relevance_factor=16.0), "fixed": dict(mode="fixed_alpha", fixed_alpha=0.7)}
_cache = {}


def fixture(golden):
    """(tests/golden/speaker_enroll_ref.npz, the float UBM, the float32 rows the library is given)"""
    if "fx" not in _cache:
        z = golden("speaker_enroll_ref.npz")
        ubm = {key: z[f"ubm_{key}_d"] for key in ("log_consts", "means", "inv_covs")}
        _cache["fx"] = (z, ubm, E.fixture_feats(z))
    return _cache["fx"]


def build_main_enroll(out):
    """examples/main_enroll.c with gcc, as its header comment shows -> the executable's path"""
    import dsp_amd
    dsp_amd.load()                                  # builds libdsp_amd.so when stale
    cmd = ["gcc", "-O2", "-std=gnu11", "-D__HIP_PLATFORM_AMD__", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
           os.path.join(ROOT, "examples", "main_enroll.c"), f"-L{LIBDIR}", "-ldsp_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return out


def write_wav(path, pcm, rate=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, np.int16).tobytes())
