"""examples/main_train_stop.c at the linker and on the GPU: a plain C caller of dsp_stop_train_*, dsp_stop_model_from_training and
dsp_classify_signal, built with gcc against include/dsp_amd.h and libdsp_amd.so as tests/test_integration_kmeans_c.py builds its
example.  CPU: it compiles, links and fails loudly without a GPU.  GPU: it trains from audio and classify_signal gets every clip right."""
import os
import re
import shutil
import subprocess

import pytest

import dsp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dsp_amd")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")


def _build(tmp_path):
    dsp_amd.load()                                  # builds libdsp_amd.so when stale
    exe = str(tmp_path / "main_train_stop")
    cmd = ["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
           os.path.join(ROOT, "examples", "main_train_stop.c"), f"-L{LIBDIR}", "-ldsp_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@needs_gcc
def test_c_caller_links_and_fails_loudly_without_a_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "-n", "4"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-n", "8", "-s", "1", "-e", "1"], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and ("no HIP device" in r.stderr or "hipMalloc" in r.stderr)      # loud, no CPU fallback


@needs_gcc
@pytest.mark.gpu
def test_c_caller_trains_and_classifies(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "-n", "24", "-s", "8", "-e", "40"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(re.findall(r"^seed +\d+:", r.stdout, re.M)) == 8 and "classify_signal: 24 of 24 clips right" in r.stdout
    kept = int(re.search(r"keeping seed (\d+)", r.stdout).group(1))
    losses = [float(v) for v in re.findall(r"val_loss ([0-9.eE+-]+|nan)", r.stdout)]
    assert losses[kept] == min(v for v in losses if v == v)
