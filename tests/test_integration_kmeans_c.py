"""examples/main_train_ubm.c at the linker and on the GPU: a plain C caller of dsp_kmeans_train_ubm_device and dsp_gmm_quantize, built
with gcc against include/dsp_amd.h and libdsp_amd.so as tests/test_integration_c.py builds the others.  CPU: it compiles, links and
fails loudly without a GPU.  GPU: its tables are dsp_amd.UbmTrainer.fit(init="kmeans", n_init=2) through dsp_amd.quantize_gmm."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dsp_amd
from tests import kmeans_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "dsp_amd")
needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")


def _build(tmp_path):
    dsp_amd.load()                                  # builds libdsp_amd.so when stale
    exe = str(tmp_path / "main_train_ubm")
    cmd = ["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include",
           os.path.join(ROOT, "examples", "main_train_ubm.c"), f"-L{LIBDIR}", "-ldsp_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _rows_file(tmp_path, x):
    path = str(tmp_path / "rows.txt")
    with open(path, "w") as f:
        f.write(f"{x.shape[0]} {x.shape[1]}\n")
        np.savetxt(f, x, fmt="%.9g")
    return path


def _rows(n=3000, k=8, d=13):
    rng = np.random.default_rng(31)
    return (rng.normal(0.0, 1.0, (k, d))[rng.integers(0, k, n)] + rng.normal(0.0, 0.4, (n, d))).astype(np.float32)


@needs_gcc
def test_c_caller_links_and_fails_loudly_without_a_gpu(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-k", "8", _rows_file(tmp_path, _rows(64))], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and ("no HIP device" in r.stderr or "hipMalloc" in r.stderr)      # loud, no CPU fallback


@needs_gcc
@pytest.mark.gpu
def test_c_caller_trains_the_tables_the_python_wrapper_trains(tmp_path):
    import torch
    x = _rows()
    exe = _build(tmp_path)
    r = subprocess.run([exe, "-k", "8", "-s", "42", _rows_file(tmp_path, x)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fit = dsp_amd.UbmTrainer(8, 13).fit(torch.from_numpy(x).cuda(), init="kmeans", n_init=2, seed=42)
    tables, saturated = dsp_amd.quantize_gmm(fit)
    for name, key in (("ubm_log_consts", "log_consts"), ("ubm_means", "means"), ("ubm_inv_covs", "inv_covs")):
        body = re.search(name + r"\[K\](?:\[D\])? = \{(.*?)\};", r.stdout, re.S).group(1)
        got = np.array([int(v) for v in re.findall(r"-?\d+", body)]).reshape(tables[key].shape)
        assert np.array_equal(got, tables[key]), name
    kept = [line for line in r.stdout.splitlines() if "<- kept" in line]
    assert len(kept) == 1 and f"restart {fit['report']['winner']}:" in kept[0]
    for i, rep in enumerate(fit["report"]["restarts"]):
        assert f"restart {i}: first seed row {int(rep['rows'][0])}, k-means {rep['kmeans_n_iter']} iterations ({rep['kmeans_stop']}" in r.stdout
        assert rep["rows"][0] == min(int(K.draw(K.restart_seed(42, i), 0, 0) * x.shape[0]), x.shape[0] - 1)
