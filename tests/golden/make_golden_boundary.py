#!/usr/bin/env python3
"""Goldens of the reference's side of two drop-in boundaries, so that the tests of those boundaries run where the reference
checkout is absent.

Runs only in the build container (needs /root/reference and oracle/_ref, the reference's mfcc.c compiled unmodified).
Writes data only:
  fft_ref.npz         in_<k> / out_<k>: the frames of tests/signals.py fft_entry_frames() and what the COMPILED REFERENCE's
                      fft_real_forward (2fa/audio/word/c/mfcc.c:16) returns for them; n_frames
  cxx_abi_ref.npz     undefined: the mangled names of the classifier functions that examples/main_classify.cpp references when
                      it is compiled against the reference's own sync/lib/classifier.h (g++ -c, nm -u)

    python tests/golden/make_golden_boundary.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("DSP_REF", "/root/reference")

from dsp_amd import lib as dl  # noqa: E402  (the names only: nothing is loaded)
from oracle import oracle as O  # noqa: E402
from tests import signals as S  # noqa: E402
from tests.test_boundary_cxx import classifier_refs  # noqa: E402


def main():
    O.build(force=True)
    assert O.have_ref(), "oracle/_ref not built (reference checkout missing?)"
    out = {}
    frames = S.fft_entry_frames(np.random.default_rng(8))
    for k, x in enumerate(frames):
        x = np.ascontiguousarray(x, np.float32)
        spec = np.empty(1024, np.float32)
        O.ref_mfcc_lib().fft_real_forward(x, spec)
        out[f"in_{k}"], out[f"out_{k}"] = x, spec
    out["n_frames"] = np.int32(len(frames))
    np.savez_compressed(os.path.join(HERE, "fft_ref.npz"), **out)
    refs = classifier_refs(["-DUSE_REFERENCE_HEADER", "-I" + os.path.join(REF, "sync", "lib")])
    assert len(refs) == len(dl.CXX_SYMBOLS), refs
    np.savez_compressed(os.path.join(HERE, "cxx_abi_ref.npz"), undefined=np.array(refs))
    print("fft_ref.npz:", len(frames), "frames; cxx_abi_ref.npz:", refs)


if __name__ == "__main__":
    main()
