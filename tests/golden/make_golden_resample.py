#!/usr/bin/env python3
"""The reference's own capture dump through scipy.signal.resample_poly, as the resampler's known-answer fixture.

Runs only where the reference checkout and scipy are present.  Writes tests/golden/resample_kat.npz -- data only:
    x             float64 [6768]   the samples of sound-processing/bird_control.txt (the firmware's ADC capture, one line of decimals)
    y_10000       float64          scipy.signal.resample_poly(x, 8, 5): 10 kHz -> 16 kHz, the ratio sound-processing/pcm_to_wav.py names
    y_9000        float64          scipy.signal.resample_poly(x, 16, 9): 9 kHz -> 16 kHz (sync/sync.cpp:186 "Actually closer to 9000")
    scipy_version
tests/test_resample_cpu.py holds tests/resample_ref.py (the definition restated from the formula) to these."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("DSP_REF", "/root/reference")


def main():
    import scipy
    from scipy.signal import resample_poly
    with open(os.path.join(REF, "sound-processing", "bird_control.txt")) as f:
        x = np.array([float(t) for t in f.read().replace("\n", ",").split(",") if t.strip()], np.float64)
    assert x.size == 6768, x.size
    out = {"x": x, "y_10000": resample_poly(x, 8, 5), "y_9000": resample_poly(x, 16, 9), "scipy_version": np.array(scipy.__version__)}
    assert out["y_10000"].dtype == np.float64 and out["y_10000"].size == -(-x.size * 8 // 5) and out["y_9000"].size == -(-x.size * 16 // 9)
    path = os.path.join(ROOT, "tests", "golden", "resample_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
