#!/usr/bin/env python3
"""Writes tests/golden/speaker_frontend_ref.npz: recorded speech for the whole-chain test of tests/test_gpu_mfcc400.py.

    python tests/golden/make_golden_speaker_frontend.py <path to the reference checkout>

From the reference only recorded data is taken: the int16 samples of four 16 kHz mono clips of 2fa/audio/data/gmm_test/ (two of the target
speaker's label 0 / 1 files each way), 32 710 samples in all, stored as one array with the clips' offsets.  The expected values are not
stored: the test computes them with the float64 restatements (tests/mfcc400_ref.py, enroll_ref.py, verify_ref.py)."""
import os
import sys
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLIPS = ["0_lucas_13", "0_nicolas_3", "0_theo_28", "1_nicolas_16"]


def read_wav(path):
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000), path
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").copy()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    pcm = [read_wav(os.path.join(sys.argv[1], "2fa/audio/data/gmm_test", name + ".wav")) for name in CLIPS]
    offsets = np.concatenate([[0], np.cumsum([p.size for p in pcm])]).astype(np.int64)
    out = os.path.join(HERE, "speaker_frontend_ref.npz")
    np.savez_compressed(out, pcm=np.concatenate(pcm), offsets=offsets, names=np.array(CLIPS))
    print(out, offsets.tolist(), os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
