"""What tests/test_vad_cpu.py and tests/test_gpu_vad.py share: the four framings of the issue, the seeded signal (room noise with
bursts of speech-like noise), clip lengths that give a wanted number of rows, and the ctypes structs of a configuration."""
import ctypes as C

import numpy as np

from dsp_amd import lib as dl
from tests import vad_ref as V

# (frame_length, hop_length, framing): the speaker plan, the reference's default plan, a 512-point plan, the scrub-jay stream plan
FRAMINGS = {"400/160 centre": (400, 160, V.CENTER), "400/160 complete": (400, 160, V.COMPLETE), "512/160 complete": (512, 160, V.COMPLETE),
            "2048/1024 stream": (2048, 1024, V.STREAM)}
REFERENCES = {"absolute": V.REF_ABSOLUTE, "max": V.REF_MAX, "mean": V.REF_MEAN}


def signal(seed, n):
    """float32 [n]: noise of amplitude 1e-3; stretches of 800 .. 6400 samples, every second one on average with a Gaussian burst of
    amplitude 0.05 .. 0.5 on top"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1e-3, n)
    at = 0
    while at < n:
        length = int(rng.integers(800, 6401))
        if rng.random() < 0.5:
            stop = min(n, at + length)
            x[at:stop] += rng.normal(0.0, rng.uniform(0.05, 0.5), stop - at)
        at += length
    return x.astype(np.float32)


def samples_for(rows, frame_length, hop, framing, extra=0):
    """a clip length that gives exactly `rows` rows under the framing; extra < hop more samples leave the count as it is"""
    assert 0 <= extra < hop
    if rows == 0:
        return 0
    if framing == V.CENTER:
        n = (rows - 1) * hop + extra
        return max(n, 1)
    if framing == V.STREAM:
        return (rows - 1) * hop + 1 + extra
    return frame_length + (rows - 1) * hop + extra


def config(frame_length, hop, framing, reference=V.REF_MAX, ratio=1e-6, floor=0.0, context=0, proportion=0.6, pad=0):
    return dl.VadConfig(frame_length, hop, framing, reference, ratio, floor, context, proportion, pad)


def geometry(cfg):
    geo = dl.VadGeometry()
    rc = dl.load().dsp_vad_geometry_for(C.byref(cfg), C.byref(geo))
    assert rc == 0, dl.last_error()
    return geo


def how(cfg):
    """the keyword arguments of vad_ref.decide / run that restate a VadConfig"""
    return dict(reference=cfg.reference, ratio=cfg.threshold_ratio, floor=cfg.floor_power, context=cfg.context_frames, proportion=cfg.proportion,
                pad=cfg.pad_frames)
