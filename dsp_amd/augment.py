"""Augmenting raw training clips on the GPU (include/dsp_amd.h dsp_augment_*): the time stretch, pitch shift and
additive noise of cepstrum/train.py's augment() for a ragged batch of float32 clips in HBM, and the complex STFT / inverse STFT
(n_fft 2048, hop 512, periodic Hann) they are made of.  ctypes and torch plumbing only: every rule lives in the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib

N_FFT, HOP, BINS = 2048, 512, 1025
_PADS = {"reflect": _lib.PAD_REFLECT, "zero": _lib.PAD_ZERO}
_KINDS = {"stretch": _lib.AUGMENT_STRETCH, "pitch": _lib.AUGMENT_PITCH, "noise": _lib.AUGMENT_NOISE}


def _rate(rate) -> float:
    rate = float(rate)
    if not (np.isfinite(rate) and 0.125 <= rate <= 8.0):
        raise ValueError("rate must be finite and in [1/8, 8]")
    return rate


def stft_frames(n: int) -> int:
    """T = 1 + n // 512: the frames of a clip of n samples."""
    if n < 0:
        raise ValueError("n must be >= 0")
    return int(_lib.check(_lib.load().dsp_stft_frames(int(n)), "dsp_stft_frames"))


def stretch_frames(n_frames: int, rate: float) -> int:
    """T_out = ceil(T / rate)."""
    if n_frames < 0:
        raise ValueError("n_frames must be >= 0")
    return int(_lib.check(_lib.load().dsp_stretch_frames(int(n_frames), _rate(rate)), "dsp_stretch_frames"))


def stretch_length(n: int, rate: float) -> int:
    """max(1, rint(n / rate)): the samples of a clip of n samples stretched by rate."""
    if n < 0:
        raise ValueError("n must be >= 0")
    return int(_lib.check(_lib.load().dsp_stretch_length(int(n), _rate(rate)), "dsp_stretch_length"))


def pitch_ratio(n_steps: int, bins_per_octave: int = 12, max_term: int = 256):
    """-> (up, down): the fraction nearest to 2^(-n_steps / bins_per_octave) with max(up, down) <= max_term."""
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)):
        raise ValueError("n_steps must be an integer")
    if bins_per_octave < 1 or not 1 <= max_term <= 1024:
        raise ValueError("bins_per_octave must be >= 1 and max_term 1 .. 1024")
    up, down = C.c_int(), C.c_int()
    _lib.check(_lib.load().dsp_pitch_ratio(int(n_steps), int(bins_per_octave), int(max_term), C.byref(up), C.byref(down)), "dsp_pitch_ratio")
    return up.value, down.value


def augment_normal(seed: int, key: int, i) -> np.ndarray:
    """The float64 values of the library's normal draws (seed, key) at sample indices i."""
    L = _lib.load()
    idx = np.atleast_1d(np.asarray(i, dtype=np.uint64))
    return np.array([L.dsp_augment_normal(int(seed), int(key), int(j)) for j in idx], np.float64).reshape(np.shape(i))


def make_ops(ops) -> np.ndarray:
    """ops: a record array of lib.AUGMENT_OP_DTYPE, or a sequence of dicts / tuples (clip, kind, rate, n_steps, sigma, key) with kind
    "stretch" / "pitch" / "noise" or its number -> a contiguous record array (dsp_augment_op[m])."""
    dt = np.dtype(_lib.AUGMENT_OP_DTYPE)
    if isinstance(ops, np.ndarray) and ops.dtype == dt:
        return np.ascontiguousarray(ops)
    out = np.zeros(len(ops), dt)
    out["rate"] = 1.0
    for j, op in enumerate(ops):
        if not isinstance(op, dict):
            op = dict(zip(("clip", "kind", "rate", "n_steps", "sigma", "key"), op))
        if "clip" not in op or "kind" not in op:
            raise ValueError(f"op {j} needs a clip and a kind")
        kind = _KINDS.get(op["kind"], op["kind"])
        if kind not in (0, 1, 2):
            raise ValueError(f"op {j}: kind must be 'stretch', 'pitch' or 'noise'")
        out[j] = (int(op["clip"]), kind, float(op.get("rate", 1.0)), int(op.get("n_steps", 0)), float(op.get("sigma", 0.0)), int(op.get("key", op["clip"])))
    return out


def _ops_ptr(ops: np.ndarray):
    return ops.ctypes.data_as(C.POINTER(_lib.AugmentOp))


def augment_out_offsets(offsets, ops) -> np.ndarray:
    """-> int64 [m + 1]: where each op's output starts (dsp_augment_out_offsets)."""
    off, n = offsets if isinstance(offsets, tuple) else _lib.c_offsets(offsets)
    ops = make_ops(ops)
    oo = np.zeros(ops.size + 1, np.int64)
    _lib.check(_lib.load().dsp_augment_out_offsets(off, n, _ops_ptr(ops), ops.size, oo.ctypes.data_as(_lib.LP)), "dsp_augment_out_offsets")
    return oo


def augment_draw(labels, prob: float = 0.5, seed: int = 0) -> np.ndarray:
    """cepstrum/train.py's policy with the library's draws (dsp_augment_draw): rows with label 1 get an op with probability prob ->
    the ops as a record array of lib.AUGMENT_OP_DTYPE."""
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError("prob must be in [0, 1]")
    lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
    if lab.ndim != 1:
        raise ValueError("labels must be 1-D")
    L = _lib.load()
    lp = lab.ctypes.data_as(C.POINTER(C.c_int))
    m = _lib.check(L.dsp_augment_draw(int(seed), lp, lab.size, float(prob), None, 0), "dsp_augment_draw")
    ops = np.zeros(m, np.dtype(_lib.AUGMENT_OP_DTYPE))
    _lib.check(L.dsp_augment_draw(int(seed), lp, lab.size, float(prob), _ops_ptr(ops), m), "dsp_augment_draw")
    return ops


class Augmenter(_lib.Handle):
    """dsp_augmenter: the transform's tables, grow-only workspaces and one resampler per pitch ratio on one GPU.  pad: "reflect"
    (np.pad's, clips of at least 1025 samples) or "zero".  Every method takes a ragged batch -- signal: cuda float32 [total], clip c =
    samples [offsets[c], offsets[c + 1]) -- and is asynchronous on torch's current stream.  One call at a time per object."""

    _destroy = "dsp_augmenter_destroy"

    def __init__(self, device: int = 0, pad: str = "reflect", max_term: int = 256):
        if pad not in _PADS:
            raise ValueError('pad must be "reflect" or "zero"')
        if isinstance(max_term, bool) or not isinstance(max_term, (int, np.integer)) or not 1 <= max_term <= 1024:
            raise ValueError("max_term must be an integer 1 .. 1024")
        self.device, self.pad, self.max_term = int(device), pad, int(max_term)
        self._create("dsp_augmenter_create", self.device, _PADS[pad], self.max_term)

    def _signal(self, signal, offsets):
        import torch
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        if channels:
            raise ValueError("signal must be float32 (convert int16 first)")
        if signal.device.index != self.device:
            raise ValueError(f"signal must live on the augmenter's device (cuda:{self.device})")
        lens = np.diff(np.frombuffer(off, dtype=np.int64))
        if off[0] < 0 or (lens < 0).any():
            raise ValueError("offsets must be non-negative and non-decreasing")
        return off, n, lens, ptr

    def _clip_lengths(self, lens):
        need = 1025 if self.pad == "reflect" else 1
        if (lens < need).any() or (lens >= 1 << 24).any():
            raise ValueError(f"every clip must hold {need} .. 2^24 - 1 samples (pad={self.pad!r})")

    def stft(self, signal, offsets):
        """-> (spec cuda float32 [sum T][1025][2] (re, im), frame_offsets int64 [n + 1])."""
        import torch
        off, n, lens, ptr = self._signal(signal, offsets)
        self._clip_lengths(lens)
        fo = np.zeros(n + 1, np.int64)
        fo[1:] = np.cumsum(1 + lens // HOP)
        spec = torch.empty((int(fo[-1]), BINS, 2), dtype=torch.float32, device=signal.device)
        if n:
            got = np.zeros(n + 1, np.int64)
            _lib.check(self._L.dsp_stft_ragged_device(self._h, ptr, n, off, spec.data_ptr(), got.ctypes.data_as(_lib.LP), self._stream()), "dsp_stft_ragged_device")
            if not np.array_equal(got, fo):
                raise _lib.DspError("dsp_stft_ragged_device counted other frames than the wrapper")
        return spec, fo

    def istft(self, spec, frame_offsets, lengths):
        """spec: cuda float32 [rows][1025][2], clip c = rows [frame_offsets[c], frame_offsets[c + 1]) -> (signal cuda float32
        [sum lengths], offsets int64 [n + 1])."""
        import torch
        if not (isinstance(spec, torch.Tensor) and spec.is_cuda and spec.dtype == torch.float32 and spec.is_contiguous() and spec.dim() == 3 and
                spec.shape[1:] == (BINS, 2)):
            raise ValueError("spec must be a contiguous float32 CUDA tensor [rows][1025][2]")
        if spec.device.index != self.device:
            raise ValueError(f"spec must live on the augmenter's device (cuda:{self.device})")
        fo = np.ascontiguousarray(np.asarray(frame_offsets, dtype=np.int64))
        if fo.ndim != 1 or fo.size < 1 or fo[0] < 0 or (np.diff(fo) < 0).any() or int(fo[-1]) > spec.shape[0]:
            raise ValueError("frame_offsets must hold n + 1 non-decreasing rows of spec")
        n = fo.size - 1
        lengths = _lib.long_array(lengths, n, "lengths")
        if (lengths < 0).any() or (lengths >= 1 << 24).any():
            raise ValueError("lengths must be 0 .. 2^24 - 1")
        oo = np.zeros(n + 1, np.int64)
        oo[1:] = np.cumsum(lengths)
        out = torch.empty((int(oo[-1]),), dtype=torch.float32, device=spec.device)
        if n:
            _lib.check(self._L.dsp_istft_ragged_device(self._h, spec.data_ptr(), n, fo.ctypes.data_as(_lib.LP), lengths.ctypes.data_as(_lib.LP), out.data_ptr(),
                                                       oo.ctypes.data_as(_lib.LP), self._stream()), "dsp_istft_ragged_device")
        return out, oo

    def time_stretch(self, signal, offsets, rates):
        """rates: one rate, or one per clip -> (signal, offsets) with clip c stretched to max(1, rint(len / rate)) samples."""
        import torch
        off, n, lens, ptr = self._signal(signal, offsets)
        self._clip_lengths(lens)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(rates, dtype=np.float64), (n,)))
        if not (np.isfinite(r).all() and (r >= 0.125).all() and (r <= 8.0).all()):
            raise ValueError("rates must be finite and in [1/8, 8]")
        ops = np.zeros(n, np.dtype(_lib.AUGMENT_OP_DTYPE))           # the entry's output offsets are those of n stretch ops: one library call
        ops["clip"], ops["kind"], ops["rate"] = np.arange(n), _lib.AUGMENT_STRETCH, r
        oo = augment_out_offsets((off, n), ops)
        out = torch.empty((int(oo[-1]),), dtype=torch.float32, device=signal.device)
        if n:
            _lib.check(self._L.dsp_time_stretch_ragged_device(self._h, ptr, n, off, r.ctypes.data_as(C.POINTER(C.c_double)), out.data_ptr(), self._stream()),
                       "dsp_time_stretch_ragged_device")
        return out, oo

    def pitch_shift(self, signal, offsets, n_steps):
        """n_steps: semitones, one value or one per clip (integers, -12 .. 12) -> (signal, offsets), every clip at its own length."""
        n = (offsets[1] if isinstance(offsets, tuple) else len(offsets) - 1)
        steps = np.broadcast_to(np.asarray(n_steps), (n,))
        if steps.dtype.kind not in "iu" or (np.abs(steps) > 12).any():
            raise ValueError("n_steps must be integers -12 .. 12")
        ops = np.zeros(n, np.dtype(_lib.AUGMENT_OP_DTYPE))
        ops["clip"], ops["kind"], ops["rate"], ops["n_steps"], ops["key"] = np.arange(n), _lib.AUGMENT_PITCH, 1.0, steps, np.arange(n)
        return self.apply(signal, offsets, ops)

    def add_noise(self, signal, offsets, sigma: float = 0.005, seed: int = 0, keys=None):
        """y + sigma N(0, 1) from the library's draws; clip c draws on stream keys[c] (default c) -> (signal, offsets)."""
        n = (offsets[1] if isinstance(offsets, tuple) else len(offsets) - 1)
        if not (np.isfinite(sigma) and sigma >= 0):
            raise ValueError("sigma must be finite and >= 0")
        keys = np.arange(n) if keys is None else _lib.long_array(keys, n, "keys")
        ops = np.zeros(n, np.dtype(_lib.AUGMENT_OP_DTYPE))
        ops["clip"], ops["kind"], ops["rate"], ops["sigma"], ops["key"] = np.arange(n), _lib.AUGMENT_NOISE, 1.0, sigma, keys
        return self.apply(signal, offsets, ops, seed=seed)

    def draw(self, labels, prob: float = 0.5, seed: int = 0) -> np.ndarray:
        """The ops of cepstrum/train.py's policy for these labels (augment_draw)."""
        return augment_draw(labels, prob, seed)

    def apply(self, signal, offsets, ops, seed: int = 0):
        """ops as make_ops takes them: op j reads clip ops[j].clip -> (signal_out cuda float32, out_offsets int64 [m + 1]) with op j's
        output at [out_offsets[j], out_offsets[j + 1])."""
        import torch
        off, n, lens, ptr = self._signal(signal, offsets)
        ops = make_ops(ops)
        if ops.size and ((ops["clip"] < 0).any() or (ops["clip"] >= n).any()):
            raise ValueError(f"ops must name clips 0 .. {n - 1}")
        oo = augment_out_offsets((off, n), ops)
        out = torch.empty((int(oo[-1]),), dtype=torch.float32, device=signal.device)
        if ops.size:
            _lib.check(self._L.dsp_augment_ragged_device(self._h, ptr, n, off, _ops_ptr(ops), ops.size, int(seed), out.data_ptr(), self._stream()),
                       "dsp_augment_ragged_device")
        return out, oo
