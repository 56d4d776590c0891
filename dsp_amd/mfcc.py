"""Host-side mirror of the reference's MFCC interface over the C ABI.

Reference: 2fa/audio/word/c/mfcc.h:16-19 (`compute_mfcc`) and its first caller
2fa/audio/word/c/stop_detector.c:12-21.  Same names, argument meaning and
return conventions; numpy arrays stand in for the caller-owned C buffers and
torch tensors for HBM-resident buffers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from .lib import DspError, MfccConfig


def default_config(**over) -> MfccConfig:
    """dsp_mfcc_default_config() with keyword overrides."""
    cfg = MfccConfig()
    _lib.load().dsp_mfcc_default_config(C.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"dsp_mfcc_config has no field {k!r}")
        setattr(cfg, k, v)
    return cfg


def speaker_config(**over) -> MfccConfig:
    """dsp_mfcc_speaker_config() -- librosa.feature.mfcc(sr 16000, n_mfcc 13, n_fft 400, hop_length 160) of
    2fa/audio/speaker/gmm_utils.py:52-58 -- with keyword overrides."""
    cfg = MfccConfig()
    _lib.load().dsp_mfcc_speaker_config(C.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"dsp_mfcc_config has no field {k!r}")
        setattr(cfg, k, v)
    return cfg


def frames_for(cfg: MfccConfig, num_samples: int, max_frames: int) -> int:
    return _lib.load().dsp_mfcc_frames_for(C.byref(cfg), int(num_samples), int(max_frames))


def ragged_frame_offsets(cfg: MfccConfig, offsets, max_frames: int) -> np.ndarray:
    """Host only: int64 [n_clips + 1] prefix sums of frames_for(cfg, offsets[c + 1] - offsets[c], max_frames) -- the first row of each
    clip in the matrix clips_ragged returns (dsp_mfcc_ragged_frame_offsets)."""
    off, n = offsets if isinstance(offsets, tuple) else _lib.c_offsets(offsets)
    fo = np.empty(n + 1, np.int64)
    _lib.check(_lib.load().dsp_mfcc_ragged_frame_offsets(C.byref(cfg), off, n, int(max_frames), fo.ctypes.data_as(_lib.LP)),
               "dsp_mfcc_ragged_frame_offsets")
    return fo


def compute_mfcc(signal: np.ndarray, max_frames: int) -> np.ndarray:
    """The reference entry point itself: `int compute_mfcc(signal, n, out, max_frames)`
    called through the C ABI with host buffers.  Returns out[:T] (frame-major [T][13])."""
    signal = np.ascontiguousarray(signal, np.float32)
    out = np.zeros((max(int(max_frames), 1), 13), np.float32)
    t = _lib.load().compute_mfcc(signal.ctypes.data, signal.size, out.ctypes.data, int(max_frames))
    return out[:t]


def tables(cfg: MfccConfig):
    """Reference-layout constant tables (window, mel, dct) for `cfg` (host only)."""
    L = _lib.load()
    win = np.empty(cfg.frame_length, np.float32)
    mel = np.empty((cfg.n_mels, cfg.n_fft // 2 + 1), np.float32)
    dct = np.empty((cfg.n_mfcc, cfg.n_mels), np.float32)
    _lib.check(L.dsp_mfcc_tables(C.byref(cfg), win.ctypes.data, mel.ctypes.data, dct.ctypes.data), "dsp_mfcc_tables")
    return win, mel, dct


class MfccPlan(_lib.Handle):
    """dsp_mfcc_plan: device tables for one configuration on one GPU."""

    _destroy = "dsp_mfcc_plan_destroy"

    def __init__(self, cfg: MfccConfig | None = None, device: int = 0):
        self.cfg = cfg or default_config()
        self.device = device
        self._create("dsp_mfcc_plan_create", C.byref(self.cfg), device)

    def set_kernel(self, kernel: int):
        """0 = one wavefront per frame (default), 1 = the general Stockham kernel (1024-point plans only), 2 = wave per frame with the
        per-frame epilogue.  3, and 1 on other plans, named 512-point kernels that were removed: DspError."""
        _lib.check(self._L.dsp_mfcc_plan_set_kernel(self._h, int(kernel)), "dsp_mfcc_plan_set_kernel")

    def set_launch(self, blocks_per_cu: int = 0, frames_per_chunk: int = 0):
        _lib.check(self._L.dsp_mfcc_plan_set_launch(self._h, blocks_per_cu, frames_per_chunk), "dsp_mfcc_plan_set_launch")

    # ---- host buffers -----------------------------------------------------
    def frames_host(self, frames: np.ndarray) -> np.ndarray:
        frames = np.ascontiguousarray(frames, np.float32)
        if frames.ndim != 2 or frames.shape[1] != self.cfg.frame_length:
            raise ValueError(f"frames must be [n][{self.cfg.frame_length}]")
        out = np.empty((frames.shape[0], self.cfg.n_mfcc), np.float32)
        _lib.check(self._L.dsp_mfcc_frames_host(self._h, frames.ctypes.data, frames.shape[0], out.ctypes.data), "dsp_mfcc_frames_host")
        return out

    def clips_host(self, clips: np.ndarray, max_frames: int) -> np.ndarray:
        clips = np.ascontiguousarray(clips, np.float32)
        if clips.ndim == 1:
            clips = clips[None, :]
        n, s = clips.shape
        t = frames_for(self.cfg, s, max_frames)
        out = np.empty((n, t, self.cfg.n_mfcc), np.float32)
        if n == 0 or t == 0:
            return out
        got = _lib.check(self._L.dsp_mfcc_clips_host(self._h, clips.ctypes.data, n, s, s, out.ctypes.data, int(max_frames)), "dsp_mfcc_clips_host")
        assert got == t
        return out

    # ---- HBM-resident buffers (torch tensors on this plan's device) -----------
    def frames(self, frames, out=None):
        """frames: cuda float32 [n][frame_length] -> cuda float32 [n][n_mfcc]; async on torch's current stream."""
        import torch
        if not (frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous()):
            raise ValueError("frames must be a contiguous float32 CUDA tensor")
        if frames.dim() != 2 or frames.shape[1] != self.cfg.frame_length:
            raise ValueError(f"frames must be [n][{self.cfg.frame_length}]")
        n = frames.shape[0]
        if out is None:
            out = torch.empty((n, self.cfg.n_mfcc), dtype=torch.float32, device=frames.device)
        _lib.check(self._L.dsp_mfcc_frames_device(self._h, frames.data_ptr(), n, out.data_ptr(), self._stream()), "dsp_mfcc_frames_device")
        return out

    def clips_pcm16(self, pcm, max_frames: int, stereo_mode: int = 0, out=None):
        """pcm: cuda int16 [n_clips][samples] (mono) or [n_clips][samples][2] (interleaved stereo;
        stereo_mode 0 = channel 0, 1 = channel average) -> cuda float32 [n_clips][T][n_mfcc]."""
        import torch
        channels, stride = _lib.pcm_device(pcm)
        n, s = int(pcm.shape[0]), int(pcm.shape[1])
        t = frames_for(self.cfg, s, max_frames)
        if out is None:
            out = torch.empty((n, t, self.cfg.n_mfcc), dtype=torch.float32, device=pcm.device)
        if n and t:
            got = _lib.check(self._L.dsp_mfcc_clips_pcm16_device(self._h, pcm.data_ptr(), n, s, stride, channels, int(stereo_mode),
                                                                  out.data_ptr(), int(max_frames), self._stream()), "dsp_mfcc_clips_pcm16_device")
            assert got == t
        return out

    def clips(self, clips, max_frames: int, out=None):
        """clips: cuda float32 [n_clips][samples] -> cuda float32 [n_clips][T][n_mfcc]."""
        import torch
        n, s = _lib.clips_device(clips, torch.float32).shape
        t = frames_for(self.cfg, s, max_frames)
        if out is None:
            out = torch.empty((n, t, self.cfg.n_mfcc), dtype=torch.float32, device=clips.device)
        if n and t:
            got = _lib.check(self._L.dsp_mfcc_clips_device(self._h, clips.data_ptr(), n, s, clips.stride(0), out.data_ptr(),
                                                            int(max_frames), self._stream()), "dsp_mfcc_clips_device")
            assert got == t
        return out

    def clips_ragged(self, signal, offsets, max_frames: int, stereo_mode: int = 0, out=None):
        """A ragged batch -- signal: cuda float32 [total], int16 [total] (mono) or int16 [total][2] (interleaved stereo; stereo_mode as
        clips_pcm16), clip c = samples [offsets[c], offsets[c + 1]) per channel -- in one launch.  Returns (mfcc, frame_offsets):
        cuda float32 [F][n_mfcc] with clip c's frames in rows [frame_offsets[c], frame_offsets[c + 1]) (numpy int64 [n_clips + 1]),
        each row bit for bit what a one-clip clips / clips_pcm16 call gives; clips shorter than a frame have no rows."""
        import torch
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        fo = ragged_frame_offsets(self.cfg, (off, n), max_frames)
        total = int(fo[-1])
        if out is None:
            out = torch.empty((total, self.cfg.n_mfcc), dtype=torch.float32, device=signal.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= total * self.cfg.n_mfcc):
            raise ValueError(f"out must be a contiguous float32 CUDA tensor of at least [{total}][{self.cfg.n_mfcc}]")
        if total and channels:
            _lib.check(self._L.dsp_mfcc_clips_ragged_pcm16_device(self._h, ptr, n, off, channels, int(stereo_mode), int(max_frames), out.data_ptr(),
                                                                  self._stream()), "dsp_mfcc_clips_ragged_pcm16_device")
        elif total:
            _lib.check(self._L.dsp_mfcc_clips_ragged_device(self._h, ptr, n, off, int(max_frames), out.data_ptr(), self._stream()),
                       "dsp_mfcc_clips_ragged_device")
        return out, fo
