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


def librosa_config(sample_rate: int = 22050, n_mfcc: int = 13, **over) -> MfccConfig:
    """dsp_mfcc_librosa_config() -- librosa.feature.mfcc(y, sr, n_mfcc) with librosa's defaults (n_fft 2048, hop 512, centred frames)
    of 2fa/audio/keyword_classifier.py:41-44 and cepstrum/train.py:38-40 -- with keyword overrides."""
    cfg = MfccConfig()
    _lib.load().dsp_mfcc_librosa_config(C.byref(cfg), int(sample_rate), int(n_mfcc))
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


def host_pipeline(device: int = 0, chunk_bytes: int | None = None, depth: int | None = None, pageable_mode: int | None = None,
                  classify_min_clips: int | None = None):
    """The host pipeline of `device` -- what every *_host entry streams its batch through: chunks of chunk_bytes input bytes in a ring of
    `depth` slots; pageable_mode (lib.PAGEABLE_*) says what is done with a pageable batch larger than a chunk, classify_min_clips is the
    fewest clips of a classifier's chunk (dsp_host_pipeline_set).  No argument given: the library's defaults are put back; otherwise the
    arguments left out keep their current value.  Returns (chunk_bytes, depth, pageable_mode, classify_min_clips) as they now stand.
    No setting changes a result bit."""
    L = _lib.load()
    cfg = _lib.HostPipelineConfig()
    given = (("chunk_bytes", chunk_bytes), ("depth", depth), ("pageable_mode", pageable_mode), ("classify_min_clips", classify_min_clips))
    if all(value is None for _, value in given):
        _lib.check(L.dsp_host_pipeline_set(int(device), None), "dsp_host_pipeline_set")
    else:
        _lib.check(L.dsp_host_pipeline_get(int(device), C.byref(cfg)), "dsp_host_pipeline_get")
        for name, value in given:
            if value is not None:
                setattr(cfg, name, int(value))
        _lib.check(L.dsp_host_pipeline_set(int(device), C.byref(cfg)), "dsp_host_pipeline_set")
    _lib.check(L.dsp_host_pipeline_get(int(device), C.byref(cfg)), "dsp_host_pipeline_get")
    return cfg.chunk_bytes, cfg.depth, cfg.pageable_mode, cfg.classify_min_clips


def host_pipeline_stats(device: int = 0) -> dict:
    """What the last host call on `device` did (dsp_host_pipeline_stats): n_chunks, depth, input_path / output_path ("staged", "pinned",
    "registered", or "direct": the caller's array handed to the runtime's copy as it is), bytes_h2d, bytes_d2h, peak_staging_bytes,
    pinned_ring_bytes."""
    st = _lib.HostStats()
    _lib.check(_lib.load().dsp_host_pipeline_stats(int(device), C.byref(st)), "dsp_host_pipeline_stats")
    out = {name: getattr(st, name) for name, _ in st._fields_}
    out["input_path"], out["output_path"] = _lib.HOST_PATHS[st.input_path], _lib.HOST_PATHS[st.output_path]
    return out


def host_pipeline_release(device: int = 0) -> None:
    """Returns the pipeline's pinned ring, device staging and streams (dsp_host_pipeline_release); the next host call makes them again."""
    _lib.check(_lib.load().dsp_host_pipeline_release(int(device)), "dsp_host_pipeline_release")


def plan_host_chunks(n_items: int, item_bytes: int, chunk_bytes: int, offsets=None) -> np.ndarray:
    """The pipeline's chunk planner (dsp_host_plan_chunks, host only): int64 first[n_chunks + 1], chunk k = items [first[k], first[k + 1]).
    offsets None: n_items uniform items of item_bytes; offsets [n_items + 1]: a ragged batch of samples of item_bytes bytes."""
    L = _lib.load()
    off = None if offsets is None else _lib.c_offsets(offsets)[0]
    first = np.empty(int(n_items) + 1 if n_items >= 0 else 1, np.int64)
    n = _lib.check(L.dsp_host_plan_chunks(int(n_items), int(item_bytes), off, int(chunk_bytes), first.ctypes.data_as(_lib.LP), first.size),
                   "dsp_host_plan_chunks")
    return first[:n + 1].copy()


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

    # ---- host buffers: numpy arrays or CPU torch tensors (pinned ones are read by the copy engines directly) ----------------
    def frames_host(self, frames) -> np.ndarray:
        frames = _lib.host_array(frames, np.float32)
        if frames.ndim != 2 or frames.shape[1] != self.cfg.frame_length:
            raise ValueError(f"frames must be [n][{self.cfg.frame_length}]")
        out = np.empty((frames.shape[0], self.cfg.n_mfcc), np.float32)
        _lib.check(self._L.dsp_mfcc_frames_host(self._h, frames.ctypes.data, frames.shape[0], out.ctypes.data), "dsp_mfcc_frames_host")
        return out

    def clips_host(self, clips, max_frames: int) -> np.ndarray:
        clips = _lib.host_array(clips, np.float32)
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

    def clips_pcm16_host(self, pcm, max_frames: int, stereo_mode: int = 0) -> np.ndarray:
        """pcm: host int16 [n_clips][samples] (mono) or [n_clips][samples][2] (interleaved stereo; stereo_mode 0 = channel 0, 1 = channel
        average) -> float32 [n_clips][T][n_mfcc], every row what clips_pcm16 gives (dsp_mfcc_clips_pcm16_host)."""
        pcm = _lib.host_array(pcm, np.int16)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        if pcm.ndim not in (2, 3) or (pcm.ndim == 3 and pcm.shape[2] != 2):
            raise ValueError("pcm must be int16 [n_clips][n] or [n_clips][n][2]")
        n, s = pcm.shape[:2]
        t = frames_for(self.cfg, s, max_frames)
        out = np.empty((n, t, self.cfg.n_mfcc), np.float32)
        got = _lib.check(self._L.dsp_mfcc_clips_pcm16_host(self._h, pcm.ctypes.data, n, s, s, pcm.ndim - 1, int(stereo_mode), out.ctypes.data,
                                                            int(max_frames)), "dsp_mfcc_clips_pcm16_host")
        assert got == t or n == 0
        return out

    def clips_ragged_host(self, signal, offsets, max_frames: int, stereo_mode: int = 0):
        """A ragged batch in host memory -- signal: float32 [total], int16 [total] (mono) or int16 [total][2] (interleaved stereo), clip c =
        samples [offsets[c], offsets[c + 1]) per channel -- streamed through the GPU in chunks of whole clips.  Returns (mfcc,
        frame_offsets) as clips_ragged does, the matrix a numpy float32 [F][n_mfcc] (dsp_mfcc_clips_ragged_host / _pcm16_host)."""
        pcm = getattr(signal, "dtype", None) in (np.dtype(np.int16), _lib.torch_int16())
        signal = _lib.host_array(signal, np.int16 if pcm else np.float32)
        if signal.ndim != 1 and not (pcm and signal.ndim == 2 and signal.shape[1] == 2):
            raise ValueError("signal must be float32 [total], int16 [total] or interleaved int16 [total][2]")
        off, n = offsets if isinstance(offsets, tuple) else _lib.c_offsets(offsets)
        if n and int(off[n]) > signal.shape[0]:
            raise ValueError("offsets run past the end of the signal")
        fo = ragged_frame_offsets(self.cfg, (off, n), max_frames)
        out = np.empty((int(fo[-1]), self.cfg.n_mfcc), np.float32)
        if pcm:
            _lib.check(self._L.dsp_mfcc_clips_ragged_pcm16_host(self._h, signal.ctypes.data, n, off, signal.ndim, int(stereo_mode), int(max_frames),
                                                                out.ctypes.data), "dsp_mfcc_clips_ragged_pcm16_host")
        else:
            _lib.check(self._L.dsp_mfcc_clips_ragged_host(self._h, signal.ctypes.data, n, off, int(max_frames), out.ctypes.data),
                       "dsp_mfcc_clips_ragged_host")
        return out, fo

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
