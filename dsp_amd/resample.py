"""Recordings at another rate: the polyphase FIR resampler of include/dsp_amd.h (dsp_resample_*) --
scipy.signal.resample_poly's defaults as one HIP launch over a ragged or uniform batch, float or int16 in HBM -- and the same
outputs from feeds that are still arriving (dsp_stream_resample*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib


def _rates(rate_in, rate_out):
    if isinstance(rate_in, bool) or isinstance(rate_out, bool) or not isinstance(rate_in, (int, np.integer)) or not isinstance(rate_out, (int, np.integer)):
        raise ValueError("rate_in and rate_out must be integers")
    if rate_in < 1 or rate_out < 1 or rate_in > 2**31 - 1 or rate_out > 2**31 - 1:
        raise ValueError("rate_in and rate_out must be >= 1 (and fit an int)")
    return int(rate_in), int(rate_out)


def resample_ratio(rate_in: int, rate_out: int):
    """-> (up, down, half): the reduced ratio and the filter's half length (2 half + 1 taps).  DspError: up or down above 1024."""
    rate_in, rate_out = _rates(rate_in, rate_out)
    up, down, half = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().dsp_resample_ratio(rate_in, rate_out, C.byref(up), C.byref(down), C.byref(half)), "dsp_resample_ratio")
    return up.value, down.value, half.value


GEOMETRY_FIELDS = ("up", "down", "half", "taps", "row", "tile", "items", "span", "staged", "lds_bytes")


def resample_geometry(rate_in: int, rate_out: int) -> dict:
    """Host only (dsp_resample_geometry): the block geometry the kernels run this ratio with -- taps per polyphase branch, outputs and
    lane work items per block, the input span a block reads, whether it is staged in LDS (0: read from global memory; no live streams)."""
    rate_in, rate_out = _rates(rate_in, rate_out)
    L = _lib.load()
    n = _lib.check(L.dsp_resample_geometry(rate_in, rate_out, None, 0), "dsp_resample_geometry")
    if n != len(GEOMETRY_FIELDS):
        raise _lib.DspError(f"the library reports {n} geometry fields, the wrapper knows {len(GEOMETRY_FIELDS)}")
    v = (C.c_int * n)()
    _lib.check(L.dsp_resample_geometry(rate_in, rate_out, v, n), "dsp_resample_geometry")
    return dict(zip(GEOMETRY_FIELDS, (int(x) for x in v)))


def resample_taps(rate_in: int, rate_out: int) -> np.ndarray:
    """The float64 taps h[2 half + 1] (= scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up)."""
    rate_in, rate_out = _rates(rate_in, rate_out)
    L = _lib.load()
    n = _lib.check(L.dsp_resample_taps(rate_in, rate_out, None, 0), "dsp_resample_taps")
    h = np.empty(n, np.float64)
    _lib.check(L.dsp_resample_taps(rate_in, rate_out, h.ctypes.data_as(C.POINTER(C.c_double)), n), "dsp_resample_taps")
    return h


def resample_offsets(rate_in: int, rate_out: int, offsets) -> np.ndarray:
    """offsets[n + 1] of a ragged batch at rate_in -> int64 [n + 1]: where each resampled recording starts (prefix sums of
    ceil(len up / down) from 0).  `offsets` as lib.c_offsets takes them, or the pair it returned."""
    rate_in, rate_out = _rates(rate_in, rate_out)
    off, n = offsets if isinstance(offsets, tuple) else _lib.c_offsets(offsets)
    out = (C.c_long * (n + 1))()
    _lib.check(_lib.load().dsp_resample_offsets(rate_in, rate_out, off, n, out), "dsp_resample_offsets")
    return np.frombuffer(out, dtype=np.int64).copy()


class Resampler(_lib.Handle):
    """dsp_resampler: the taps of rate_in -> rate_out on one GPU."""

    _destroy = "dsp_resampler_destroy"

    def __init__(self, rate_in: int, rate_out: int, device: int = 0):
        self.rate_in, self.rate_out = _rates(rate_in, rate_out)
        self.up, self.down, self.half = resample_ratio(rate_in, rate_out)
        self.device = int(device)
        self._create("dsp_resampler_create", self.device, self.rate_in, self.rate_out)

    def out_samples(self, n: int) -> int:
        """ceil(n up / down): the output length of a recording of n samples."""
        if n < 0:
            raise ValueError("n must be >= 0")
        return -((-int(n) * self.up) // self.down)

    def ragged(self, signal, offsets, stereo_mode: int = 0, out=None):
        """signal: cuda float32 [total], int16 [total] (mono) or int16 [total][2] (interleaved stereo; stereo_mode 0 = channel 0,
        1 = channel average), recording c = samples [offsets[c], offsets[c + 1]) per channel.  Returns (out, out_offsets): cuda float32
        [out_offsets[-1]] with recording c at [out_offsets[c], out_offsets[c + 1]) (numpy int64) -- what every *_ragged entry, Scanner and
        StreamSession-free per-clip call takes as (signal, offsets).  Async on torch's current stream."""
        import torch
        if stereo_mode not in (0, 1):
            raise ValueError("stereo_mode must be 0 (channel 0) or 1 (channel average)")
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        oo = resample_offsets(self.rate_in, self.rate_out, (off, n))
        total = int(oo[-1])
        if out is None:
            out = torch.empty((total,), dtype=torch.float32, device=signal.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= total):
            raise ValueError(f"out must be a contiguous float32 CUDA tensor of at least {total} samples")
        if total and channels:
            _lib.check(self._L.dsp_resample_ragged_pcm16_device(self._h, ptr, n, off, channels, int(stereo_mode), out.data_ptr(), self._stream()),
                       "dsp_resample_ragged_pcm16_device")
        elif total:
            _lib.check(self._L.dsp_resample_ragged_device(self._h, ptr, n, off, out.data_ptr(), self._stream()), "dsp_resample_ragged_device")
        return out, oo

    def clips(self, clips, stereo_mode: int = 0, out=None):
        """clips: cuda float32 [n][samples], int16 [n][samples] or interleaved int16 [n][samples][2] -> cuda float32 [n][n_out],
        row c bit for bit what ragged() gives for that clip."""
        import torch
        if stereo_mode not in (0, 1):
            raise ValueError("stereo_mode must be 0 (channel 0) or 1 (channel average)")
        if not (isinstance(clips, torch.Tensor) and clips.is_cuda and clips.dtype in (torch.float32, torch.int16)):
            raise ValueError("clips must be a float32 or int16 CUDA tensor")
        if clips.dim() >= 2 and clips.numel() == 0:             # no clips, or clips without samples: the strides of an empty tensor say nothing
            if not (clips.dim() == 2 or (clips.dim() == 3 and clips.dtype == torch.int16 and clips.shape[2] == 2)):
                raise ValueError("clips must be [n][samples], or interleaved int16 [n][samples][2]")
            channels, stride = 0, int(clips.shape[1])
        elif clips.dtype == torch.int16:
            channels, stride = _lib.pcm_device(clips)
        else:
            channels, stride = 0, _lib.clips_device(clips, torch.float32).stride(0)
        n, s = int(clips.shape[0]), int(clips.shape[1])
        n_out = self.out_samples(s)
        if out is None:
            out = torch.empty((n, n_out), dtype=torch.float32, device=clips.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape == (n, n_out) and (out.numel() == 0 or out.stride(1) == 1)):
            raise ValueError(f"out must be a float32 CUDA tensor [{n}][{n_out}] with unit inner stride")
        if n and n_out:
            if channels:
                got = _lib.check(self._L.dsp_resample_clips_pcm16_device(self._h, clips.data_ptr(), n, s, stride, channels, int(stereo_mode), out.data_ptr(),
                                                                         out.stride(0), self._stream()), "dsp_resample_clips_pcm16_device")
            else:
                got = _lib.check(self._L.dsp_resample_clips_device(self._h, clips.data_ptr(), n, s, stride, out.data_ptr(), out.stride(0), self._stream()),
                                 "dsp_resample_clips_device")
            if got != n_out:
                raise _lib.DspError(f"the library resampled {s} samples to {got}, the wrapper expected {n_out}")
        return out


def stream_resample_plan(rate_in: int, rate_out: int, received, chunk_offsets) -> np.ndarray:
    """Host only (dsp_stream_resample_plan): streams that have received `received[s]` sample frames (None: none) and now get chunks
    [chunk_offsets[s], chunk_offsets[s + 1]) -> int64 [n + 1], the prefix sums of the outputs that become complete."""
    rate_in, rate_out = _rates(rate_in, rate_out)
    co = np.ascontiguousarray(np.asarray(chunk_offsets, dtype=np.int64))
    if co.ndim != 1 or co.size < 1:
        raise ValueError("chunk_offsets must hold n_streams + 1 positions")
    n = co.size - 1
    if co[0] < 0 or (np.diff(co) < 0).any():
        raise ValueError("chunk_offsets must be non-negative and non-decreasing")
    rec = None
    if received is not None:
        rec = _lib.long_array(received, n, "received")
        if (rec < 0).any():
            raise ValueError("received must be non-negative")
    oo = np.zeros(n + 1, np.int64)
    _lib.check(_lib.load().dsp_stream_resample_plan(rate_in, rate_out, rec.ctypes.data_as(_lib.LP) if rec is not None else None, co.ctypes.data_as(_lib.LP), n,
                                                    oo.ctypes.data_as(_lib.LP)), "dsp_stream_resample_plan")
    return oo


class StreamResampler(_lib.Handle):
    """dsp_stream_resampler: n_streams live feeds at rate_in on one GPU.  Every push hands over the next chunk of each feed (any length)
    and returns the outputs at rate_out that became complete with it; concatenated over the pushes they are, bit for bit, the first
    outputs of Resampler.ragged on the whole feed, and finish() emits the rest.  dtype: torch.float32 samples, or torch.int16 PCM
    ([total] mono, [total][2] interleaved stereo with stereo_mode 0 = channel 0 / 1 = average; channels=2 selects stereo).  One stream
    at a time per object."""

    _destroy = "dsp_stream_resampler_destroy"

    def __init__(self, rate_in: int, rate_out: int, n_streams: int, dtype=None, stereo_mode: int = 0, channels: int = 1, device: int = 0):
        self.rate_in, self.rate_out = _rates(rate_in, rate_out)
        self.dtype, self.channels, self.stereo_mode, self.n_streams, pcm16 = _lib.stream_format(dtype, channels, stereo_mode, n_streams)
        self.up, self.down, self.half = resample_ratio(rate_in, rate_out)
        self.device = int(device)
        self._create("dsp_stream_resampler_create", self.device, self.rate_in, self.rate_out, self.n_streams, self.channels, self.stereo_mode, pcm16)

    def counts(self):
        """-> (sample frames received, outputs emitted), int64 [n_streams] each."""
        out = [np.zeros(self.n_streams, np.int64) for _ in range(2)]
        _lib.check(self._L.dsp_stream_resampler_counts(self._h, *[a.ctypes.data_as(_lib.LP) for a in out]), "dsp_stream_resampler_counts")
        return tuple(out)

    def plan(self, chunk_offsets) -> np.ndarray:
        """What a push of these chunks would emit now: int64 [n_streams + 1], the prefix sums of the new outputs."""
        co = _lib.long_array(chunk_offsets, self.n_streams + 1, "chunk_offsets")
        return stream_resample_plan(self.rate_in, self.rate_out, self.counts()[0], co)

    def _named(self, streams):
        idx = np.ascontiguousarray(np.asarray(streams, dtype=np.int64))
        if idx.ndim != 1 or (idx.size and (idx.min() < 0 or idx.max() >= self.n_streams)):
            raise ValueError(f"streams must name streams 0 .. {self.n_streams - 1}")
        return idx

    def reset(self, streams=None):
        """Forget the named streams' samples and counters (None: all of them, which also revives a broken object)."""
        if streams is None:
            _lib.check(self._L.dsp_stream_resampler_reset(self._h, None, 0, None), "dsp_stream_resampler_reset")
            return
        idx = self._named(streams)
        _lib.check(self._L.dsp_stream_resampler_reset(self._h, idx.ctypes.data_as(_lib.LP), idx.size, None), "dsp_stream_resampler_reset")

    def _out(self, out, total, dev):
        import torch
        if out is None:
            return torch.empty((total,), dtype=torch.float32, device=dev)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 1 and out.numel() >= total):
            raise ValueError(f"out must be a contiguous float32 CUDA tensor of at least {total} samples")
        return out

    def push(self, chunks, chunk_offsets, out=None):
        """chunks: a contiguous CUDA tensor of the object's dtype on its device ([total], or [total][2] for stereo), stream s's chunk =
        sample frames [chunk_offsets[s], chunk_offsets[s + 1]) -> (out float32 [new outputs], out_offsets int64 [n + 1]): stream s's new
        outputs are out[out_offsets[s] : out_offsets[s + 1]].  Async on torch's current stream."""
        co = _lib.stream_chunks(chunks, chunk_offsets, self.n_streams, self.dtype, self.channels, self.device)
        oo = stream_resample_plan(self.rate_in, self.rate_out, self.counts()[0], co)
        out = self._out(out, int(oo[-1]), chunks.device)
        oo2 = np.zeros_like(oo)
        _lib.check(self._L.dsp_stream_resample_push_device(self._h, chunks.data_ptr(), co.ctypes.data_as(_lib.LP), out.data_ptr(), oo2.ctypes.data_as(_lib.LP),
                                                           self._stream()), "dsp_stream_resample_push_device")
        if not np.array_equal(oo, oo2):
            raise _lib.DspError("dsp_stream_resample_push_device emitted other outputs than dsp_stream_resample_plan announced")
        return out[:int(oo2[-1])], oo2

    def finish(self, streams=None, out=None):
        """End the named streams (None: all): -> (out float32, out_offsets int64 [len(streams) + 1]) with the outputs a whole recording
        has beyond those the pushes emitted, in the order named; the streams start afresh."""
        import torch
        idx = self._named(np.arange(self.n_streams) if streams is None else streams)
        if np.unique(idx).size != idx.size:
            raise ValueError("a stream may be named once")
        n_in, n_out = self.counts()
        total = int(sum(-((-int(n_in[s]) * self.up) // self.down) - int(n_out[s]) for s in idx))
        out = self._out(out, total, torch.device("cuda", self.device))
        oo = np.zeros(idx.size + 1, np.int64)
        _lib.check(self._L.dsp_stream_resample_finish_device(self._h, idx.ctypes.data_as(_lib.LP), idx.size, out.data_ptr(), oo.ctypes.data_as(_lib.LP),
                                                             self._stream()), "dsp_stream_resample_finish_device")
        if int(oo[-1]) != total:
            raise _lib.DspError(f"the library finished with {int(oo[-1])} outputs, the wrapper expected {total}")
        return out[:total], oo
