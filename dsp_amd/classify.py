"""Host-side mirror of the donut classifier interface (sync/lib/classifier.h:14-19,
donut-classifier/classifier.c:319-592) over the C ABI: same function names and
argument meaning; numpy arrays stand in for the caller-owned / malloc'd C buffers.
All arithmetic runs in the HIP kernels of dsp_amd/csrc/classify_kernels.hip.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib


def butter_bandpass(lowcut: float, highcut: float):
    """-> (ok, b[9], a[9]) float64; ok False for any band but (1000,3000) / (3000,7500)
    (classifier.c:402-407)."""
    b = (C.c_double * 9)()
    a = (C.c_double * 9)()
    ok = _lib.load().dsp_butter_bandpass(float(lowcut), float(highcut), b, a)
    return bool(ok), np.array(b[:], np.float64), np.array(a[:], np.float64)


def butter_bandpass_filter(data: np.ndarray, b, a) -> np.ndarray:
    """Direct form II from zero state along the last axis; float32 input runs the fp32
    firmware arithmetic (classifier.cpp:193-219), float64 the fp64 one (classifier.c:420-446)."""
    data = np.asarray(data)
    dt = np.float64 if data.dtype == np.float64 else np.float32
    x = np.ascontiguousarray(np.atleast_2d(data), dt)
    y = np.empty_like(x)
    bb = np.ascontiguousarray(b, dt)
    aa = np.ascontiguousarray(a, dt)
    fn = _lib.load().dsp_butter_bandpass_filter_f64 if dt == np.float64 else _lib.load().dsp_butter_bandpass_filter_f32
    _lib.check(fn(x.ctypes.data, x.shape[0], x.shape[1], x.shape[1], bb.ctypes.data, aa.ctypes.data, y.ctypes.data),
               "dsp_butter_bandpass_filter")
    return y.reshape(data.shape)


def compute_spectrogram(signal: np.ndarray, fs: int = 16000):
    """-> (frequencies[129], times[T], Sxx[129][T]).  float32 input: the fp32 firmware arithmetic, bit-identical to
    classifier.cpp:221-368; float64 input: the float64 pipeline of donut-classifier/classifier.c:448-592."""
    signal = np.asarray(signal)
    dt = np.float64 if signal.dtype == np.float64 else np.float32
    signal = np.ascontiguousarray(signal, dt)
    t_max = max(1, (signal.size - 256) // 224 + 1) if signal.size >= 256 else 1
    freqs = np.empty(129, dt)
    times = np.empty(t_max, dt)
    sxx = np.empty((129, t_max), dt)
    fn = _lib.load().dsp_compute_spectrogram_f64 if dt == np.float64 else _lib.load().dsp_compute_spectrogram_f32
    t = _lib.check(fn(signal.ctypes.data, signal.size, int(fs), freqs.ctypes.data, times.ctypes.data, sxx.ctypes.data),
                   "dsp_compute_spectrogram")
    return freqs, times[:t], sxx.reshape(-1)[: 129 * t].reshape(129, t)


def classify(data: np.ndarray) -> int:
    """`int classify(float *data, int data_size)` (sync/lib/classifier.h:19) through the C ABI."""
    data = np.ascontiguousarray(data, np.float32)
    return int(_lib.load().dsp_classify(data.ctypes.data, data.size))


# thresholds of the reference's variants: (keep_lo, keep_hi, midpoint_db, middle_max, above_min, below_min)
CLASSIFY_SYNC_LIB = (0.65, 0.80, 70.0, 100.0, 200.0, 80.0)        # sync/lib/classifier.cpp:67-68, :436, :109 (default)
CLASSIFY_MICROPHONE = (0.70, 0.85, 45.0, 100.0, 200.0, 150.0)     # microphone/src/classifier.cpp:79-80, :448, :123
CLASSIFY_MICROPHONE_C = (0.70, 0.85, 45.0, 50.0, 200.0, 200.0)    # microphone/src/classifier.c:120-121, :608, :164 (thresholds of the float64 file)
CLASSIFY_DONUT_C = (0.70, 0.85, 45.0, 75.0, 300.0, 100.0)         # donut-classifier/classifier.c:141-142, :660, :184 (thresholds of the float64 file)


def classify_config(values=None) -> "_lib.ClassifyConfig":
    """dsp_classify_config: the library's defaults (sync/lib thresholds) or a 6-tuple like CLASSIFY_MICROPHONE."""
    c = _lib.ClassifyConfig()
    _lib.load().dsp_classify_default_config(C.byref(c))
    if values is not None:
        c.keep_lo, c.keep_hi, c.midpoint_db, c.middle_max, c.above_min, c.below_min = (float(v) for v in values)
    return c


STEREO_CHANNEL0, STEREO_AVERAGE = 0, 1       # dsp_amd.h: how interleaved stereo PCM becomes mono


# ---- the calls both precisions share: f64 picks the float64 entry point (name + "_f64"), its config and trace types ----------------

def _config(config, f64: bool):
    """None (the library's defaults), a 6-tuple or a config struct -> the config argument of an entry point."""
    if config is None:
        return None
    if f64:
        cfg = config if isinstance(config, _lib.ClassifyConfigF64) else _lib.ClassifyConfigF64(*[float(v) for v in config])
    else:
        cfg = config if isinstance(config, _lib.ClassifyConfig) else classify_config(config)
    return C.byref(cfg)


def _traces(tr, n_clips: int, dtype):
    """trace records -> [(midpoints[k], band sums[k][3])] per clip."""
    return [(np.array(t.midpoints[:t.n_midpoints], dtype), np.array([t.sums[i][:] for i in range(t.n_midpoints)], dtype).reshape(-1, 3))
            for t in tr[:n_clips]]


def _host(name: str, f64: bool, signal: np.ndarray, n_clips: int, with_trace: bool, config, *args):
    """One host entry point: (config, signal, n_clips, *args, labels, trace) -> labels (+ traces)."""
    name += "_f64" if f64 else ""
    labels = np.zeros(n_clips, np.int32)
    tr = ((_lib.ClassifyTraceF64 if f64 else _lib.ClassifyTrace) * max(n_clips, 1))() if with_trace else None
    _lib.check(getattr(_lib.load(), name)(_config(config, f64), signal.ctypes.data, n_clips, *args, labels.ctypes.data,
                                          C.byref(tr) if with_trace else None), name)
    return (labels, _traces(tr, n_clips, np.float64 if f64 else np.float32)) if with_trace else labels


def _device(name: str, f64: bool, signal, n_clips: int, labels, config, *args):
    """One device entry point: (config, signal, n_clips, *args, labels, [trace,] stream) on torch's current stream -> cuda int32 labels."""
    import torch
    name += "_f64" if f64 else ""
    if labels is None:
        labels = torch.empty(n_clips, dtype=torch.int32, device=signal.device)
    trace = (None,) if f64 else ()
    _lib.check(getattr(_lib.load(), name)(_config(config, f64), signal.data_ptr(), n_clips, *args, labels.data_ptr(), *trace, _lib.current_stream(signal)), name)
    return labels


def _pcm_host(pcm):
    """int16 [n], [n_clips][n] or [n_clips][n][2] -> (contiguous [n_clips][n](...), channels)."""
    pcm = np.ascontiguousarray(pcm, np.int16)
    if pcm.ndim == 1:
        pcm = pcm[None, :]
    if pcm.ndim not in (2, 3) or (pcm.ndim == 3 and pcm.shape[2] != 2):
        raise ValueError("pcm must be int16 [n_clips][n] or [n_clips][n][2]")
    return pcm, (2 if pcm.ndim == 3 else 1)


def _float(f64: bool):
    import torch
    return torch.float64 if f64 else torch.float32


def _ragged_host(f64: bool, signal, offsets, stereo_mode, with_trace, config):
    signal = np.ascontiguousarray(signal)
    off, n_clips = _lib.c_offsets(offsets)
    if off[n_clips] > signal.shape[0]:
        raise ValueError("offsets run past the end of the signal")
    if signal.dtype == np.int16:
        if signal.ndim not in (1, 2):
            raise ValueError("int16 signal must be [total] or interleaved [total][2]")
        return _host("dsp_classify_batch_ragged_pcm16_host", f64, signal, n_clips, with_trace, config, off, signal.ndim, int(stereo_mode))
    signal = np.ascontiguousarray(signal, np.float64 if f64 else np.float32)
    if signal.ndim != 1:
        raise ValueError("float signal must be one flat buffer [total]")
    return _host("dsp_classify_batch_ragged_host", f64, signal, n_clips, with_trace, config, off)


def _ragged_device(f64: bool, signal, offsets, labels, stereo_mode, config):
    off, n_clips, channels, _ = _lib.ragged_signal(signal, offsets, _float(f64))
    if channels:
        return _device("dsp_classify_batch_ragged_pcm16_device", f64, signal, n_clips, labels, config, off, channels, int(stereo_mode))
    return _device("dsp_classify_batch_ragged_device", f64, signal, n_clips, labels, config, off)


# ---- float32: sync/lib/classifier.cpp ---------------------------------------------------------------------------------------------

def classify_batch(clips: np.ndarray, with_trace: bool = False, config=None):
    """clips [n_clips][n] float32 (host) -> labels int32 [n_clips] (+ per-clip midpoints / band sums).
    config: None (sync/lib thresholds) or a 6-tuple / ClassifyConfig (dsp_classify_batch_host_cfg)."""
    clips = np.ascontiguousarray(np.atleast_2d(clips), np.float32)
    n_clips, n = clips.shape
    return _host("dsp_classify_batch_host_cfg", False, clips, n_clips, with_trace, config, n, n)


def classify_batch_pcm16(pcm: np.ndarray, stereo_mode: int = 0, with_trace: bool = False, config=None):
    """dsp_classify_batch_pcm16_host: the float32 classify() on int16 PCM [n_clips][n] (mono) or [n_clips][n][2] (interleaved stereo:
    channel 0 or the channels' average), converted in the kernels' loads as sync/sync.cpp:237-242 does (pcmSample / 32768.0)."""
    pcm, channels = _pcm_host(pcm)
    n_clips, n = pcm.shape[:2]
    return _host("dsp_classify_batch_pcm16_host", False, pcm, n_clips, with_trace, config, n, n, channels, int(stereo_mode))


def classify_device(clips, labels=None, config=None):
    """clips: cuda float32 [n_clips][n] -> cuda int32 labels; runs on torch's current stream."""
    n_clips, n = _lib.clips_device(clips, _float(False)).shape
    return _device("dsp_classify_batch_device_cfg", False, clips, n_clips, labels, config, n, clips.stride(0))


def classify_device_pcm16(pcm, labels=None, stereo_mode: int = 0, config=None):
    """pcm: cuda int16 [n_clips][n] or [n_clips][n][2] -> cuda int32 labels (dsp_classify_batch_pcm16_device), stream-ordered."""
    channels, stride = _lib.pcm_device(pcm)
    n_clips, n = pcm.shape[:2]
    return _device("dsp_classify_batch_pcm16_device", False, pcm, n_clips, labels, config, n, stride, channels, int(stereo_mode))


def classify_ragged(signal: np.ndarray, offsets, stereo_mode: int = 0, with_trace: bool = False, config=None):
    """Clips of different lengths in ONE call (dsp_classify_batch_ragged_host / _pcm16_host): `signal` is a flat host buffer -- float32
    [total], int16 [total] or interleaved stereo int16 [total][2] -- and clip c is samples [offsets[c], offsets[c + 1]).  Labels (and
    traces) as one classify() per clip gives them."""
    return _ragged_host(False, signal, offsets, stereo_mode, with_trace, config)


def classify_device_ragged(signal, offsets, labels=None, stereo_mode: int = 0, config=None):
    """The same on a flat cuda buffer (float32 [total], int16 [total] or [total][2]) -> cuda int32 labels, stream-ordered."""
    return _ragged_device(False, signal, offsets, labels, stereo_mode, config)


def classify_release(device: int = -1) -> None:
    _lib.check(_lib.load().dsp_classify_release(int(device)), "dsp_classify_release")


# ---- float64: donut-classifier/classifier.c ---------------------------------------------------------------------------------------

def classify_batch_f64(clips: np.ndarray, with_trace: bool = False, config=None):
    """The float64 classifier of donut-classifier/classifier.c (:83-192) on the GPU: clips [n_clips][n] float64 (host) -> labels
    int32 (+ per-clip float64 midpoints / band sums).  config: None (the file's thresholds 0.70 / 0.85, 45 dB, 75 / 300 / 100) or a
    6-tuple (keep_lo, keep_hi, midpoint_db, middle_max, above_min, below_min) of doubles."""
    clips = np.ascontiguousarray(np.atleast_2d(clips), np.float64)
    n_clips, n = clips.shape
    return _host("dsp_classify_batch_host", True, clips, n_clips, with_trace, config, n, n)


def classify_device_f64(clips, labels=None, config=None):
    """clips: cuda float64 [n_clips][n] -> cuda int32 labels (dsp_classify_batch_device_f64); runs on torch's current stream."""
    n_clips, n = _lib.clips_device(clips, _float(True)).shape
    return _device("dsp_classify_batch_device", True, clips, n_clips, labels, config, n, clips.stride(0))


def classify_batch_f64_pcm16(pcm: np.ndarray, stereo_mode: int = STEREO_CHANNEL0, with_trace: bool = False, config=None):
    """dsp_classify_batch_pcm16_host_f64: pcm int16 [n_clips][n] (mono) or [n_clips][n][2] (interleaved stereo; channel 0 as
    donut-classifier/classifier.c:286-297 or the channels' average) -> labels (+ midpoints / band sums), the samples converted in the
    kernels' loads exactly like classifier.c:55-59 (s / 32768.0)."""
    pcm, channels = _pcm_host(pcm)
    n_clips, n = pcm.shape[:2]
    return _host("dsp_classify_batch_pcm16_host", True, pcm, n_clips, with_trace, config, n, n, channels, int(stereo_mode))


def classify_device_f64_pcm16(pcm, labels=None, stereo_mode: int = STEREO_CHANNEL0, config=None):
    """pcm: cuda int16 [n_clips][n] or [n_clips][n][2] -> cuda int32 labels (dsp_classify_batch_pcm16_device_f64), stream-ordered on
    torch's current stream."""
    channels, stride = _lib.pcm_device(pcm)
    n_clips, n = pcm.shape[:2]
    return _device("dsp_classify_batch_pcm16_device", True, pcm, n_clips, labels, config, n, stride, channels, int(stereo_mode))


def classify_ragged_f64(signal: np.ndarray, offsets, stereo_mode: int = STEREO_CHANNEL0, with_trace: bool = False, config=None):
    """The float64 classifier on clips of different lengths in ONE call (dsp_classify_batch_ragged_host_f64 / _pcm16_host_f64): `signal`
    is a flat host buffer -- float64 [total], int16 [total] or interleaved stereo int16 [total][2] -- and clip c is samples
    [offsets[c], offsets[c + 1])."""
    return _ragged_host(True, signal, offsets, stereo_mode, with_trace, config)


def classify_device_ragged_f64(signal, offsets, labels=None, stereo_mode: int = STEREO_CHANNEL0, config=None):
    """The same on a flat cuda buffer (float64 [total], int16 [total] or [total][2]) -> cuda int32 labels, stream-ordered."""
    return _ragged_device(True, signal, offsets, labels, stereo_mode, config)


def classify_stats_f64(device: int = 0):
    """-> (segments, undecided, listed_clips) of the last float64 classifier pass on `device` (dsp_classify_stats_f64)."""
    a, b, c = C.c_long(), C.c_long(), C.c_long()
    _lib.check(_lib.load().dsp_classify_stats_f64(int(device), C.byref(a), C.byref(b), C.byref(c)), "dsp_classify_stats_f64")
    return a.value, b.value, c.value


def classify_release_f64(device: int = -1) -> None:
    _lib.check(_lib.load().dsp_classify_release_f64(int(device)), "dsp_classify_release_f64")


def find_midpoints(data: np.ndarray, fs: int = 16000) -> np.ndarray:
    """sync/lib/classifier.h:18: midpoints (seconds) of the loud 1000-3000 Hz stretches of one clip."""
    data = np.ascontiguousarray(data, np.float32).reshape(-1)
    out = np.zeros(64, np.float32)
    n = _lib.check(_lib.load().dsp_find_midpoints(data.ctypes.data, data.size, int(fs), out.ctypes.data, out.size), "dsp_find_midpoints")
    return out[:n].copy()
