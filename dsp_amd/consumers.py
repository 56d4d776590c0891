"""Host-side mirror of the reference's consumers of the MFCC matrix and of its resampler, over the C ABI:

  StopModel      classify_signal / audio_classifier_predict   2fa/audio/word/c/stop_detector.c:12-55,
                                                              audio_classifier_inference.c:38-90
  SpeakerModel   mfcc_target_speaker_llr_mean / classify_speaker   2fa/audio/pico-audio/src/speaker_gmm.c:127-141
  upsample_linear   upsampleLinear                             sync/particle/main.cpp:62-77
  Scanner        both per sliding window of long recordings     sync/sync.cpp:188-213 (one 1 s buffer at a time)
  StreamSession  the same for audio that is still arriving       sync/sync.cpp:188-213 (the capture loop itself, many feeds)
  Cmvn           sliding_cmvn                                   2fa/audio/speaker/gmm_utils.py:14-25
  SpeakerFrontEnd   extract_features_from_array, a batch at once  2fa/audio/speaker/gmm_utils.py:47-61
  SpeakerEnroller   map_adapt_gmm (means only)                  2fa/audio/speaker/adapt_ubm.py:72-86, 2fa/audio/adapt_ubm.py:97-110
  SpeakerVerifier   score_models / evaluate_dir (float GMMs)      2fa/audio/speaker/gmm_utils.py:99-126, evaluate_gmm.py
  Segmenter      segments on top of any scan's window scores (no counterpart in the reference: its callers threshold one window)
  TrialEvaluator   the threshold sweep, roc_curve and auc         2fa/audio/speaker/evaluate_gmm.py:73-81, generate_charts.py:52-54,68-69
  ScoreCalibrator   CAL_A * raw_score + CAL_B + CAL_C * log(n_frames), and the fit the reference leaves "to be learned on dev set"
                                                              2fa/audio/speaker/adapt_ubm.py:27-28,97-99
  ScoreNormalizer   Z-, T- and S-norm against cohorts, all members or the K closest (no counterpart in the reference: one threshold, 1.1,
                                                              for every model and clip, 2fa/audio/audio_driver.py:10)
  Vad            energy-based frame selection between the front end and the models (no counterpart in the reference:
                                                              extract_features_from_array keeps every row, gmm_utils.py:28-62)
  UbmTrainer     GaussianMixture(covariance_type="diag").fit    2fa/audio/speaker/train_ubm.py
  StopTrainer    the stop-word net's Keras fit, many seeds at once  2fa/audio/word/python/keyword_classifier.py:155-232
  quantize_gmm   the Q6 / Q11 / Q8 tables of gmm_params.inc     2fa/audio/pico-audio/src/gmm_params.inc

Trained parameters are passed in as arrays (the reference compiles them in from model_params.h / gmm_params.inc).
Tensors are HBM-resident torch tensors; Python only moves pointers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from .mfcc import MfccPlan, default_config, ragged_frame_offsets, speaker_config


def _scan_config(window_frames, hop_frames):
    window_frames, hop_frames = int(window_frames), int(hop_frames)
    if window_frames < 1 or hop_frames < 1:
        raise ValueError("window_frames and hop_frames must be >= 1")
    return _lib.ScanConfig(window_frames, hop_frames)


def _frame_offsets(frame_offsets):
    return _lib.offsets_array(frame_offsets, "frame_offsets", "rows")


def scan_window_offsets(frame_offsets, window_frames: int, hop_frames: int) -> np.ndarray:
    """Host only: int64 [n_recordings + 1], the prefix sums of the window counts of recordings of frame_offsets[r + 1] - frame_offsets[r]
    MFCC rows (dsp_scan_window_offsets): R >= window_frames rows give 1 + (R - window_frames) // hop_frames windows, fewer rows one."""
    cfg = _scan_config(window_frames, hop_frames)
    fo = _frame_offsets(frame_offsets)
    wo = np.zeros(fo.size, np.int64)
    _lib.check(_lib.load().dsp_scan_window_offsets(C.byref(cfg), fo.ctypes.data_as(_lib.LP), fo.size - 1, wo.ctypes.data_as(_lib.LP)),
               "dsp_scan_window_offsets")
    return wo


def _scan_mfcc(mfcc, fo, d):
    if not (hasattr(mfcc, "is_cuda") and mfcc.is_cuda and mfcc.dim() == 2 and mfcc.shape[1] == d):
        raise ValueError(f"mfcc must be a CUDA tensor [F][{d}]")
    if int(fo[-1]) > mfcc.shape[0]:
        raise ValueError("frame_offsets run past the end of mfcc")
    import torch
    if mfcc.dtype != torch.float32:
        raise ValueError("mfcc must be float32")
    return mfcc.contiguous()


class StopModel(_lib.Handle):
    """dsp_stop_model: StandardScaler + 4 dense layers (ReLU, ReLU, ReLU, sigmoid)."""

    _destroy = "dsp_stop_model_destroy"

    def __init__(self, params: dict, device: int = 0):
        """params: scaler_mean, scaler_scale [n_coef * max_frames], kernel0..3 ((in, out) row-major), bias0..3,
        optional n_coef (13), max_frames (500)."""
        keep = {k: np.ascontiguousarray(params[k], np.float32).reshape(-1) for k in
                ["scaler_mean", "scaler_scale"] + [f"kernel{i}" for i in range(4)] + [f"bias{i}" for i in range(4)]}
        p = _lib.StopModelParams()
        p.n_coef, p.max_frames = int(params.get("n_coef", 13)), int(params.get("max_frames", 500))
        if keep["scaler_mean"].size != p.n_coef * p.max_frames or keep["scaler_scale"].size != p.n_coef * p.max_frames:
            raise _lib.DspError("scaler arrays must have n_coef * max_frames entries")
        fan_in = p.n_coef * p.max_frames
        for i in range(4):
            p.units[i] = keep[f"bias{i}"].size
            if keep[f"kernel{i}"].size != fan_in * p.units[i]:
                raise _lib.DspError(f"kernel{i} must have {fan_in} x {p.units[i]} entries")
            p.kernel[i] = keep[f"kernel{i}"].ctypes.data
            p.bias[i] = keep[f"bias{i}"].ctypes.data
            fan_in = p.units[i]
        p.scaler_mean, p.scaler_scale = keep["scaler_mean"].ctypes.data, keep["scaler_scale"].ctypes.data
        self._create("dsp_stop_model_create", C.byref(p), device)
        self.device, self.n_coef, self.max_frames = device, p.n_coef, p.max_frames

    def predict(self, mfcc):
        """mfcc: cuda float32 [n_clips][T][n_coef] (frame-major, as compute_mfcc writes) -> prob float32 [n_clips]."""
        import torch
        n, t = mfcc.shape[0], mfcc.shape[1]
        prob = torch.empty(n, dtype=torch.float32, device=mfcc.device)
        _lib.check(self._L.dsp_stop_predict_device(self._h, mfcc.contiguous().data_ptr(), n, t, prob.data_ptr(), _lib.current_stream(mfcc)),
                   "dsp_stop_predict_device")
        return prob

    def classify_signal_batch(self, plan: MfccPlan, clips):
        """clips: cuda float32 [n_clips][samples] -> P("stop") float32 [n_clips] (classify_signal per clip)."""
        import torch
        _lib.clips_device(clips, torch.float32)
        prob = torch.empty(clips.shape[0], dtype=torch.float32, device=clips.device)
        _lib.check(self._L.dsp_classify_signal_batch_device(plan._h, self._h, clips.data_ptr(), clips.shape[0], clips.shape[1],
                                                            clips.stride(0), prob.data_ptr(), _lib.current_stream(clips)),
                   "dsp_classify_signal_batch_device")
        return prob

    def classify_signal_batch_pcm16(self, plan: MfccPlan, pcm, stereo_mode: int = 0):
        """pcm: cuda int16 [n_clips][samples] or [n_clips][samples][2] -> P("stop") (dsp_classify_signal_batch_pcm16_device: what
        main_test.c:198-217 decodes in front of classify_signal, converted in the kernel's load)."""
        import torch
        channels, stride = _lib.pcm_device(pcm)
        prob = torch.empty(pcm.shape[0], dtype=torch.float32, device=pcm.device)
        _lib.check(self._L.dsp_classify_signal_batch_pcm16_device(plan._h, self._h, pcm.data_ptr(), pcm.shape[0], pcm.shape[1], stride,
                                                                  channels, int(stereo_mode), prob.data_ptr(), _lib.current_stream(pcm)),
                   "dsp_classify_signal_batch_pcm16_device")
        return prob

    def classify_signal_ragged(self, plan: MfccPlan, signal, offsets, stereo_mode: int = 0):
        """Clips of different lengths in ONE launch (the files main_test.c:254-331 loops over): `signal` is a flat cuda buffer (float32
        [total], int16 [total] or stereo int16 [total][2]), clip c = samples [offsets[c], offsets[c + 1]) -> P("stop") per clip."""
        import torch
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        prob = torch.empty(n, dtype=torch.float32, device=signal.device)
        if channels:
            _lib.check(self._L.dsp_classify_signal_batch_ragged_pcm16_device(plan._h, self._h, ptr, n, off, channels, int(stereo_mode), prob.data_ptr(),
                                                                             _lib.current_stream(signal)), "dsp_classify_signal_batch_ragged_pcm16_device")
        else:
            _lib.check(self._L.dsp_classify_signal_batch_ragged_device(plan._h, self._h, ptr, n, off, prob.data_ptr(), _lib.current_stream(signal)),
                       "dsp_classify_signal_batch_ragged_device")
        return prob

    def scan(self, mfcc, frame_offsets, window_frames: int, hop_frames: int):
        """P("stop") per sliding window of rows of a ragged MFCC matrix (MfccPlan.clips_ragged with no frame cap): recording r = rows
        [frame_offsets[r], frame_offsets[r + 1]) -> (window_offsets int64 [n + 1], prob cuda float32 [window_offsets[-1]])."""
        import torch
        wo = scan_window_offsets(frame_offsets, window_frames, hop_frames)
        fo = _frame_offsets(frame_offsets)
        mfcc = _scan_mfcc(mfcc, fo, self.n_coef)
        prob = torch.empty(int(wo[-1]), dtype=torch.float32, device=mfcc.device)
        _lib.check(self._L.dsp_stop_scan_device(self._h, mfcc.data_ptr(), fo.size - 1, fo.ctypes.data_as(_lib.LP),
                                                C.byref(_scan_config(window_frames, hop_frames)), prob.data_ptr(), _lib.current_stream(mfcc)),
                   "dsp_stop_scan_device")
        return wo, prob

    def classify_signal(self, signal: np.ndarray) -> float:
        """The reference's classify_signal(signal, num_samples) on a host buffer."""
        signal = np.ascontiguousarray(signal, np.float32)
        return float(self._L.dsp_classify_signal(self._h, signal.ctypes.data, signal.size))

    @classmethod
    def train(cls, plan: MfccPlan, clips, labels, train_rows=None, val_rows=None, seeds=range(8), device: int = 0, max_frames: int = 500,
              units=(4, 2, 2, 1), **hyper):
        """Trains the net from audio (StopTrainer.fit, which takes `hyper`) and returns (the StopModel built on the best run, the fit's
        report).  clips: cuda float32 [n][samples]; labels 0 / 1 on the host; train_rows / val_rows default to every row (the validation
        loss is then the training rows' without dropout)."""
        mfcc = plan.clips(clips, max_frames)
        n, t, n_coef = mfcc.shape
        rows = np.arange(n, dtype=np.int32)
        trainer = StopTrainer(n_coef, max_frames, units, device)
        try:
            trainer.set(mfcc.reshape(n * t, n_coef), np.arange(n + 1, dtype=np.int64) * t, scaler_rows=train_rows)
            params, report = trainer.fit(labels, rows if train_rows is None else train_rows, rows if val_rows is None else val_rows, seeds=seeds, **hyper)
        finally:
            trainer.close()
        return cls(params, device), report


def stop_train_param_count(n_coef: int, max_frames: int, units) -> int:
    """Host only: the number of parameters of a model shape (dsp_stop_train_param_count)."""
    u = (C.c_int * 4)(*[int(v) for v in units])
    return _lib.check(_lib.load().dsp_stop_train_param_count(int(n_coef), int(max_frames), u), "dsp_stop_train_param_count")


def stop_train_uniform(seed: int, stream: int, counter: int) -> float:
    """Host only: the library's draw u in [0, 1) (dsp_stop_train_uniform)."""
    return float(_lib.load().dsp_stop_train_uniform(int(seed), int(stream), int(counter)))


def stop_train_order(n: int, seed: int, epoch: int) -> np.ndarray:
    """Host only: the permutation of 0 .. n - 1 an epoch's training rows come in (dsp_stop_train_order)."""
    order = np.empty(max(int(n), 0), np.int32)
    _lib.check(_lib.load().dsp_stop_train_order(int(n), int(seed), int(epoch), order.ctypes.data), "dsp_stop_train_order")
    return order


def stop_train_init(n_coef: int, max_frames: int, units, seed: int) -> np.ndarray:
    """Host only: the initial weights of a run, float64 [n_params] (dsp_stop_train_init)."""
    u = (C.c_int * 4)(*[int(v) for v in units])
    params = np.empty(stop_train_param_count(n_coef, max_frames, units), np.float64)
    _lib.check(_lib.load().dsp_stop_train_init(int(n_coef), int(max_frames), u, int(seed), params.ctypes.data), "dsp_stop_train_init")
    return params


def stop_model_from_training(n_coef: int, max_frames: int, units, params, mean, scale) -> dict:
    """Host only: flat float64 parameters plus the Scaler -> the dict StopModel takes, float32 (dsp_stop_model_from_training)."""
    u = (C.c_int * 4)(*[int(v) for v in units])
    n_in = int(n_coef) * int(max_frames)
    params = np.ascontiguousarray(params, np.float64).reshape(-1)
    mean, scale = np.ascontiguousarray(mean, np.float32).reshape(-1), np.ascontiguousarray(scale, np.float32).reshape(-1)
    if params.size != stop_train_param_count(n_coef, max_frames, units) or mean.size != n_in or scale.size != n_in:
        raise ValueError("params must hold n_params values, mean and scale n_coef * max_frames")
    arrays = np.empty(2 * n_in + params.size, np.float32)
    m = _lib.StopModelParams()
    _lib.check(_lib.load().dsp_stop_model_from_training(int(n_coef), int(max_frames), u, params.ctypes.data, mean.ctypes.data, scale.ctypes.data,
                                                        arrays.ctypes.data, C.byref(m)), "dsp_stop_model_from_training")
    out = {"n_coef": int(n_coef), "max_frames": int(max_frames), "scaler_mean": arrays[:n_in].copy(), "scaler_scale": arrays[n_in:2 * n_in].copy()}
    fan = n_in
    for l in range(4):
        k0, b0 = (m.kernel[l] - arrays.ctypes.data) // 4, (m.bias[l] - arrays.ctypes.data) // 4
        out[f"kernel{l}"], out[f"bias{l}"] = arrays[k0:k0 + fan * int(units[l])].copy(), arrays[b0:b0 + int(units[l])].copy()
        fan = int(units[l])
    return out


class StopTrainer(_lib.Handle):
    """dsp_stop_trainer: the stop-word net from labelled MFCC matrices, keyword_classifier.py:155-232 on the GPU -- the Scaler and many
    Keras-style fits (seeds, folds, dropout or learning rates) per launch over one standardised matrix.  One stream at a time per trainer."""

    _destroy = "dsp_stop_trainer_destroy"
    HYPER = {"learning_rate": 1e-3, "dropout": (0.3, 0.3, 0.2), "batch_size": 32, "epochs": 50, "patience": 10, "restore_best": True}

    def __init__(self, n_coef: int = 13, max_frames: int = 500, units=(4, 2, 2, 1), device: int = 0):
        self.units = tuple(int(u) for u in units)
        if len(self.units) != 4:
            raise ValueError("units must hold four layer widths")
        self._create("dsp_stop_trainer_create", device, int(n_coef), int(max_frames), (C.c_int * 4)(*self.units))
        self.n_coef, self.max_frames, self.device, self.n, self.f_used = int(n_coef), int(max_frames), device, 0, 0
        self.n_params = stop_train_param_count(n_coef, max_frames, self.units)
        self.mean = self.scale = None

    def set(self, mfcc, frame_offsets, scaler_rows=None, mean=None, scale=None):
        """The dataset of the calls that follow (dsp_stop_train_set_device): clip i is rows [frame_offsets[i], frame_offsets[i + 1]) of the
        ragged matrix mfcc (cuda float32 [F][n_coef]); fits the Scaler on `scaler_rows` (default: all clips) or takes the caller's mean /
        scale -> (mean, scale) float32 [n_coef * max_frames]."""
        fo = _frame_offsets(frame_offsets)
        if fo.size < 2:
            raise ValueError("frame_offsets must hold at least one clip")
        mfcc = _scan_mfcc(mfcc, fo, self.n_coef)
        if mfcc.device.index != self.device:
            raise ValueError(f"mfcc is on GPU {mfcc.device.index}, the trainer on GPU {self.device}")
        if (mean is None) != (scale is None):
            raise ValueError("mean and scale must be given together")
        n_in = self.n_coef * self.max_frames
        rows = None if scaler_rows is None else np.ascontiguousarray(scaler_rows, np.int32)
        given = None if mean is None else (np.ascontiguousarray(mean, np.float32).reshape(-1), np.ascontiguousarray(scale, np.float32).reshape(-1))
        if given is not None and (given[0].size != n_in or given[1].size != n_in):
            raise ValueError("mean and scale must hold n_coef * max_frames values")
        m, s = np.empty(n_in, np.float32), np.empty(n_in, np.float32)
        self.n = 0
        _lib.check(self._L.dsp_stop_train_set_device(self._h, mfcc.data_ptr(), fo.size - 1, fo.ctypes.data, None if rows is None else rows.ctypes.data,
                                                     0 if rows is None else rows.size, None if given is None else given[0].ctypes.data,
                                                     None if given is None else given[1].ctypes.data, m.ctypes.data, s.ctypes.data, self._stream()),
                   "dsp_stop_train_set_device")
        self.n, self.f_used = fo.size - 1, int(self._L.dsp_stop_train_used_features(self._h))
        self.mean, self.scale = m, s
        return m, s

    def rows(self):
        """the standardised rows of the dataset, float32 [n][F_used] on the host (used feature c * T_used + t is input c * max_frames + t)"""
        z = np.empty((self.n, self.f_used), np.float32)
        _lib.check(self._L.dsp_stop_train_rows_host(self._h, z.ctypes.data, self._stream()), "dsp_stop_train_rows_host")
        return z

    def train(self, runs, labels, prob: bool = True):
        """Trains runs = [dict(train_rows=, val_rows=, seed=, and any of HYPER), ...] together (dsp_stop_train_runs_device) -> (results:
        numpy records of STOP_TRAIN_RESULT_DTYPE [P], history cuda float64 [P][max epochs][2], prob cuda float64 [P][n] or None, params
        cuda float64 [P][n_params])."""
        import torch
        labels = np.ascontiguousarray(labels, np.int32)
        if labels.size != self.n:
            raise ValueError(f"labels must hold the dataset's {self.n} clips")
        table = (_lib.StopTrainRun * max(1, len(runs)))()
        keep, max_epochs = [], 1
        for k, r in enumerate(runs):
            unknown = set(r) - set(self.HYPER) - {"train_rows", "val_rows", "seed"}
            if unknown:
                raise ValueError(f"runs[{k}]: unknown keys {sorted(unknown)}")
            h = {**self.HYPER, **r}
            tr = np.ascontiguousarray(h["train_rows"], np.int32).reshape(-1)
            va = np.ascontiguousarray(h["val_rows"] if h.get("val_rows") is not None else [], np.int32).reshape(-1)
            keep += [tr, va]
            drop = tuple(float(d) for d in h["dropout"])
            if len(drop) != 3:
                raise ValueError(f"runs[{k}]: dropout must hold three rates")
            table[k] = _lib.StopTrainRun(tr.ctypes.data if tr.size else None, va.ctypes.data if va.size else None, tr.size, va.size, int(h.get("seed", 0)),
                                         float(h["learning_rate"]), (C.c_double * 3)(*drop), int(h["batch_size"]), int(h["epochs"]), int(h["patience"]),
                                         int(bool(h["restore_best"])))
            max_epochs = max(max_epochs, int(h["epochs"]))
        results = np.zeros(len(runs), _lib.STOP_TRAIN_RESULT_DTYPE)
        dev = torch.device("cuda", self.device)
        history = torch.empty((len(runs), max_epochs, 2), dtype=torch.float64, device=dev)
        params = torch.empty((len(runs), self.n_params), dtype=torch.float64, device=dev)
        p = torch.empty((len(runs), self.n), dtype=torch.float64, device=dev) if prob else None
        _lib.check(self._L.dsp_stop_train_runs_device(self._h, table, len(runs), labels.ctypes.data, results.ctypes.data, history.data_ptr(),
                                                      p.data_ptr() if prob else None, params.data_ptr(), self._stream()), "dsp_stop_train_runs_device")
        return results, history, p, params

    def fit(self, labels, train_rows, val_rows, seeds=range(8), **hyper):
        """All seeds in one call -> (the parameter dict StopModel takes for the run with the lowest best_val_loss, ties to the earliest
        seed; report: dict with every run's result, so that a caller sees how many seeds died)."""
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError("seeds must hold at least one seed")
        runs = [dict(train_rows=train_rows, val_rows=val_rows, seed=s, **hyper) for s in seeds]
        results, history, _p, params = self.train(runs, labels, prob=False)
        loss = np.where(np.isnan(results["best_val_loss"]), np.inf, results["best_val_loss"])
        best = int(np.argmin(loss))                                  # (argmin: the first of equals)
        model = stop_model_from_training(self.n_coef, self.max_frames, self.units, params[best].cpu().numpy(), self.mean, self.scale)
        return model, {"best": best, "seed": seeds[best], "seeds": seeds, "results": results, "history": history.cpu().numpy(),
                       "params": params[best].cpu().numpy(), "n_dead_runs": int((results["n_dead_units"] > 0).sum())}


def _gmm_params(g: dict):
    keep = (np.ascontiguousarray(g["means"], np.int8), np.ascontiguousarray(g["inv_covs"], np.int32),
            np.ascontiguousarray(g["log_consts"], np.int16))
    p = _lib.GmmParams()
    p.k, p.d = keep[0].shape
    p.means, p.inv_covs, p.log_consts = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data
    return p, keep


class SpeakerModel(_lib.Handle):
    """dsp_speaker_model: target GMM vs UBM in the reference's fixed point (Q6 / Q11 / Q8)."""

    _destroy = "dsp_speaker_model_destroy"

    def __init__(self, target: dict, ubm: dict, device: int = 0):
        pt, _k1 = _gmm_params(target)
        pu, _k2 = _gmm_params(ubm)
        self._create("dsp_speaker_model_create", C.byref(pt), C.byref(pu), device)
        self.device, self.d = device, pt.d

    def llr(self, mfcc, per_frame: bool = False):
        """mfcc: cuda float32 [n_clips][T][d] -> (llr_mean int64 [n], label int32 [n][, ll_target, ll_ubm int64 [n][T]])."""
        import torch
        n, t = mfcc.shape[0], mfcc.shape[1]
        mean = torch.empty(n, dtype=torch.int64, device=mfcc.device)
        label = torch.empty(n, dtype=torch.int32, device=mfcc.device)
        lt = torch.empty((n, t), dtype=torch.int64, device=mfcc.device) if per_frame else None
        lu = torch.empty((n, t), dtype=torch.int64, device=mfcc.device) if per_frame else None
        _lib.check(self._L.dsp_speaker_llr_device(self._h, mfcc.contiguous().data_ptr(), n, t, mean.data_ptr(), label.data_ptr(),
                                                  lt.data_ptr() if per_frame else None, lu.data_ptr() if per_frame else None,
                                                  _lib.current_stream(mfcc)), "dsp_speaker_llr_device")
        return (mean, label, lt, lu) if per_frame else (mean, label)

    def llr_ragged(self, mfcc, frame_offsets, per_frame: bool = False):
        """The same per clip of a ragged MFCC matrix (MfccPlan.clips_ragged): mfcc cuda float32 [F][d], clip c = rows
        [frame_offsets[c], frame_offsets[c + 1]), every clip >= 1 row -> (llr_mean int64 [n], label int32 [n][, ll_target, ll_ubm int64 [F]])."""
        import torch
        fo = np.ascontiguousarray(np.asarray(frame_offsets, dtype=np.int64))
        if fo.ndim != 1 or fo.size < 1:
            raise ValueError("frame_offsets must hold n_clips + 1 rows")
        if mfcc.dim() != 2 or mfcc.shape[1] != self.d or int(fo[-1]) > mfcc.shape[0]:
            raise ValueError(f"mfcc must be [F][{self.d}] with F >= frame_offsets[-1]")
        mfcc = mfcc.contiguous()
        n, rows = fo.size - 1, int(fo[-1])
        mean = torch.empty(n, dtype=torch.int64, device=mfcc.device)
        label = torch.empty(n, dtype=torch.int32, device=mfcc.device)
        lt = torch.empty(rows, dtype=torch.int64, device=mfcc.device) if per_frame else None
        lu = torch.empty(rows, dtype=torch.int64, device=mfcc.device) if per_frame else None
        _lib.check(self._L.dsp_speaker_llr_ragged_device(self._h, mfcc.data_ptr(), n, fo.ctypes.data_as(_lib.LP), mean.data_ptr(),
                                                         label.data_ptr(), lt.data_ptr() if per_frame else None,
                                                         lu.data_ptr() if per_frame else None, _lib.current_stream(mfcc)), "dsp_speaker_llr_ragged_device")
        return (mean, label, lt, lu) if per_frame else (mean, label)

    def scan(self, mfcc, frame_offsets, window_frames: int, hop_frames: int):
        """The speaker LLR per sliding window of rows of a ragged MFCC matrix (as StopModel.scan), every recording >= 1 row
        -> (window_offsets int64 [n + 1], llr_mean cuda int64, labels cuda int32 [window_offsets[-1]])."""
        import torch
        wo = scan_window_offsets(frame_offsets, window_frames, hop_frames)
        fo = _frame_offsets(frame_offsets)
        mfcc = _scan_mfcc(mfcc, fo, self.d)
        nw = int(wo[-1])
        mean = torch.empty(nw, dtype=torch.int64, device=mfcc.device)
        label = torch.empty(nw, dtype=torch.int32, device=mfcc.device)
        _lib.check(self._L.dsp_speaker_scan_device(self._h, mfcc.data_ptr(), fo.size - 1, fo.ctypes.data_as(_lib.LP),
                                                   C.byref(_scan_config(window_frames, hop_frames)), mean.data_ptr(), label.data_ptr(), _lib.current_stream(mfcc)),
                   "dsp_speaker_scan_device")
        return wo, mean, label


class Scanner(_lib.Handle):
    """dsp_scanner: recordings back to back in HBM -> ragged MFCC matrix -> P("stop") and / or the speaker LLR per window of
    window_frames rows every hop_frames rows.  One stream at a time per scanner."""

    _destroy = "dsp_scanner_destroy"

    def __init__(self, plan: MfccPlan, stop: StopModel | None = None, speaker: SpeakerModel | None = None, window_frames: int = 98,
                 hop_frames: int = 10):
        if stop is None and speaker is None:
            raise ValueError("a Scanner needs a stop model, a speaker model or both")
        self.cfg = _scan_config(window_frames, hop_frames)
        self._create("dsp_scanner_create", plan._h, stop._h if stop else None, speaker._h if speaker else None, C.byref(self.cfg))
        self.plan, self.stop, self.speaker = plan, stop, speaker      # (the scanner borrows them: keep them alive)

    def run(self, signal, offsets, stereo_mode: int = 0):
        """signal: cuda float32 [total], int16 [total] (mono) or int16 [total][2] (stereo), recording r = samples [offsets[r], offsets[r + 1])
        per channel -> (window_offsets int64 [n + 1], prob float32 | None, llr_mean int64 | None, labels int32 | None), one entry per window."""
        import torch
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        if channels and stereo_mode not in (0, 1):
            raise ValueError("stereo_mode must be 0 (channel 0) or 1 (average)")
        fo = ragged_frame_offsets(self.plan.cfg, (off, n), 2**31 - 1)
        wo = scan_window_offsets(fo, self.cfg.window_frames, self.cfg.hop_frames)
        nw, dev = int(wo[-1]), signal.device
        prob = torch.empty(nw, dtype=torch.float32, device=dev) if self.stop else None
        mean = torch.empty(nw, dtype=torch.int64, device=dev) if self.speaker else None
        label = torch.empty(nw, dtype=torch.int32, device=dev) if self.speaker else None
        ptrs = [t.data_ptr() if t is not None else None for t in (prob, mean, label)]
        st = _lib.current_stream(signal)
        if channels:
            _lib.check(self._L.dsp_scanner_run_pcm16_device(self._h, ptr, n, off, channels, int(stereo_mode), *ptrs, st), "dsp_scanner_run_pcm16_device")
        else:
            _lib.check(self._L.dsp_scanner_run_device(self._h, ptr, n, off, *ptrs, st), "dsp_scanner_run_device")
        return wo, prob, mean, label


def _chunk_offsets(chunk_offsets, n_streams):
    co = _lib.long_array(chunk_offsets, n_streams + 1, "chunk_offsets")
    if co[0] < 0 or (np.diff(co) < 0).any():
        raise ValueError("chunk_offsets must be non-negative and non-decreasing")
    return co


def stream_push_plan(cfg, received, chunk_offsets, window_frames=None, hop_frames=None):
    """Host only (dsp_stream_push_plan): what a push of chunks [chunk_offsets[s], chunk_offsets[s + 1]) emits for streams that have
    received `received[s]` samples so far (None: none) -> (row_offsets int64 [n + 1], window_offsets int64 [n + 1] | None), the prefix
    sums of the new MFCC rows and, when window_frames / hop_frames are given, of the new windows."""
    if (window_frames is None) != (hop_frames is None):
        raise ValueError("window_frames and hop_frames go together")
    co = np.ascontiguousarray(np.asarray(chunk_offsets, dtype=np.int64))
    if co.ndim != 1 or co.size < 1:
        raise ValueError("chunk_offsets must hold n_streams + 1 positions")
    n = co.size - 1
    co = _chunk_offsets(co, n)
    rec = None
    if received is not None:
        rec = _lib.long_array(received, n, "received")
        if (rec < 0).any():
            raise ValueError("received must be non-negative")
    scan = None
    if window_frames is not None:
        scan = _scan_config(window_frames, hop_frames)
        if scan.hop_frames > scan.window_frames:
            raise ValueError("hop_frames must not exceed window_frames")
    ro = np.zeros(n + 1, np.int64)
    wo = np.zeros(n + 1, np.int64) if scan is not None else None
    _lib.check(_lib.load().dsp_stream_push_plan(C.byref(cfg), C.byref(scan) if scan is not None else None,
                                                rec.ctypes.data_as(_lib.LP) if rec is not None else None, co.ctypes.data_as(_lib.LP), n,
                                                ro.ctypes.data_as(_lib.LP), wo.ctypes.data_as(_lib.LP) if wo is not None else None), "dsp_stream_push_plan")
    return ro, wo


class StreamSession(_lib.Handle):
    """dsp_stream_session: n_streams live streams on one GPU.  Every push hands over the next chunk of each stream (any length) and
    returns the MFCC rows and the window scores that became complete with it; concatenated over the pushes they are, bit for bit,
    MfccPlan.clips_ragged and Scanner.run on the whole recording -- except that a stream has no window before it holds window_frames
    rows.  dtype: torch.float32 samples, or torch.int16 PCM ([total] mono, [total][2] interleaved stereo with stereo_mode 0 = channel
    0 / 1 = average; channels=2 selects stereo).  rate_in: the feeds arrive at this rate instead of the plan's -- the session puts a
    StreamResampler (rate_in -> the plan's sample_rate, same dtype / channels / stereo_mode) in front of itself, push() takes chunks at
    rate_in, and counts() keeps counting samples at the plan's rate.  One stream at a time per session."""

    _destroy = "dsp_stream_session_destroy"
    resampler = None

    def __init__(self, plan: MfccPlan, n_streams: int, stop: StopModel | None = None, speaker: SpeakerModel | None = None,
                 window_frames: int = 98, hop_frames: int = 10, dtype=None, stereo_mode: int = 0, channels: int = 1, rate_in: int | None = None):
        dtype, channels, stereo_mode, n_streams, pcm16 = _lib.stream_format(dtype, channels, stereo_mode, n_streams)
        self.cfg = _scan_config(window_frames, hop_frames) if (stop or speaker) else None
        if self.cfg is not None and self.cfg.hop_frames > self.cfg.window_frames:
            raise ValueError("hop_frames must not exceed window_frames")
        if rate_in is not None:      # the resampler decodes the caller's format; the session behind it takes its float mono output
            from .resample import StreamResampler
            self.resampler = StreamResampler(rate_in, plan.cfg.sample_rate, n_streams, dtype, stereo_mode, channels, plan.device)
        own = (1, 0, 0) if self.resampler is not None else (channels, stereo_mode, pcm16)
        self._create("dsp_stream_session_create", plan._h, stop._h if stop else None, speaker._h if speaker else None,
                     C.byref(self.cfg) if self.cfg is not None else None, n_streams, *own)
        self.plan, self.stop, self.speaker = plan, stop, speaker      # (the session borrows them: keep them alive)
        self.n_streams, self.dtype, self.channels, self.device = n_streams, dtype, channels, plan.device
        if self.resampler is not None:
            _lib.check(self._L.dsp_stream_session_attach_resampler(self._h, self.resampler._h), "dsp_stream_session_attach_resampler")

    def close(self):
        super().close()      # the session first: it holds the resampler's handle
        if self.resampler is not None:
            self.resampler.close()
            self.resampler = None

    def counts(self):
        """-> (samples received, rows emitted, windows emitted), int64 [n_streams] each."""
        out = [np.zeros(self.n_streams, np.int64) for _ in range(3)]
        _lib.check(self._L.dsp_stream_session_counts(self._h, *[a.ctypes.data_as(_lib.LP) for a in out]), "dsp_stream_session_counts")
        return tuple(out)

    def reset(self, streams=None):
        """Forget the named streams' samples, rows and counters (None: all of them, which also revives a broken session)."""
        if streams is None:
            _lib.check(self._L.dsp_stream_session_reset(self._h, None, 0, None), "dsp_stream_session_reset")
            return
        idx = np.ascontiguousarray(np.asarray(streams, dtype=np.int64))
        if idx.ndim != 1 or (idx.size and (idx.min() < 0 or idx.max() >= self.n_streams)):
            raise ValueError(f"streams must name streams 0 .. {self.n_streams - 1}")
        _lib.check(self._L.dsp_stream_session_reset(self._h, idx.ctypes.data_as(_lib.LP), idx.size, None), "dsp_stream_session_reset")

    def push(self, chunks, chunk_offsets, want_rows: bool = True):
        """chunks: a contiguous CUDA tensor of the session's dtype on the plan's device ([total], or [total][2] for stereo), stream s's
        chunk = sample frames [chunk_offsets[s], chunk_offsets[s + 1]) -> (row_offsets int64 [n + 1], rows float32 [new rows][n_mfcc] | None,
        window_offsets int64 [n + 1], prob float32 | None, llr_mean int64 | None, label int32 | None), one entry per new window."""
        import torch
        if not (isinstance(chunks, torch.Tensor) and chunks.is_cuda and chunks.is_contiguous()):
            raise ValueError("chunks must be a contiguous CUDA tensor")
        if chunks.dtype != self.dtype:
            raise ValueError(f"chunks must be {str(self.dtype).replace('torch.', '')}, as the session was created")
        if chunks.device.index != self.device:
            raise ValueError(f"chunks must live on the session's device (cuda:{self.device})")
        if not (chunks.dim() == 1 if self.channels == 1 else (chunks.dim() == 2 and chunks.shape[1] == 2)):
            raise ValueError("chunks must be [total] (mono) or [total][2] (interleaved stereo), as the session was created")
        co = _chunk_offsets(chunk_offsets, self.n_streams)
        if int(co[-1]) > chunks.shape[0]:
            raise ValueError("chunk_offsets run past the end of chunks")
        rs = self.resampler
        at_rate = rs.plan(co) if rs is not None else co      # the chunks as the MFCC front end will see them
        ro, wo = stream_push_plan(self.plan.cfg, self.counts()[0], at_rate, *((self.cfg.window_frames, self.cfg.hop_frames) if self.cfg is not None else ()))
        if wo is None:
            wo = np.zeros(self.n_streams + 1, np.int64)
        nr, nw, dev = int(ro[-1]), int(wo[-1]), chunks.device
        rows = torch.empty((nr, self.plan.cfg.n_mfcc), dtype=torch.float32, device=dev) if want_rows else None
        prob = torch.empty(nw, dtype=torch.float32, device=dev) if self.stop else None
        mean = torch.empty(nw, dtype=torch.int64, device=dev) if self.speaker else None
        label = torch.empty(nw, dtype=torch.int32, device=dev) if self.speaker else None
        ptrs = [t.data_ptr() if t is not None else None for t in (rows, prob, mean, label)]
        ro2, wo2 = np.zeros_like(ro), np.zeros_like(wo)
        _lib.check(self._L.dsp_stream_push_device(self._h, chunks.data_ptr(), co.ctypes.data_as(_lib.LP), *ptrs, ro2.ctypes.data_as(_lib.LP),
                                                  wo2.ctypes.data_as(_lib.LP), _lib.current_stream(chunks)), "dsp_stream_push_device")
        if not (np.array_equal(ro, ro2) and np.array_equal(wo, wo2)):
            raise _lib.DspError("dsp_stream_push_device emitted other rows / windows than dsp_stream_push_plan announced")
        return ro2, rows, wo2, prob, mean, label


class Cmvn(_lib.Handle):
    """dsp_cmvn: sliding cepstral mean and variance normalisation of a ragged MFCC matrix -- row t of a recording by the mean and the
    population standard deviation of rows [t - window // 2, t + window // 2) of its own recording (the UBM's feature space)."""

    _destroy = "dsp_cmvn_destroy"

    def __init__(self, d: int, window: int = 300, device: int = 0):
        d, window = int(d), int(window)
        if not 1 <= d <= 16:
            raise ValueError("d must be 1 .. 16")
        if window < 2:
            raise ValueError("window must be >= 2")
        self._create("dsp_cmvn_create", int(device), d, window)
        self.d, self.window, self.device = d, window, int(device)

    def apply(self, mfcc, frame_offsets):
        """mfcc: cuda float32 [F][d], recording r = rows [frame_offsets[r], frame_offsets[r + 1]) -> a new cuda float32 [F][d]; rows of
        no recording are zeros."""
        import torch
        fo = _frame_offsets(frame_offsets)
        mfcc = _scan_mfcc(mfcc, fo, self.d)
        out = torch.zeros_like(mfcc)
        if fo.size > 1 and mfcc.numel():
            _lib.check(self._L.dsp_cmvn_ragged_device(self._h, mfcc.data_ptr(), fo.size - 1, fo.ctypes.data_as(_lib.LP), out.data_ptr(), _lib.current_stream(mfcc)),
                       "dsp_cmvn_ragged_device")
        return out


class SpeakerFrontEnd(_lib.Closing):
    """extract_features_from_array (gmm_utils.py:47-61) for a whole batch: librosa.feature.mfcc(n_mfcc 13, n_fft 400, hop 160) as
    speaker_config() states it, then sliding_cmvn over a window of 300 rows -- the rows the float GMMs are trained and scored on."""

    CMVN_WINDOW = 300      # gmm_utils.py:14
    plan = cmvn = None

    def __init__(self, device: int = 0):
        self.device = int(device)
        self.plan = MfccPlan(speaker_config(), self.device)
        self.cmvn = Cmvn(self.plan.cfg.n_mfcc, self.CMVN_WINDOW, self.device)

    def close(self):
        for part in ("cmvn", "plan"):
            if getattr(self, part):
                getattr(self, part).close()
                setattr(self, part, None)

    def features(self, signal, offsets, vad=None):
        """signal: cuda float32 [total] at 16 kHz, clip c = samples [offsets[c], offsets[c + 1]) -> (feats, frame_offsets): cuda float32
        [F][13] with clip c's rows in [frame_offsets[c], frame_offsets[c + 1]) (numpy int64), 1 + n // 160 of them for n samples.  As it
        is, the input of UbmTrainer.fit, SpeakerEnroller.enroll and SpeakerVerifier.verify.  vad: a Vad made for this front end's plan:
        the rows it keeps are selected AFTER the CMVN (Kaldi's order: silence still shapes the sliding statistics), and frame_offsets
        are its kept_offsets; ValueError names the first clip that keeps no row (the enroller would refuse it)."""
        off = np.asarray(offsets, np.int64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("offsets must be a 1-d array of n_clips + 1 sample positions")
        n_fft = self.plan.cfg.n_fft
        short = np.flatnonzero(np.diff(off) < n_fft)
        if short.size:      # gmm_utils.py:49-50 returns no rows for such a clip
            c = int(short[0])
            raise ValueError(f"clip {c} has {int(off[c + 1] - off[c])} samples: extract_features_from_array yields no rows below n_fft = {n_fft}")
        mfcc, fo = self.plan.clips_ragged(signal, off, 2**31 - 1)
        feats = self.cmvn.apply(mfcc, fo)
        if vad is None:
            return feats, fo
        flags, kept, _records = vad.run(signal, off, fo)
        silent = np.flatnonzero(np.diff(kept) == 0)
        if silent.size:
            raise ValueError(f"clip {int(silent[0])} keeps no row: the voice activity detector found no speech in it")
        return vad.select(feats, flags, fo, kept), kept


def _gmm_float_params(params: dict, name: str):
    """float GMM dict -> (GmmFloatParams, k, d, the float64 arrays its pointers point into: to be kept until the struct has been read)"""
    keep = {key: np.ascontiguousarray(params[key], np.float64) for key in ("log_consts", "means", "inv_covs")}
    if keep["means"].ndim != 2 or keep["inv_covs"].shape != keep["means"].shape or keep["log_consts"].shape != keep["means"].shape[:1]:
        raise ValueError(f"{name}: means and inv_covs must be [k][d], log_consts [k]")
    k, d = keep["means"].shape
    if not (1 <= k <= 64 and 1 <= d <= 16):
        raise ValueError(f"{name}: k must be 1 .. 64 and d 1 .. 16")
    return _lib.GmmFloatParams(k, d, *(keep[key].ctypes.data for key in ("log_consts", "means", "inv_covs"))), k, d, keep


class SpeakerEnroller(_lib.Handle):
    """dsp_speaker_enroller: MAP adaptation of a float UBM's means to each speaker of a ragged matrix of (CMVN'd) feature rows."""

    _destroy = "dsp_speaker_enroller_destroy"
    MODES = {"relevance": _lib.MAP_RELEVANCE, "fixed_alpha": _lib.MAP_FIXED_ALPHA}

    def __init__(self, ubm_float: dict, device: int = 0):
        """ubm_float: log_consts [k], means [k][d], inv_covs [k][d] -- the DOUBLE_GMM arrays of gmm_params.inc (log_consts = log w -
        0.5 sum log(2 pi var), inv_covs = 1 / var)."""
        p, k, d, _keep = _gmm_float_params(ubm_float, "ubm_float")
        self._create("dsp_speaker_enroller_create", C.byref(p), int(device))
        self.k, self.d, self.device = k, d, int(device)

    def enroll(self, feats, frame_offsets, mode: str = "relevance", relevance_factor: float = 16.0, fixed_alpha: float = 0.7):
        """feats: cuda float32 [F][d], speaker s = rows [frame_offsets[s], frame_offsets[s + 1]), every speaker >= 1 row -> a dict of cuda
        tensors: means float32 [S][k][d], means_q6 int8 [S][k][d], counts float32 [S][k], ll_mean float32 [S], saturated int32 [S]."""
        import torch
        if mode not in self.MODES:
            raise ValueError("mode must be 'relevance' or 'fixed_alpha'")
        relevance_factor, fixed_alpha = float(relevance_factor), float(fixed_alpha)
        if mode == "relevance" and not (0.0 < relevance_factor < float("inf")):
            raise ValueError("relevance_factor must be > 0 and finite")
        if mode == "fixed_alpha" and not (0.0 <= fixed_alpha <= 1.0):
            raise ValueError("fixed_alpha must lie in [0, 1]")
        fo = _frame_offsets(frame_offsets)
        feats = _scan_mfcc(feats, fo, self.d)
        if (np.diff(fo) == 0).any():
            raise ValueError(f"speaker {int(np.flatnonzero(np.diff(fo) == 0)[0])} has no rows")
        n, dev = fo.size - 1, feats.device
        out = {"means": torch.empty((n, self.k, self.d), dtype=torch.float32, device=dev),
               "means_q6": torch.empty((n, self.k, self.d), dtype=torch.int8, device=dev),
               "counts": torch.empty((n, self.k), dtype=torch.float32, device=dev),
               "ll_mean": torch.empty(n, dtype=torch.float32, device=dev),
               "saturated": torch.empty(n, dtype=torch.int32, device=dev)}
        cfg = _lib.EnrollConfig(self.MODES[mode], relevance_factor, fixed_alpha)
        _lib.check(self._L.dsp_speaker_enroll_ragged_device(self._h, feats.data_ptr(), n, fo.ctypes.data_as(_lib.LP), C.byref(cfg),
                                                            *[out[key].data_ptr() for key in ("means", "means_q6", "counts", "ll_mean", "saturated")],
                                                            _lib.current_stream(feats)), "dsp_speaker_enroll_ragged_device")
        return out

    @staticmethod
    def speaker_model(means_q6, ubm_int: dict, device: int = 0) -> SpeakerModel:
        """The SpeakerModel of one enrolled speaker: means_q6 int8 [k][d] (a row of enroll()'s means_q6, tensor or array) as the target's
        means, the UBM's own inv_covs (Q11) and log_consts (Q8) as the target's, against ubm_int (means, inv_covs, log_consts)."""
        q6 = means_q6.cpu().numpy() if hasattr(means_q6, "cpu") else np.asarray(means_q6)
        if q6.dtype != np.int8 or q6.shape != np.shape(ubm_int["means"]):
            raise ValueError("means_q6 must be int8 [k][d], the shape of the UBM's means")
        return SpeakerModel({"means": q6, "inv_covs": ubm_int["inv_covs"], "log_consts": ubm_int["log_consts"]}, ubm_int, device)


class SpeakerVerifier(_lib.Handle):
    """dsp_speaker_verifier: every clip of a ragged matrix of (CMVN'd) feature rows against a float UBM and S enrolled speakers -- the
    mean log-sum-exp log-likelihood of each model and target.score - ubm.score per (clip, speaker)."""

    _destroy = "dsp_speaker_verifier_destroy"
    OUTPUTS = ("llr", "ll_ubm", "ll_target", "best", "best_llr")

    def __init__(self, ubm_float: dict, device: int = 0):
        """ubm_float: log_consts [k], means [k][d], inv_covs [k][d], as SpeakerEnroller takes them.  No device is touched here."""
        p, k, d, _keep = _gmm_float_params(ubm_float, "ubm_float")
        self._create("dsp_speaker_verifier_create", C.byref(p), int(device))
        self.k, self.d, self.device = k, d, int(device)

    def verify(self, feats, frame_offsets, means, want=("llr", "ll_ubm", "best", "best_llr")):
        """feats: cuda float32 [F][d], clip c = rows [frame_offsets[c], frame_offsets[c + 1]), every clip >= 1 row; means: cuda float32
        [S][k][d] (SpeakerEnroller.enroll(...)["means"] as it is) -> a dict of cuda tensors, those named in `want` of: llr float32 [C][S],
        ll_ubm float32 [C], ll_target float32 [C][S], best int32 [C] (the smallest s with the largest llr), best_llr float32 [C]."""
        feats, fo, means, want = self._inputs(feats, frame_offsets, means, want, "clip")
        n, n_spk = fo.size - 1, means.shape[0]
        out, ptrs = self._outputs(n, n_spk, want, feats.device)
        _lib.check(self._L.dsp_speaker_verify_ragged_device(self._h, feats.data_ptr(), n, fo.ctypes.data_as(_lib.LP), means.data_ptr(), n_spk, *ptrs,
                                                            _lib.current_stream(feats)), "dsp_speaker_verify_ragged_device")
        return out

    def _outputs(self, n, n_spk, want, dev):
        """-> (the tensors `want` names for n clips or windows and n_spk speakers, their addresses in OUTPUTS order, None where not wanted)"""
        import torch
        shape = {"llr": (n, n_spk), "ll_ubm": (n,), "ll_target": (n, n_spk), "best": (n,), "best_llr": (n,)}
        out = {key: torch.empty(shape[key], dtype=torch.int32 if key == "best" else torch.float32, device=dev) for key in want}
        return out, [out[key].data_ptr() if key in out else None for key in self.OUTPUTS]

    def _inputs(self, feats, frame_offsets, means, want, what):
        """the argument checks verify and scan share -> (feats, fo, means, want)"""
        import torch
        want = tuple(want)
        if not want or any(key not in self.OUTPUTS for key in want):
            raise ValueError(f"want must name at least one of {self.OUTPUTS}")
        fo = _frame_offsets(frame_offsets)
        if (np.diff(fo) == 0).any():
            raise ValueError(f"{what} {int(np.flatnonzero(np.diff(fo) == 0)[0])} has no rows")
        feats = _scan_mfcc(feats, fo, self.d)
        if not (isinstance(means, torch.Tensor) and means.is_cuda and means.dtype == torch.float32 and means.dim() == 3
                and tuple(means.shape[1:]) == (self.k, self.d)):
            raise ValueError(f"means must be a float32 CUDA tensor [S][{self.k}][{self.d}]")
        if means.device != feats.device:
            raise ValueError("means and feats must be on the same device")
        return feats, fo, means.contiguous(), want

    def scan(self, feats, frame_offsets, means, window_frames: int, hop_frames: int, want=("llr", "ll_ubm", "best", "best_llr")):
        """The same scores per sliding window of window_frames rows every hop_frames rows (dsp_speaker_float_scan_device): feats cuda
        float32 [F][d], recording r = rows [frame_offsets[r], frame_offsets[r + 1]), CMVN'd over the recording, every recording >= 1
        row; means as verify takes them -> a dict of cuda tensors with the Wt windows of all recordings leading, recording r's at
        scan_window_offsets(frame_offsets, window_frames, hop_frames)[r : r + 2]: llr float32 [Wt][S], ll_ubm float32 [Wt], ll_target
        float32 [Wt][S], best int32 [Wt], best_llr float32 [Wt].  Each equals verify on the window's rows as a clip, bit for bit."""
        cfg = _scan_config(window_frames, hop_frames)
        feats, fo, means, want = self._inputs(feats, frame_offsets, means, want, "recording")
        nw, n_spk = int(scan_window_offsets(fo, window_frames, hop_frames)[-1]), means.shape[0]
        out, ptrs = self._outputs(nw, n_spk, want, feats.device)
        _lib.check(self._L.dsp_speaker_float_scan_device(self._h, feats.data_ptr(), fo.size - 1, fo.ctypes.data_as(_lib.LP), C.byref(cfg), means.data_ptr(),
                                                         n_spk, *ptrs, _lib.current_stream(feats)), "dsp_speaker_float_scan_device")
        return out


def _segment_config(on, off, min_windows, max_gap, exclusive):
    on = float(on)
    off = on if off is None else float(off)
    min_windows, max_gap = int(min_windows), int(max_gap)
    if on != on or off != off or off > on:
        raise ValueError("on and off must not be NaN, and off <= on")
    if min_windows < 1 or max_gap < 0:
        raise ValueError("min_windows must be >= 1 and max_gap >= 0")
    return _lib.SegmentConfig(on, off, min_windows, max_gap, _lib.SEG_EXCLUSIVE if exclusive else _lib.SEG_INDEPENDENT)


def segments_capacity(window_offsets, n_columns: int = 1, min_windows: int = 1, max_gap: int = 0) -> int:
    """Host only: the most segments Segmenter.segments can find (dsp_segments_capacity): n_columns times the sum over recordings of
    (W_r + max_gap + 1) // (min_windows + max_gap + 1)."""
    cfg = _segment_config(0.0, 0.0, min_windows, max_gap, False)
    wo = _lib.offsets_array(window_offsets, "window_offsets", "windows")
    return _lib.check(_lib.load().dsp_segments_capacity(C.byref(cfg), wo.ctypes.data_as(_lib.LP), wo.size - 1, int(n_columns)), "dsp_segments_capacity")


def segment_sample_spans(cfg, offsets, segments, window_frames: int, hop_frames: int):
    """Host only: (starts, lengths) int64 [n_segments], each segment in samples from its first window's start to its last window's end
    (dsp_segment_sample_spans): cfg the MfccConfig of the plan that made the rows, offsets the recordings' sample offsets, segments
    what Segmenter.segments returned (the numpy records)."""
    scan = _scan_config(window_frames, hop_frames)
    off, n = offsets if isinstance(offsets, tuple) else _lib.c_offsets(offsets)
    segs = np.ascontiguousarray(segments, dtype=np.dtype(_lib.SEGMENT_DTYPE))
    starts, lengths = np.zeros(segs.size, np.int64), np.zeros(segs.size, np.int64)
    _lib.check(_lib.load().dsp_segment_sample_spans(C.byref(cfg), C.byref(scan), off, n, segs.ctypes.data, segs.size, starts.ctypes.data_as(_lib.LP),
                                                    lengths.ctypes.data_as(_lib.LP)), "dsp_segment_sample_spans")
    return starts, lengths


class _Stage:
    """The constructor of a stage on a score matrix, a Handle that `_make`(device) creates (a mix-in in front of lib.Handle, which
    stays the base of the classes that own a native handle).  No device is touched before the first call that launches."""

    _make = None

    def __init__(self, device: int = 0):
        self._create(self._make, int(device))
        self.device = int(device)


def _truth(truth, n_rows, n_col):
    """truth as a contiguous C int array: one column index (or -1) per row of scores, or ValueError"""
    tr = np.ascontiguousarray(np.asarray(truth), dtype=np.intc)
    if tr.ndim != 1 or tr.size != n_rows:
        raise ValueError(f"truth must hold one column index (or -1) per row of scores: {n_rows}")
    bad = (tr < -1) | (tr >= n_col)
    if bad.any():
        raise ValueError(f"truth[{int(np.flatnonzero(bad)[0])}] is neither -1 nor a column")
    return tr


def _n_thresholds(n, name="n_thresholds"):
    n = int(n)
    if n < 2 or n > 1024:
        raise ValueError(f"{name} must be 2 .. 1024")
    return n


def _out_like(out, x, scores, verb):
    """where an apply writes: a new tensor like x (scores made contiguous), or the caller's `out`, which may be `scores` itself"""
    import torch
    if out is None:
        return torch.empty_like(x)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
            and out.device == x.device):
        raise ValueError("out must be a contiguous float32 CUDA tensor of the shape of scores, on their GPU")
    if out is scores and x is not scores:
        raise ValueError(f"scores must be contiguous to be {verb} in place")
    return out


class Segmenter(_Stage, _lib.Handle):
    """dsp_segmenter: segments from the window scores of any scan -- hysteresis between two thresholds, runs joined over short gaps,
    short segments dropped -- found on the GPU in (recording, column, first_window) order.  One stream at a time per segmenter."""

    _make, _destroy = "dsp_segmenter_create", "dsp_segmenter_destroy"
    CAP = 1 << 20          # segments the first call makes room for at most; a second call follows when more are found

    def segments(self, scores, window_offsets, on, off=None, min_windows: int = 1, max_gap: int = 0, exclusive: bool = False, as_tensor: bool = False):
        """scores: cuda float32 [Wt] or [Wt][S] (a scan's prob, prob1, decision or llr as it is), recording r = windows [window_offsets[r],
        window_offsets[r + 1]) (scan_window_offsets); a window with score >= on switches its track on, one with not (score >= off) off
        (off defaults to on); runs at most max_gap windows apart are joined, spans below min_windows dropped; exclusive: only the best
        column of a window counts -> numpy records (recording, column, first_window, n_windows, n_active, peak_window, peak, mean), or
        with as_tensor the same 32 bytes per segment as a cuda int32 [n][8] (peak and mean: .view(torch.float32) of columns 6 and 7)."""
        import torch
        cfg = _segment_config(on, off, min_windows, max_gap, exclusive)
        wo = _lib.offsets_array(window_offsets, "window_offsets", "windows")
        scores, n_col = _lib.scores_device(scores, self.device)
        if int(wo[-1]) > scores.shape[0]:
            raise ValueError("window_offsets run past the end of scores")
        dev, n = scores.device, wo.size - 1
        if n == 0 or wo[-1] == wo[0]:                       # (no window: nothing to launch, and an empty tensor has no address)
            out = torch.zeros((0, 8), dtype=torch.int32, device=dev)
            return out if as_tensor else np.zeros(0, np.dtype(_lib.SEGMENT_DTYPE))
        total = torch.zeros(2, dtype=torch.int64, device=dev)
        room = min(_lib.check(self._L.dsp_segments_capacity(C.byref(cfg), wo.ctypes.data_as(_lib.LP), n, n_col), "dsp_segments_capacity"), self.CAP)
        for _ in range(2):
            out = torch.empty((room, 8), dtype=torch.int32, device=dev)
            _lib.check(self._L.dsp_segments_device(self._h, scores.data_ptr(), n, wo.ctypes.data_as(_lib.LP), n_col, C.byref(cfg), out.data_ptr(), room, None,
                                                   total.data_ptr(), _lib.current_stream(scores)), "dsp_segments_device")
            found = int(total[0])
            if found <= room:
                break
            room = found
        out = out[:found]
        return out if as_tensor else out.cpu().numpy().view(np.dtype(_lib.SEGMENT_DTYPE)).reshape(-1)


class TrialEvaluator(_Stage, _lib.Handle):
    """dsp_trial_evaluator: labelled trials on the GPU -- per column of a score matrix and pooled, the reference's threshold sweep
    (evaluate_gmm.py:77-81), the exact ROC step curve as counts and the AUC (generate_charts.py:68-69).  One stream at a time per
    evaluator."""

    _make, _destroy = "dsp_trial_evaluator_create", "dsp_trial_evaluator_destroy"
    WANT = ("columns", "sweep", "roc")

    def evaluate(self, scores, truth, n_thresholds: int = 200, want=("columns", "sweep", "roc")):
        """scores: cuda float32 [T] or [T][S] (SpeakerVerifier.verify(...)["llr"] or .scan(...)["llr"] as it is); truth: T integers on
        the host, the column that is the row's true speaker or -1 -> a dict with n_thresholds and, as `want` names them,
          "columns": columns, numpy records [S + 1] (TRIAL_COLUMN_DTYPE), the last one pooled;
          "sweep":   sweep_tp, sweep_fp int64 [S + 1][n_thresholds] (the thresholds: trial_thresholds(lo, hi, n_thresholds));
          "roc":     target_offsets int64 [S + 1], target_rows int64 [targets], target_scores float32 [targets], fa_above and fa_equal
                     int32 [targets] (roc_points turns a column's into a curve).
        A matrix without rows is a ValueError here (there is nothing to return), where dsp_trials_evaluate_device answers DSP_OK and
        launches nothing."""
        import torch
        want = tuple(want)
        if not want or any(key not in self.WANT for key in want):
            raise ValueError(f"want must name at least one of {self.WANT}")
        n = _n_thresholds(n_thresholds)
        scores, n_col = _lib.scores_device(scores, self.device, "evaluator")
        n_rows = scores.shape[0]
        if n_rows < 1:
            raise ValueError("scores hold no trial")
        tr = _truth(truth, n_rows, n_col)
        tp = tr.ctypes.data_as(C.POINTER(C.c_int))
        dev, out, ptr = scores.device, {"n_thresholds": n}, {}
        if "columns" in want:
            cols = torch.empty((n_col + 1, 10), dtype=torch.int64, device=dev)
            ptr["columns"] = cols.data_ptr()
        if "sweep" in want:
            tps, fps = (torch.empty((n_col + 1, n), dtype=torch.int64, device=dev) for _ in range(2))
            ptr["tp"], ptr["fp"] = tps.data_ptr(), fps.data_ptr()
        if "roc" in want:
            offsets = np.zeros(n_col + 1, np.int64)
            n_tgt = _lib.check(self._L.dsp_trials_target_offsets(tp, n_rows, n_col, offsets.ctypes.data_as(_lib.LP), None), "dsp_trials_target_offsets")
            rows = np.zeros(n_tgt, np.int64)
            _lib.check(self._L.dsp_trials_target_offsets(tp, n_rows, n_col, None, rows.ctypes.data_as(_lib.LP)), "dsp_trials_target_offsets")
            above, equal = (torch.empty(max(n_tgt, 1), dtype=torch.int32, device=dev) for _ in range(2))   # (an empty tensor has no address)
            ptr["above"], ptr["equal"] = above.data_ptr(), equal.data_ptr()
        cfg = _lib.TrialsConfig(n)
        _lib.check(self._L.dsp_trials_evaluate_device(self._h, scores.data_ptr(), n_rows, n_col, tp, C.byref(cfg),
                                                      *[ptr.get(key) for key in ("columns", "tp", "fp", "above", "equal")], _lib.current_stream(scores)),
                   "dsp_trials_evaluate_device")
        if "columns" in want:
            out["columns"] = cols.cpu().numpy().view(np.dtype(_lib.TRIAL_COLUMN_DTYPE)).reshape(-1)
        if "sweep" in want:
            out["sweep_tp"], out["sweep_fp"] = tps.cpu().numpy(), fps.cpu().numpy()
        if "roc" in want:
            flat = scores.reshape(n_rows, n_col)
            at = torch.from_numpy(rows).to(dev)
            out.update(target_offsets=offsets, target_rows=rows, fa_above=above[:n_tgt].cpu().numpy(), fa_equal=equal[:n_tgt].cpu().numpy(),
                       target_scores=flat[at, torch.from_numpy(tr[rows].astype(np.int64)).to(dev)].cpu().numpy())
        return out


def trial_thresholds(lo, hi, n: int) -> np.ndarray:
    """Host only: the n thresholds of the sweep between a column's lo and hi, float64 -- np.linspace(lo, hi, n) as
    evaluate_gmm.py:77 calls it: i * ((hi - lo) / (n - 1)) + lo in two roundings, the last one hi itself."""
    n = _n_thresholds(n, "n")
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(invalid="ignore"):
        t = np.arange(n, dtype=np.float64) * ((hi - lo) / np.float64(n - 1)) + lo
    t[-1] = hi
    return t


def roc_points(result: dict, column: int):
    """Host only: (fpr, tpr, thresholds) of one column from TrialEvaluator.evaluate(..., want=("columns", "roc")), laid out as
    sklearn.metrics.roc_curve(labels, scores, drop_intermediate=False) returns them -- thresholds descending from inf, the point (0, 0)
    first, "accept when x >= threshold" -- with the corners of the exact step curve only.  Every distinct target score v gives the
    point (above + equal, targets >= v) at threshold v, and where non-targets lie between v and the target score before it, the
    corner (above, targets > v) in front of it, at the float32 next above v ("accept when x > v").  sklearn's further points, at
    scores that only non-targets have, lie on the horizontal stretches between these and carry no area.  Where the last point is not
    (1, 1) already, (1, 1) at -inf closes the curve.  A column without targets or without non-targets has rates of NaN, as sklearn's."""
    for key in ("columns", "target_offsets", "fa_above", "fa_equal", "target_scores"):
        if key not in result:
            raise ValueError('roc_points needs a result of want=("columns", "roc")')
    column = int(column)
    if column < 0 or column >= result["target_offsets"].size - 1:
        raise ValueError("no such column")
    a, b = (int(v) for v in result["target_offsets"][column:column + 2])
    x, above, equal = result["target_scores"][a:b], result["fa_above"][a:b].astype(np.int64), result["fa_equal"][a:b].astype(np.int64)
    keep = x == x
    x, above, equal = x[keep].astype(np.float32), above[keep], equal[keep]
    n_tgt, n_non = int(result["columns"]["n_target"][column]), int(result["columns"]["n_nontarget"][column])
    neg, first, count = np.unique(-x.astype(np.float64), return_index=True, return_counts=True)      # descending scores
    tps, fps, thr = [0], [0], [np.inf]
    for v, j, c in zip(-neg, first, count):
        if above[j] > fps[-1]:
            tps, fps, thr = tps + [tps[-1]], fps + [int(above[j])], thr + [float(np.nextafter(np.float32(v), np.float32(np.inf)))]
        tps, fps, thr = tps + [tps[-1] + int(c)], fps + [int(above[j] + equal[j])], thr + [float(v)]
    if fps[-1] < n_non or len(thr) == 1:
        tps, fps, thr = tps + [n_tgt], fps + [n_non], thr + [-np.inf]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array(fps, np.float64) / np.float64(n_non), np.array(tps, np.float64) / np.float64(n_tgt), np.array(thr, np.float64)


class ScoreCalibrator(_Stage, _lib.Handle):
    """dsp_calibrator: c = A x + B + C log(n_frames) on a score matrix on the GPU -- fit by prior-weighted logistic regression (damped
    Newton, every pass and solve on the device) on labelled trials, and apply.  One stream at a time per calibrator."""

    _make, _destroy = "dsp_calibrator_create", "dsp_calibrator_destroy"

    @staticmethod
    def duration_term(n_frames) -> np.ndarray:
        """Host only: log(n_frames + 1e-8) as float64, exactly the values fit and apply use (dsp_calibration_duration_term)."""
        nf = _frames(n_frames, None)
        out = np.empty(nf.size, np.float64)
        _lib.check(_lib.load().dsp_calibration_duration_term(nf.ctypes.data_as(_lib.LP), nf.size, out.ctypes.data_as(C.POINTER(C.c_double))),
                   "dsp_calibration_duration_term")
        return out

    def fit(self, scores, truth, n_frames=None, prior: float = 0.5, tol: float = 1e-10, max_iter: int = 100, init=None) -> dict:
        """scores: cuda float32 [T] or [T][S]; truth: T integers on the host, the row's true column or -1; n_frames: T frame counts on
        the host, or None for the two-parameter model (C stays 0); init: (a, b, c) or a dict with those keys, None: 1, 0, 0 -> the
        report as a dict: a, b, c, params = (a, b, c), n_target, n_nontarget, n_excluded, objective_start, objective, last_step,
        n_iter, n_rejected, status (lib.CAL_*) and status_name.  Waits for the stream once."""
        if not (0.0 < float(prior) < 1.0):
            raise ValueError("prior must lie inside (0, 1)")
        if not float(tol) > 0.0:
            raise ValueError("tol must be > 0")
        if int(max_iter) < 1 or int(max_iter) > 10000:
            raise ValueError("max_iter must be 1 .. 10000")
        scores, n_col = _lib.scores_device(scores, self.device, "calibrator")
        n_rows = scores.shape[0]
        if n_rows < 1:
            raise ValueError("scores hold no trial")
        tr = _truth(truth, n_rows, n_col)
        nf = _frames(n_frames, n_rows)
        start = _calibration(init, nf is not None)
        cfg, rep = _lib.CalibrationConfig(float(prior), float(tol), int(max_iter), 0), _lib.CalibrationReport()
        _lib.check(self._L.dsp_calibration_fit_device(self._h, scores.data_ptr(), n_rows, n_col, tr.ctypes.data_as(C.POINTER(C.c_int)),
                                                      nf.ctypes.data_as(_lib.LP) if nf is not None else None, C.byref(cfg), C.byref(start), C.byref(rep),
                                                      _lib.current_stream(scores)), "dsp_calibration_fit_device")
        out = {name: getattr(rep, name) for name, _ in _lib.CalibrationReport._fields_ if name not in ("params", "reserved")}
        out.update(a=rep.params.a, b=rep.params.b, c=rep.params.c, params=(rep.params.a, rep.params.b, rep.params.c),
                   status_name=_lib.CAL_STATUS[rep.status])
        return out

    def apply(self, scores, params, n_frames=None, out=None):
        """scores: cuda float32 [T] or [T][S]; params: (a, b, c) or what fit returned; n_frames as in fit (None needs c == 0) -> the
        calibrated scores, float32 of the same shape: a new tensor, or `out` (which may be `scores` itself).  Only enqueues."""
        x, n_col = _lib.scores_device(scores, self.device, "calibrator")
        n_rows = x.shape[0]
        nf = _frames(n_frames, n_rows)
        p = _calibration(params, nf is not None)
        out = _out_like(out, x, scores, "calibrated")
        if n_rows:
            _lib.check(self._L.dsp_calibration_apply_device(self._h, x.data_ptr(), n_rows, n_col, nf.ctypes.data_as(_lib.LP) if nf is not None else None,
                                                            C.byref(p), out.data_ptr(), _lib.current_stream(x)), "dsp_calibration_apply_device")
        return out


def _frames(n_frames, n_rows):
    """n_frames as a contiguous int64 array (None stays None), or ValueError"""
    if n_frames is None:
        return None
    nf = np.ascontiguousarray(np.asarray(n_frames), dtype=np.int64)
    if nf.ndim != 1 or (n_rows is not None and nf.size != n_rows):
        raise ValueError("n_frames must hold one frame count per row of scores")
    if (nf < 0).any():
        raise ValueError(f"n_frames[{int(np.flatnonzero(nf < 0)[0])}] is negative")
    return nf


def _calibration(params, with_frames: bool):
    """(a, b, c), a dict with those keys (what ScoreCalibrator.fit returned) or None (1, 0, 0) -> lib.Calibration, or ValueError"""
    if params is None:
        a, b, c = 1.0, 0.0, 0.0
    elif isinstance(params, dict):
        a, b, c = (float(params[key]) for key in ("a", "b", "c"))
    else:
        a, b, c = (float(v) for v in params)
    if not all(np.isfinite(v) for v in (a, b, c)):
        raise ValueError("the calibration's parameters must be finite")
    if c != 0.0 and not with_frames:
        raise ValueError("c != 0 needs n_frames")
    return _lib.Calibration(a, b, c)


class ScoreNormalizer(_lib.Closing):
    """Z-, T- and S-norm of a score matrix against cohorts on one GPU (dsp_cohort_stats_device, dsp_score_normalize_device), and
    their adaptive forms that keep the top_k closest cohort members.  A statistic per row of a [T][N] cohort (clips against cohort
    speakers) and per column of an [M][S] cohort (cohort clips against the enrolled speakers), then the apply.  The reference has no
    such step.  Keeping a speaker's own clips out of the cohort is the caller's job.  The library keeps no state between calls, so
    there is no native handle: the object holds the device index, and close() (or `with`) ends its use.  One stream at a time per
    normaliser."""

    AXES = {"row": _lib.COHORT_PER_ROW, "column": _lib.COHORT_PER_COLUMN}

    def __init__(self, device: int = 0):
        if int(device) < 0:
            raise ValueError("device index out of range")
        self._L = _lib.load()
        self.device = int(device)

    def close(self):
        self._L = None

    def _lib_or_closed(self):
        if self._L is None:
            raise _lib.DspError("the ScoreNormalizer is closed")
        return self._L

    def _matrix(self, x, what):
        """a float32 CUDA matrix [R][C] on the normaliser's GPU, made contiguous, or ValueError"""
        import torch
        if not (isinstance(x, torch.Tensor) and x.dim() == 2):
            raise ValueError(f"{what} must be a float32 CUDA tensor [rows][columns]")
        return _lib.scores_device(x, self.device, "normalizer")[0]

    def _records(self, stats, size, what):
        """the records stats() returned: a contiguous int64 CUDA tensor [size][4] on the normaliser's GPU, or ValueError"""
        import torch
        if not (isinstance(stats, torch.Tensor) and stats.is_cuda and stats.dtype == torch.int64 and stats.shape == (size, 4) and stats.is_contiguous()):
            raise ValueError(f"{what} must be what stats() returned for {size} vectors: a contiguous int64 CUDA tensor [{size}][4]")
        if stats.device.index != self.device:
            raise ValueError(f"{what} are on GPU {stats.device.index}, the normalizer on GPU {self.device}")
        return stats

    def stats(self, cohort, axis, top_k: int = 0):
        """cohort: cuda float32 [R][C]; axis "row" (R records, each over the C values of a row) or "column" (C records, each over the R
        values of a column, read where they lie); top_k: the closest (largest) cohort members kept, 0 for all -> the records, an int64
        CUDA tensor [vectors][4] of 32-byte dsp_cohort_stat (stats_to_numpy reads it).  Only enqueues."""
        import torch
        L = self._lib_or_closed()
        if axis not in self.AXES:
            raise ValueError('axis must be "row" or "column"')
        k = int(top_k)
        if k < 0 or k > _lib.COHORT_MAX_TOP_K:
            raise ValueError("top_k must be 0 .. 2^22")
        x = self._matrix(cohort, "cohort")
        vectors, length = (x.shape[0], x.shape[1]) if axis == "row" else (x.shape[1], x.shape[0])
        if length < 1 or length > _lib.COHORT_MAX_LENGTH:
            raise ValueError("a cohort must hold 1 .. 2^22 values per vector")
        out = torch.empty((vectors, 4), dtype=torch.int64, device=x.device)
        if vectors:
            _lib.check(L.dsp_cohort_stats_device(self.device, x.data_ptr(), x.shape[0], x.shape[1], self.AXES[axis], k, out.data_ptr(),
                                                       _lib.current_stream(x)), "dsp_cohort_stats_device")
        return out

    @staticmethod
    def stats_to_numpy(stats) -> dict:
        """the records of stats() on the host: a dict of numpy arrays mean, std (float64), threshold (float32), n_finite, n_selected,
        n_above (int32), one entry per vector.  Waits for the stream."""
        rec = stats.cpu().numpy().view(np.dtype(_lib.COHORT_STAT_DTYPE)).reshape(-1)
        return {name: rec[name].copy() for name in rec.dtype.names}

    def apply(self, scores, mode, row_stats=None, col_stats=None, std_floor: float = 1e-6, out=None):
        """scores: cuda float32 [T][S]; mode "z" (needs col_stats [S]), "t" (needs row_stats [T]) or "s" (both); std_floor: the least
        sigma a score is divided by -> the normalised scores, float32 [T][S]: a new tensor, or `out` (which may be `scores` itself).
        Only enqueues."""
        L = self._lib_or_closed()
        if mode not in _lib.NORM_MODES:
            raise ValueError('mode must be "z", "t" or "s"')
        floor = float(std_floor)
        if not (np.isfinite(floor) and floor >= 0.0):
            raise ValueError("std_floor must be finite and >= 0")
        x = self._matrix(scores, "scores")
        n_rows, n_col = x.shape
        if mode != "z" and row_stats is None:
            raise ValueError(f'mode "{mode}" needs row_stats')
        if mode != "t" and col_stats is None:
            raise ValueError(f'mode "{mode}" needs col_stats')
        row = self._records(row_stats, n_rows, "row_stats") if mode != "z" else None
        col = self._records(col_stats, n_col, "col_stats") if mode != "t" else None
        out = _out_like(out, x, scores, "normalised")
        if n_rows and n_col:
            cfg = _lib.SnormConfig(_lib.NORM_MODES[mode], 0, floor)
            _lib.check(L.dsp_score_normalize_device(self.device, x.data_ptr(), n_rows, n_col, row.data_ptr() if row is not None else None,
                                                          col.data_ptr() if col is not None else None, C.byref(cfg), out.data_ptr(),
                                                          _lib.current_stream(x)), "dsp_score_normalize_device")
        return out

    def normalize(self, scores, row_cohort=None, col_cohort=None, mode="s", top_k: int = 0, std_floor: float = 1e-6):
        """scores: cuda float32 [T][S]; row_cohort [T][N], the trial clips against N cohort speakers (modes "t" and "s"); col_cohort
        [M][S], M cohort clips against the enrolled speakers (modes "z" and "s") -> the normalised scores, a new tensor.  Only
        enqueues."""
        self._lib_or_closed()
        if mode not in _lib.NORM_MODES:
            raise ValueError('mode must be "z", "t" or "s"')
        x = self._matrix(scores, "scores")
        row = col = None
        if mode != "z":
            if row_cohort is None:
                raise ValueError(f'mode "{mode}" needs row_cohort')
            rc = self._matrix(row_cohort, "row_cohort")
            if rc.shape[0] != x.shape[0]:
                raise ValueError(f"row_cohort must hold one row per row of scores: {x.shape[0]}")
        if mode != "t":
            if col_cohort is None:
                raise ValueError(f'mode "{mode}" needs col_cohort')
            cc = self._matrix(col_cohort, "col_cohort")
            if cc.shape[1] != x.shape[1]:
                raise ValueError(f"col_cohort must hold one column per column of scores: {x.shape[1]}")
        if mode != "z":
            row = self.stats(rc, "row", top_k)
        if mode != "t":
            col = self.stats(cc, "column", top_k)
        return self.apply(x, mode, row, col, std_floor)


class Vad(_lib.Closing):
    """Voice activity detection between the front end and the models (dsp_vad_*, dsp_rows_*): float64 frame power of the rows of an
    MFCC plan, an energy threshold against each clip's own level (librosa's top_db with ref = np.max, or the mean, or an absolute
    power), Kaldi's smoothing over context_frames, a hangover of pad_frames, and the selection of the kept rows of any matrix.  The
    reference has no such step.  The library keeps nothing between calls, so there is no native handle: the object holds the
    configuration and a grow-only workspace tensor on its GPU, and close() (or `with`) lets that go.  One stream at a time per Vad."""

    _ws = None

    def __init__(self, plan_or_cfg, reference="max", threshold_db: float = -60.0, floor_db: float = float("-inf"), context_frames: int = 0,
                 proportion: float = 0.6, pad_frames: int = 0, device: int = 0):
        """plan_or_cfg: the MfccPlan (or its MfccConfig) whose rows are to be filtered: frame_length, hop_length and framing are taken
        from it.  threshold_db is relative to the reference ("max", "mean") or to power 1 ("absolute"); floor_db is an absolute power
        below which nothing is speech."""
        mfcc = getattr(plan_or_cfg, "cfg", plan_or_cfg)
        if not isinstance(mfcc, _lib.MfccConfig):
            raise ValueError("plan_or_cfg must be an MfccPlan or an MfccConfig")
        if reference not in _lib.VAD_REFERENCES:
            raise ValueError('reference must be "absolute", "max" or "mean"')
        if int(device) < 0:
            raise ValueError("device index out of range")
        threshold_db, floor_db, proportion = float(threshold_db), float(floor_db), float(proportion)
        if np.isnan(threshold_db) or threshold_db == float("inf") or np.isnan(floor_db):
            raise ValueError("threshold_db must be below +inf and floor_db must not be NaN")
        if not (0 <= int(context_frames) <= 64 and 0 <= int(pad_frames) <= 64):
            raise ValueError("context_frames and pad_frames must be 0 .. 64")
        if not 0.0 < proportion <= 1.0:
            raise ValueError("proportion must lie in (0, 1]")
        self._L = _lib.load()
        self.device = int(device)
        self.cfg = _lib.VadConfig()
        self._L.dsp_vad_default_config(C.byref(mfcc), C.byref(self.cfg))
        self.cfg.reference = _lib.VAD_REFERENCES[reference]
        self.cfg.threshold_ratio = self._L.dsp_vad_ratio_from_db(threshold_db)
        self.cfg.floor_power = self._L.dsp_vad_ratio_from_db(floor_db)
        self.cfg.context_frames, self.cfg.proportion, self.cfg.pad_frames = int(context_frames), proportion, int(pad_frames)
        geo = _lib.VadGeometry()
        rc = self._L.dsp_vad_geometry_for(C.byref(self.cfg), C.byref(geo))
        if rc < 0:
            raise ValueError(_lib.last_error())
        self.geometry = {name: getattr(geo, name) for name, _ in _lib.VadGeometry._fields_}

    def close(self):
        self._L = self._ws = None

    def _lib_or_closed(self):
        if self._L is None:
            raise _lib.DspError("the Vad is closed")
        return self._L

    def _workspace(self, n_clips, n_rows):
        """(pointer, bytes) of the workspace, grown to what n_clips clips of n_rows rows need"""
        import torch
        need = _lib.check(self._L.dsp_vad_workspace_bytes(n_clips, n_rows), "dsp_vad_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + need // 2, dtype=torch.uint8, device=f"cuda:{self.device}")
        return self._ws.data_ptr(), self._ws.numel()

    def _on_device(self, x, what, dtype, dims=(1,)):
        import torch
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.dim() in dims):
            raise ValueError(f"{what} must be a {str(dtype).replace('torch.', '')} CUDA tensor")
        if x.device.index != self.device:
            raise ValueError(f"{what} is on GPU {x.device.index}, the Vad on GPU {self.device}")
        return x.contiguous()

    def _signal(self, signal, offsets, frame_offsets):
        import torch
        signal = self._on_device(signal, "signal", torch.float32)
        off, n, _, _ = _lib.ragged_signal(signal, offsets, torch.float32)
        fo = _frame_offsets(frame_offsets)
        if fo.size != n + 1:
            raise ValueError("frame_offsets must hold one entry more than there are clips")
        return signal, off, n, fo

    def power(self, signal, offsets, frame_offsets):
        """signal: cuda float32 [total], clip c = samples [offsets[c], offsets[c + 1]) and rows [frame_offsets[c], frame_offsets[c + 1]) ->
        cuda float64 [frame_offsets[-1]]: the mean square of each row's frame (rows of no clip are zeros).  Only enqueues."""
        import torch
        L = self._lib_or_closed()
        signal, off, n, fo = self._signal(signal, offsets, frame_offsets)
        out = torch.zeros(int(fo[-1]), dtype=torch.float64, device=signal.device)
        if n and fo[-1] > fo[0]:
            ws, ws_bytes = self._workspace(n, int(fo[-1] - fo[0]))
            _lib.check(L.dsp_vad_frame_power_ragged_device(self.device, C.byref(self.cfg), signal.data_ptr(), n, off, fo.ctypes.data_as(_lib.LP), out.data_ptr(),
                                                           ws, ws_bytes, _lib.current_stream(signal)), "dsp_vad_frame_power_ragged_device")
        return out

    def _decide(self, entry, name, where, n, fo, levels, *front):
        import torch
        R = int(fo[-1])
        flags = torch.zeros(R, dtype=torch.uint8, device=where.device)
        level = torch.zeros(R, dtype=torch.float32, device=where.device) if levels else None
        clips = torch.zeros((n, 4), dtype=torch.int64, device=where.device)
        kept = np.zeros(n + 1, np.int64)
        if n and fo[-1] > fo[0]:
            ws, ws_bytes = self._workspace(n, int(fo[-1] - fo[0]))
            _lib.check(entry(self.device, C.byref(self.cfg), *front, fo.ctypes.data_as(_lib.LP), flags.data_ptr(), level.data_ptr() if levels else None,
                             clips.data_ptr(), kept.ctypes.data_as(_lib.LP), ws, ws_bytes, _lib.current_stream(where)), name)
        records = clips.cpu().numpy().view(np.dtype(_lib.VAD_CLIP_DTYPE)).reshape(-1)
        if not (n and fo[-1] > fo[0]):                      # no row, no launch: the records of clips without rows
            scaled = float(self.cfg.reference == _lib.VAD_REF_ABSOLUTE) * self.cfg.threshold_ratio
            records["reference"] = float(self.cfg.reference == _lib.VAD_REF_ABSOLUTE)
            records["threshold"] = scaled if scaled >= self.cfg.floor_power else self.cfg.floor_power
            records["first_kept"] = records["last_kept"] = -1
        return (flags, kept, records, level) if levels else (flags, kept, records)

    def decide(self, power, frame_offsets, levels: bool = False):
        """power: cuda float64 [R] as power() returns it -> (flags, kept_offsets, records[, level_db]): flags cuda uint8 [R], 1 = speech;
        kept_offsets numpy int64 [n_clips + 1], the prefix sums of the kept rows; records numpy (reference, threshold, n_raw, n_kept,
        first_kept, last_kept) per clip; level_db cuda float32 [R] = 10 log10(P / threshold), a score track for Segmenter.  Waits for
        the stream once."""
        import torch
        L = self._lib_or_closed()
        power = self._on_device(power, "power", torch.float64)
        fo = _frame_offsets(frame_offsets)
        if int(fo[-1]) > power.shape[0]:
            raise ValueError("frame_offsets run past the end of power")
        n = fo.size - 1
        return self._decide(L.dsp_vad_decide_ragged_device, "dsp_vad_decide_ragged_device", power, n, fo, levels, power.data_ptr(), n)

    def run(self, signal, offsets, frame_offsets, levels: bool = False):
        """power() and decide() in one call, the power kept in the workspace -> what decide() returns."""
        L = self._lib_or_closed()
        signal, off, n, fo = self._signal(signal, offsets, frame_offsets)
        return self._decide(L.dsp_vad_run_ragged_device, "dsp_vad_run_ragged_device", signal, n, fo, levels, signal.data_ptr(), n, off)

    def kept_offsets(self, flags, frame_offsets) -> np.ndarray:
        """flags from any source, cuda uint8 [R] -> numpy int64 [n_clips + 1]: the prefix sums of each clip's non-zero flags
        (dsp_rows_kept_offsets_device).  Waits for the stream once."""
        import torch
        L = self._lib_or_closed()
        flags = self._on_device(flags, "flags", torch.uint8)
        fo = _frame_offsets(frame_offsets)
        if int(fo[-1]) > flags.shape[0]:
            raise ValueError("frame_offsets run past the end of flags")
        n = fo.size - 1
        kept = np.zeros(n + 1, np.int64)
        if n and fo[-1] > fo[0]:
            ws, ws_bytes = self._workspace(n, int(fo[-1] - fo[0]))
            _lib.check(L.dsp_rows_kept_offsets_device(self.device, flags.data_ptr(), n, fo.ctypes.data_as(_lib.LP), kept.ctypes.data_as(_lib.LP), ws, ws_bytes,
                                                      _lib.current_stream(flags)), "dsp_rows_kept_offsets_device")
        return kept

    def select(self, x, flags, frame_offsets, kept_offsets, index: bool = False):
        """x: cuda float32 [R][d] (d 1 .. 64) or [R]; flags cuda uint8 [R]; kept_offsets as decide(), run() or kept_offsets() gave them ->
        the rows whose flag is set, in order: a new cuda float32 [kept_offsets[-1]][d] (or [kept]), and with index their original row
        numbers as a cuda int64 [kept].  Only enqueues."""
        import torch
        L = self._lib_or_closed()
        x = self._on_device(x, "x", torch.float32, (1, 2))
        flags = self._on_device(flags, "flags", torch.uint8)
        fo = _frame_offsets(frame_offsets)
        ko = _lib.long_array(kept_offsets, fo.size, "kept_offsets")
        d = x.shape[1] if x.dim() == 2 else 1
        if not 1 <= d <= 64:
            raise ValueError("x must have 1 .. 64 columns")
        if int(fo[-1]) > min(x.shape[0], flags.shape[0]):
            raise ValueError("frame_offsets run past the end of x or flags")
        n, kept = fo.size - 1, int(ko[-1]) if fo.size > 1 else 0
        out = torch.zeros((kept, d) if x.dim() == 2 else (kept,), dtype=torch.float32, device=x.device)
        rows = torch.zeros(kept, dtype=torch.int64, device=x.device) if index else None
        if n and fo[-1] > fo[0]:
            ws, ws_bytes = self._workspace(n, int(fo[-1] - fo[0]))
            _lib.check(L.dsp_rows_select_ragged_device(self.device, x.data_ptr(), d, flags.data_ptr(), n, fo.ctypes.data_as(_lib.LP), ko.ctypes.data_as(_lib.LP),
                                                       out.data_ptr() if kept else None, rows.data_ptr() if index and kept else None, ws, ws_bytes,
                                                       _lib.current_stream(x)), "dsp_rows_select_ragged_device")
        return (out, rows) if index else out

    def trim_spans(self, records, offsets):
        """Host only, librosa's trim: records as decide() or run() returned them, offsets the clips' sample offsets -> (starts, lengths,
        n): clip c cut to its first and last kept row, starts absolute, length 0 where nothing is kept; n clips keep something."""
        L = self._lib_or_closed()
        off, n = _lib.c_offsets(offsets)
        rec = np.ascontiguousarray(records, np.dtype(_lib.VAD_CLIP_DTYPE))
        if rec.shape != (n,):
            raise ValueError(f"records must hold one entry per clip: {n}")
        starts, lengths = np.zeros(n, np.int64), np.zeros(n, np.int64)
        kept = _lib.check(L.dsp_vad_trim_spans(C.byref(self.cfg), off, n, rec.ctypes.data, starts.ctypes.data_as(_lib.LP), lengths.ctypes.data_as(_lib.LP)),
                          "dsp_vad_trim_spans")
        return starts, lengths, kept


class UbmTrainer(_lib.Handle):
    """dsp_ubm_trainer: EM for a diagonal GMM of k components on a matrix of (CMVN'd) feature rows [n][d] -- sklearn's M-step and stopping
    rule; the float UBM SpeakerEnroller takes, and through quantize_gmm the integer tables SpeakerModel takes."""

    _destroy = "dsp_ubm_trainer_destroy"

    def __init__(self, k: int, d: int, device: int = 0):
        k, d = int(k), int(d)
        if not (1 <= k <= 64 and 1 <= d <= 16):
            raise ValueError("k must be 1 .. 64 and d 1 .. 16")
        self._create("dsp_ubm_trainer_create", int(device), k, d)
        self.k, self.d, self.device = k, d, int(device)

    def _rows(self, feats):
        import torch
        if not (hasattr(feats, "is_cuda") and feats.is_cuda and feats.dim() == 2 and feats.shape[1] == self.d and feats.dtype == torch.float32):
            raise ValueError(f"feats must be a float32 CUDA tensor [n][{self.d}]")
        if feats.shape[0] < self.k:
            raise ValueError(f"feats must hold at least k = {self.k} rows")
        return feats.contiguous()

    @staticmethod
    def _reg_covar(reg_covar):
        reg_covar = float(reg_covar)
        if not (0.0 <= reg_covar < float("inf")):
            raise ValueError("reg_covar must be >= 0 and finite")
        return reg_covar

    def init_rows(self, feats, reg_covar: float = 1e-6) -> dict:
        """The library's deterministic start on feats (cuda float32 [n][d]): means = rows floor((i + 0.5) n / k), variances = the rows'
        global variance per dimension + reg_covar, weights 1 / k -> dict of float64 arrays weights [k], means [k][d], variances [k][d]."""
        reg_covar = self._reg_covar(reg_covar)
        feats = self._rows(feats)
        out = {"weights": np.empty(self.k), "means": np.empty((self.k, self.d)), "variances": np.empty((self.k, self.d))}
        _lib.check(self._L.dsp_ubm_init_rows_device(self._h, feats.data_ptr(), feats.shape[0], reg_covar,
                                                    *[out[key].ctypes.data for key in ("weights", "means", "variances")], _lib.current_stream(feats)),
                   "dsp_ubm_init_rows_device")
        return out

    def kmeans_seed(self, feats, seed: int = 0) -> np.ndarray:
        """Greedy k-means++ on feats (cuda float32 [n][d]), deterministic from the 64-bit seed (the draws are defined in include/dsp_amd.h)
        -> int64 [k], the chosen rows in the order chosen.  DspError when feats holds fewer than k distinct rows."""
        seed = self._seed(seed)
        feats = self._rows(feats)
        rows = np.empty(self.k, np.int64)
        _lib.check(self._L.dsp_kmeans_seed_device(self._h, feats.data_ptr(), feats.shape[0], seed, rows.ctypes.data, _lib.current_stream(feats)), "dsp_kmeans_seed_device")
        return rows

    @staticmethod
    def _seed(seed):
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be in [0, 2^64)")
        return seed

    @staticmethod
    def _kmeans_numbers(max_iter, tol):
        max_iter, tol = int(max_iter), float(tol)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        if not (0.0 <= tol < float("inf")):
            raise ValueError("tol must be >= 0 and finite")
        return max_iter, tol

    def kmeans(self, feats, centres, max_iter: int = 300, tol: float = 1e-4, reg_covar: float = 1e-6, want_labels: bool = False) -> dict:
        """Lloyd on feats (cuda float32 [n][d]) from centres [k][d] (sklearn's stop rules; an empty cluster keeps its centre) and the GMM of
        the final labels -> dict: centres [k][d], counts [k], inertia, n_iter, stop ("max_iter" / "tol" / "strict"), n_empty, the GMM start
        weights [k], means, variances [k][d] (fit's init as it is), and with want_labels the labels (cuda int32 [n])."""
        import torch
        max_iter, tol = self._kmeans_numbers(max_iter, tol)
        reg_covar = self._reg_covar(reg_covar)
        k, d = self.k, self.d
        start = np.ascontiguousarray(centres, np.float64)
        if start.shape != (k, d):
            raise ValueError(f"centres must be [{k}][{d}]")
        if not np.isfinite(start).all():
            raise ValueError("centres must be finite")
        feats = self._rows(feats)
        out = {"centres": np.empty((k, d)), "counts": np.empty(k, np.int64), "weights": np.empty(k), "means": np.empty((k, d)), "variances": np.empty((k, d))}
        labels = torch.empty(feats.shape[0], dtype=torch.int32, device=feats.device) if want_labels else None
        res = _lib.KmeansResult(*[out[key].ctypes.data for key in ("centres", "counts", "weights", "means", "variances")],
                                labels.data_ptr() if want_labels else None)
        cfg = _lib.KmeansConfig(max_iter, tol, reg_covar)
        _lib.check(self._L.dsp_kmeans_fit_device(self._h, feats.data_ptr(), feats.shape[0], start.ctypes.data, C.byref(cfg), C.byref(res), _lib.current_stream(feats)),
                   "dsp_kmeans_fit_device")
        out.update(inertia=float(res.inertia), n_iter=int(res.n_iter), stop=_lib.KMEANS_STOP[res.stop], n_empty=int(res.n_empty))
        if want_labels:
            out["labels"] = labels
        return out

    def fit(self, feats, init: dict | str | None = None, max_iter: int = 300, tol: float = 1e-3, reg_covar: float = 1e-6, n_init: int = 1, seed: int = 0,
            kmeans_max_iter: int = 300, kmeans_tol: float = 1e-4) -> dict:
        """EM on feats (cuda float32 [n][d], n >= k) from init (weights [k], means [k][d], variances [k][d]; None: init_rows) until the
        lower bound changes by less than tol or max_iter iterations -> dict of float64 arrays weights [k], means, variances, inv_covs [k][d],
        log_consts [k], lower_bounds [n_iter], and n_iter, converged.  The dict is a SpeakerEnroller's ubm_float as it is.
        init="kmeans": sklearn's own start and restarts (dsp_kmeans_train_ubm_device) -- n_init times k-means++ seeding from `seed`, Lloyd
        (kmeans_max_iter, kmeans_tol), the GMM of the labels, EM; the restart with the largest last lower bound is returned, and the dict
        also carries "report": winner and per restart rows, kmeans_n_iter, kmeans_stop, kmeans_n_empty, em_n_iter, em_converged, lower_bound."""
        max_iter, tol = int(max_iter), float(tol)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        if not tol >= 0.0:
            raise ValueError("tol must be >= 0")
        if isinstance(init, str):
            if init != "kmeans":
                raise ValueError('init must be None, a dict or "kmeans"')
            return self._fit_kmeans(feats, max_iter, tol, self._reg_covar(reg_covar), n_init, seed, kmeans_max_iter, kmeans_tol)
        if int(n_init) != 1:
            raise ValueError('n_init restarts need init="kmeans"')
        reg_covar = self._reg_covar(reg_covar)
        k, d = self.k, self.d
        start = None
        if init is not None:
            keep = {key: np.ascontiguousarray(init[key], np.float64) for key in ("weights", "means", "variances")}
            if keep["weights"].shape != (k,) or keep["means"].shape != (k, d) or keep["variances"].shape != (k, d):
                raise ValueError(f"init: weights must be [{k}], means and variances [{k}][{d}]")
            if not all(np.isfinite(v).all() for v in keep.values()):
                raise ValueError("init: weights, means and variances must be finite")
            if not ((keep["weights"] > 0).all() and abs(keep["weights"].sum() - 1.0) <= 1e-6):
                raise ValueError("init: weights must be > 0 and sum to 1")
            if not (keep["variances"] > 0).all():
                raise ValueError("init: variances must be > 0")
            start = _lib.UbmInit(*[keep[key].ctypes.data for key in ("weights", "means", "variances")])
        feats = self._rows(feats)
        out, res = self._result_arrays(max_iter)
        cfg = _lib.UbmConfig(max_iter, tol, reg_covar)
        _lib.check(self._L.dsp_ubm_train_device(self._h, feats.data_ptr(), feats.shape[0], C.byref(start) if start is not None else None,
                                                C.byref(cfg), C.byref(res), _lib.current_stream(feats)), "dsp_ubm_train_device")
        out["lower_bounds"] = out["lower_bounds"][:res.n_iter].copy()
        out["n_iter"], out["converged"] = int(res.n_iter), bool(res.converged)
        return out

    def _result_arrays(self, max_iter):
        k, d = self.k, self.d
        out = {"weights": np.empty(k), "means": np.empty((k, d)), "variances": np.empty((k, d)), "log_consts": np.empty(k),
               "inv_covs": np.empty((k, d)), "lower_bounds": np.full(max_iter, np.nan)}
        res = _lib.UbmResult()
        res.gmm.log_consts, res.gmm.means, res.gmm.inv_covs = (out[key].ctypes.data for key in ("log_consts", "means", "inv_covs"))
        res.weights, res.variances, res.lower_bounds = (out[key].ctypes.data for key in ("weights", "variances", "lower_bounds"))
        return out, res

    def _fit_kmeans(self, feats, max_iter, tol, reg_covar, n_init, seed, kmeans_max_iter, kmeans_tol):
        n_init, seed = int(n_init), self._seed(seed)
        if n_init < 1:
            raise ValueError("n_init must be >= 1")
        kmeans_max_iter, kmeans_tol = self._kmeans_numbers(kmeans_max_iter, kmeans_tol)
        feats = self._rows(feats)
        out, res = self._result_arrays(max_iter)
        restarts = (_lib.KmeansRestart * n_init)()
        report = _lib.KmeansUbmReport(restarts, -1)
        cfg = _lib.KmeansUbmConfig(n_init, seed, kmeans_max_iter, kmeans_tol, _lib.UbmConfig(max_iter, tol, reg_covar))
        _lib.check(self._L.dsp_kmeans_train_ubm_device(self._h, feats.data_ptr(), feats.shape[0], C.byref(cfg), C.byref(res), C.byref(report), _lib.current_stream(feats)),
                   "dsp_kmeans_train_ubm_device")
        out["lower_bounds"] = out["lower_bounds"][:res.n_iter].copy()
        out["n_iter"], out["converged"] = int(res.n_iter), bool(res.converged)
        out["report"] = {"winner": int(report.winner),
                         "restarts": [{"rows": np.array(r.rows[:self.k], np.int64), "kmeans_n_iter": int(r.kmeans_n_iter), "kmeans_stop": _lib.KMEANS_STOP[r.kmeans_stop],
                                       "kmeans_n_empty": int(r.kmeans_n_empty), "em_n_iter": int(r.em_n_iter), "em_converged": bool(r.em_converged),
                                       "lower_bound": float(r.lower_bound)} for r in restarts]}
        return out


def quantize_gmm(float_params: dict):
    """Host only (dsp_gmm_quantize): a float GMM (log_consts [k], means [k][d], inv_covs [k][d]; a UbmTrainer.fit result as it is) ->
    (ubm_int, saturated): the integer scorer's tables means int8 = rint(64 mean), inv_covs int32 = rint(2048 inv_cov), log_consts int16 =
    rint(256 log_const), ties to even, each saturated to its type, and the number of entries clamped per table in that order."""
    p, k, d, _keep = _gmm_float_params(float_params, "float_params")
    out = {"means": np.empty((k, d), np.int8), "inv_covs": np.empty((k, d), np.int32), "log_consts": np.empty(k, np.int16)}
    sat = (C.c_int * 3)()
    _lib.check(_lib.load().dsp_gmm_quantize(C.byref(p), out["means"].ctypes.data, out["inv_covs"].ctypes.data, out["log_consts"].ctypes.data, sat),
               "dsp_gmm_quantize")
    return out, {"means": int(sat[0]), "inv_covs": int(sat[1]), "log_consts": int(sat[2])}


def upsample_linear(x, new_size: int):
    """x: cuda float32 [n_clips][old] (or [old]) -> [n_clips][new_size]; numpy input goes through the host entry point."""
    L = _lib.load()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(new_size, np.float32)
        _lib.check(L.dsp_upsample_linear_host(x.ctypes.data, x.size, out.ctypes.data, new_size), "dsp_upsample_linear_host")
        return out
    import torch
    squeeze = x.dim() == 1
    x2 = x[None] if squeeze else x
    if x2.stride(1) != 1:
        raise ValueError("x must have unit inner stride")
    out = torch.empty((x2.shape[0], new_size), dtype=torch.float32, device=x.device)
    _lib.check(L.dsp_upsample_linear_device(x2.data_ptr(), x2.shape[0], x2.shape[1], x2.stride(0), out.data_ptr(), new_size,
                                            new_size, _lib.current_stream(x)), "dsp_upsample_linear_device")
    return out[0] if squeeze else out


__all__ = ["StopModel", "SpeakerModel", "Scanner", "StreamSession", "Cmvn", "SpeakerEnroller", "UbmTrainer", "quantize_gmm", "stream_push_plan", "scan_window_offsets", "upsample_linear", "MfccPlan", "default_config"]
