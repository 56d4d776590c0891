"""Host-side mirror of cepstrum/scrubjay_infer.c: clip -> MFCC -> mean|std pooling
(`mfcc_stats`, :19-77) -> Scaler + RBF-SVM (`ort_predict`, :105-141, graph
cepstrum/scrubjay_svm.onnx) over the C ABI, all on HBM-resident tensors.

The reference's MFCC front end is aubio (unvendored, unpinned) with a 2048/1024 framing;
here the front end is this library's MFCC chain with `n_mfcc = 20`,
so feature VALUES are not comparable with the reference's -- the pooling and the SVM
arithmetic are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from .consumers import _frame_offsets, _scan_config, _scan_mfcc, scan_window_offsets
from .mfcc import MfccPlan, default_config, ragged_frame_offsets


class SvmModel(_lib.Handle):
    """dsp_svm: Scaler + SVMClassifier attributes as decoded from the ONNX file."""

    _destroy = "dsp_svm_destroy"

    def __init__(self, attrs: dict, device: int = 0):
        a = {k: np.ascontiguousarray(attrs[k], np.float32) for k in ("offset", "scale", "sv", "coef")}
        self.n_features = a["offset"].size
        self.n_sv = a["coef"].size
        if a["sv"].shape != (self.n_sv, self.n_features):
            raise ValueError(f"sv must be [n_sv][n_features] = [{self.n_sv}][{self.n_features}]")
        self._create("dsp_svm_create", device, self.n_features, self.n_sv, a["offset"].ctypes.data, a["scale"].ctypes.data,
                     a["sv"].ctypes.data, a["coef"].ctypes.data,
                     float(np.ravel(attrs["kernel_params"])[0]), float(np.ravel(attrs["rho"])[0]),
                     float(np.ravel(attrs["prob_a"])[0]), float(np.ravel(attrs["prob_b"])[0]))
        self.device = device

    def predict(self, feat):
        """feat: cuda float32 [n][n_features] -> (labels int32, decision float32, prob1 float32)."""
        import torch
        n = feat.shape[0]
        labels = torch.empty(n, dtype=torch.int32, device=feat.device)
        dec = torch.empty(n, dtype=torch.float32, device=feat.device)
        p1 = torch.empty(n, dtype=torch.float32, device=feat.device)
        st = _lib.current_stream(feat)
        _lib.check(self._L.dsp_svm_predict_device(self._h, feat.contiguous().data_ptr(), n, labels.data_ptr(), dec.data_ptr(),
                                                  p1.data_ptr(), st), "dsp_svm_predict_device")
        return labels, dec, p1

    def scan(self, mfcc, frame_offsets, window_frames: int, hop_frames: int):
        """mean | std and the SVM per sliding window of rows of a ragged MFCC matrix (dsp_svm_scan_device): mfcc cuda float32
        [F][n_features / 2], recording r = rows [frame_offsets[r], frame_offsets[r + 1]), every recording >= 1 row -> (window_offsets
        int64 [n + 1], labels int32, decision float32, prob1 float32 [W], feat float32 [W][n_features]).  No head rows: under stream
        framing a window's first rows differ from its cut-out clip's (ScrubJayScanner computes those)."""
        wo = scan_window_offsets(frame_offsets, window_frames, hop_frames)
        fo = _frame_offsets(frame_offsets)
        if self.n_features % 2:
            raise ValueError("the scan pools n_features / 2 coefficients per row: n_features must be even")
        mfcc = _scan_mfcc(mfcc, fo, self.n_features // 2)
        out = _window_outputs(int(wo[-1]), self.n_features, mfcc.device)
        st = _lib.current_stream(mfcc)
        _lib.check(self._L.dsp_svm_scan_device(self._h, mfcc.data_ptr(), fo.size - 1, fo.ctypes.data_as(_lib.LP),
                                               C.byref(_scan_config(window_frames, hop_frames)), *[t.data_ptr() for t in out], st),
                   "dsp_svm_scan_device")
        return (wo,) + out


def _window_outputs(n, n_features, device):
    import torch
    return (torch.empty(n, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.float32, device=device),
            torch.empty(n, dtype=torch.float32, device=device), torch.empty((n, n_features), dtype=torch.float32, device=device))


def scan_window_spans(config, offsets, window_frames: int, hop_frames: int):
    """Host only: each scan window's clip in samples (dsp_scan_window_spans) for recordings r = samples [offsets[r], offsets[r + 1]) under
    the MfccConfig `config` -> (starts int64 [W], lengths int64 [W]), absolute positions in the buffer.  Cutting these out and running
    them as clips gives what the scans compute per window."""
    cfg = _scan_config(window_frames, hop_frames)
    off, n = _lib.c_offsets(offsets)
    L, lp = _lib.load(), _lib.LP
    total = _lib.check(L.dsp_scan_window_spans(C.byref(config), C.byref(cfg), off, n, None, None), "dsp_scan_window_spans")
    starts, lengths = np.zeros(total, np.int64), np.zeros(total, np.int64)
    _lib.check(L.dsp_scan_window_spans(C.byref(config), C.byref(cfg), off, n, starts.ctypes.data_as(lp), lengths.ctypes.data_as(lp)),
               "dsp_scan_window_spans")
    return starts, lengths


def mfcc_stats(mfcc):
    """mfcc: cuda float32 [n_clips][T][n_coef] -> cuda float32 [n_clips][2*n_coef] (mean | std)."""
    import torch
    n, t, c = mfcc.shape
    feat = torch.empty((n, 2 * c), dtype=torch.float32, device=mfcc.device)
    st = _lib.current_stream(mfcc)
    _lib.check(_lib.load().dsp_mfcc_stats_device(mfcc.contiguous().data_ptr(), n, t, c, feat.data_ptr(), st), "dsp_mfcc_stats_device")
    return feat


def scrubjay_infer_config(sample_rate: int = 16000, aubio: bool = True):
    """The front end cepstrum/scrubjay_infer.c itself runs (:9-13, :28-30, :39-53).  aubio=True (default):
    dsp_mfcc_scrubjay_infer_config -- aubio 0.4's semantics for the calls the file makes: streaming 2048 / 1024 frames with zero
    history and the zero-padded last hop (T = ceil(n / 1024)), periodic Hann, MAGNITUDE spectrum, the 40-filter Slaney bank,
    log10, orthonormal DCT-II, 20 coefficients (aubio is unvendored: restated from its published algorithm, parity unpinned).
    aubio=False: only the file's numbers (2048 / 1024 / 40 / 20) on this library's mfcc.c semantics (round 2's config5_2048)."""
    if not aubio:
        return default_config(sample_rate=sample_rate, n_fft=2048, frame_length=2048, hop_length=1024, n_mels=40, n_mfcc=20,
                              fmin=0.0, fmax=sample_rate / 2.0)
    from .lib import MfccConfig
    cfg = MfccConfig()
    _lib.load().dsp_mfcc_scrubjay_infer_config(C.byref(cfg), int(sample_rate))
    return cfg


class ScrubJay:
    """clips -> label / probability, the scrubjay_infer.c main loop (:158-177) for a batch in HBM."""

    def __init__(self, svm_attrs: dict, device: int = 0, n_mfcc: int = 20, config=None):
        """config: an MfccConfig (its n_mfcc must be half the SVM's feature count), e.g. scrubjay_infer_config();
        default: the reference's 512-point keyword front end with n_mfcc coefficients (BASELINE config 5)."""
        self.plan = MfccPlan(config if config is not None else default_config(n_mfcc=n_mfcc), device)
        self.svm = SvmModel(svm_attrs, device)

    @classmethod
    def train(cls, clips_or_features, labels, device: int = 0, n_mfcc: int = 20, config=None, max_frames: int = 1 << 20, **fit_args):
        """Trains the SVM (SvmTrainer.fit, which takes fit_args) and returns (the ScrubJay built on it, the fit's report).  A float32 CUDA
        tensor [n][2 n_mfcc] is taken as pooled features; anything else as clips [n][samples], pooled by this front end first."""
        cfg = config if config is not None else default_config(n_mfcc=n_mfcc)
        x = clips_or_features
        if not (x.dim() == 2 and x.shape[1] == 2 * cfg.n_mfcc):
            x = mfcc_stats(MfccPlan(cfg, device).clips(x, max_frames))
        trainer = SvmTrainer(2 * cfg.n_mfcc, device)
        try:
            attrs, report = trainer.fit(x, labels, **fit_args)
        finally:
            trainer.close()
        return cls(attrs, device, config=cfg), report

    def __call__(self, clips, max_frames: int = 1 << 20, fused: bool = True):
        """-> (labels int32, decision float32, prob1 float32, features float32 [n][2 n_mfcc]).  fused: one kernel from PCM to
        label (dsp_scrubjay_fused_device, BASELINE config 5); otherwise MFCC -> pooling -> SVM as three kernels."""
        if not fused:
            mfcc = self.plan.clips(clips, max_frames)
            feat = mfcc_stats(mfcc)
            return self.svm.predict(feat) + (feat,)
        import torch
        n = _lib.clips_device(clips, torch.float32).shape[0]
        labels = torch.empty(n, dtype=torch.int32, device=clips.device)
        dec = torch.empty(n, dtype=torch.float32, device=clips.device)
        p1 = torch.empty(n, dtype=torch.float32, device=clips.device)
        feat = torch.empty((n, self.svm.n_features), dtype=torch.float32, device=clips.device)
        st = _lib.current_stream(clips)
        _lib.check(_lib.load().dsp_scrubjay_fused_device(self.plan._h, self.svm._h, clips.data_ptr(), n, clips.shape[1], clips.stride(0),
                                                         int(min(max_frames, 1 << 30)), labels.data_ptr(), dec.data_ptr(), p1.data_ptr(),
                                                         feat.data_ptr(), st), "dsp_scrubjay_fused_device")
        return labels, dec, p1, feat

    def pcm16(self, pcm, max_frames: int = 1 << 20, stereo_mode: int = 0):
        """The fused clip -> label kernel on int16 PCM [n_clips][n] (mono) or [n_clips][n][2] (interleaved stereo: channel 0 or the
        channels' average), converted in the kernel's load (dsp_scrubjay_fused_pcm16_device): the float path's results, bit for bit."""
        import torch
        channels, stride = _lib.pcm_device(pcm)
        n = pcm.shape[0]
        labels = torch.empty(n, dtype=torch.int32, device=pcm.device)
        dec = torch.empty(n, dtype=torch.float32, device=pcm.device)
        p1 = torch.empty(n, dtype=torch.float32, device=pcm.device)
        feat = torch.empty((n, self.svm.n_features), dtype=torch.float32, device=pcm.device)
        st = _lib.current_stream(pcm)
        _lib.check(_lib.load().dsp_scrubjay_fused_pcm16_device(self.plan._h, self.svm._h, pcm.data_ptr(), n, pcm.shape[1], stride,
                                                               channels, int(stereo_mode), int(min(max_frames, 1 << 30)), labels.data_ptr(), dec.data_ptr(),
                                                               p1.data_ptr(), feat.data_ptr(), st), "dsp_scrubjay_fused_pcm16_device")
        return labels, dec, p1, feat

    def ragged(self, signal, offsets, max_frames: int = 1 << 20, stereo_mode: int = 0):
        """Clips of different lengths in ONE launch (the files scrubjay_infer.c:158-176 loops over): `signal` is a flat cuda buffer --
        float32 [total], int16 [total] or interleaved stereo int16 [total][2] -- and clip c is samples [offsets[c], offsets[c + 1]).
        Results as a one-clip call per clip gives them (dsp_scrubjay_fused_ragged_device / _pcm16_device)."""
        import torch
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        labels = torch.empty(n, dtype=torch.int32, device=signal.device)
        dec = torch.empty(n, dtype=torch.float32, device=signal.device)
        p1 = torch.empty(n, dtype=torch.float32, device=signal.device)
        feat = torch.empty((n, self.svm.n_features), dtype=torch.float32, device=signal.device)
        st = _lib.current_stream(signal)
        mf = int(min(max_frames, 1 << 30))
        if channels:
            _lib.check(_lib.load().dsp_scrubjay_fused_ragged_pcm16_device(self.plan._h, self.svm._h, ptr, n, off, channels, int(stereo_mode), mf,
                                                                          labels.data_ptr(), dec.data_ptr(), p1.data_ptr(), feat.data_ptr(), st),
                       "dsp_scrubjay_fused_ragged_pcm16_device")
        else:
            _lib.check(_lib.load().dsp_scrubjay_fused_ragged_device(self.plan._h, self.svm._h, ptr, n, off, mf, labels.data_ptr(), dec.data_ptr(),
                                                                    p1.data_ptr(), feat.data_ptr(), st), "dsp_scrubjay_fused_ragged_device")
        return labels, dec, p1, feat


def svm_folds(n: int, k: int, seed: int = 0):
    """Host only: fold ids int32 [n] in 0 .. k - 1 by libsvm's shuffle on the library's own draws (dsp_svm_folds)."""
    ids = np.empty(int(n), np.int32)
    _lib.check(_lib.load().dsp_svm_folds(int(n), int(k), int(seed) & (2**64 - 1), ids.ctypes.data), "dsp_svm_folds")
    return ids


def svm_balanced_weights(labels, c: float = 1.0, rows=None):
    """Host only: sklearn's class_weight="balanced" as box bounds, C n / (2 n_label) over `rows` (default: all) -> (C_label0, C_label1)."""
    labels = np.ascontiguousarray(labels, np.int32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    c0, c1 = C.c_double(), C.c_double()
    _lib.check(_lib.load().dsp_svm_balanced_weights(labels.ctypes.data, None if rows is None else rows.ctypes.data,
                                                    labels.size if rows is None else rows.size, float(c), C.byref(c0), C.byref(c1)),
               "dsp_svm_balanced_weights")
    return c0.value, c1.value


def svm_model_from_training(z, labels, coef):
    """Host only: the support vectors of a solved problem in libsvm's order (dsp_svm_model_from_training): z float32 [n][nf], labels [n],
    coef float64 [n] -> (sv float32 [n_sv][nf], coef float32 [n_sv], how many carry label 0)."""
    z = np.ascontiguousarray(z, np.float32)
    labels = np.ascontiguousarray(labels, np.int32)
    coef = np.ascontiguousarray(coef, np.float64)
    n, nf = z.shape
    sv, c32, n0 = np.empty((n, nf), np.float32), np.empty(n, np.float32), C.c_long()
    n_sv = _lib.check(_lib.load().dsp_svm_model_from_training(z.ctypes.data, labels.ctypes.data, coef.ctypes.data, n, nf, sv.ctypes.data,
                                                               c32.ctypes.data, n, C.byref(n0)), "dsp_svm_model_from_training")
    return sv[:n_sv].copy(), c32[:n_sv].copy(), n0.value


class SvmTrainer(_lib.Handle):
    """dsp_svm_trainer: the scrub-jay RBF-SVM from pooled features, cepstrum/train.py:66-85 on the GPU -- the Scaler, batched SMO over one
    shared distance matrix, libsvm's Platt fit, cross-validation over a (C, gamma) grid.  Features are cuda float32 [n][n_features]
    (mfcc_stats, or the features ScrubJay returns), labels 0 / 1 on the host.  One stream at a time per trainer."""

    _destroy = "dsp_svm_trainer_destroy"

    def __init__(self, n_features: int, device: int = 0):
        self._create("dsp_svm_trainer_create", device, int(n_features))
        self.n_features, self.device, self.n = int(n_features), device, 0

    def _features(self, feat):
        import torch
        if not (isinstance(feat, torch.Tensor) and feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 2 and feat.shape[1] == self.n_features):
            raise ValueError(f"feat must be a float32 CUDA tensor [n][{self.n_features}]")
        if feat.device.index != self.device:
            raise ValueError(f"feat is on GPU {feat.device.index}, the trainer on GPU {self.device}")
        return feat.contiguous()

    def set(self, feat, scaler_rows=None, offset=None, scale=None):
        """The dataset of the calls that follow (dsp_svm_train_set_device): fits the Scaler on `scaler_rows` (default: all rows) or takes
        the caller's offset / scale, standardises and builds the distance matrix -> (offset, scale) float32 [n_features]."""
        feat = self._features(feat)
        rows = None if scaler_rows is None else np.ascontiguousarray(scaler_rows, np.int32)
        given = None if offset is None else (np.ascontiguousarray(offset, np.float32), np.ascontiguousarray(scale, np.float32))
        if given is not None and (given[0].size != self.n_features or given[1].size != self.n_features):
            raise ValueError("offset and scale must hold n_features values")
        off, scl = np.empty(self.n_features, np.float32), np.empty(self.n_features, np.float32)
        self.n = 0
        _lib.check(self._L.dsp_svm_train_set_device(self._h, feat.data_ptr(), feat.shape[0], None if rows is None else rows.ctypes.data,
                                                    0 if rows is None else rows.size, None if given is None else given[0].ctypes.data,
                                                    None if given is None else given[1].ctypes.data, off.ctypes.data, scl.ctypes.data, self._stream()),
                   "dsp_svm_train_set_device")
        self.n = feat.shape[0]
        return off, scl

    def rows(self):
        """the standardised rows of the dataset, float32 [n][n_features] on the host"""
        z = np.empty((self.n, self.n_features), np.float32)
        _lib.check(self._L.dsp_svm_train_rows_host(self._h, z.ctypes.data, self._stream()), "dsp_svm_train_rows_host")
        return z

    def problems(self, problems, labels, eps: float = 1e-3, max_iter: int = 0, decisions: bool = True, q_float32: bool = False):
        """Solves problems = [(rows, C_label0, C_label1, gamma), ...] on the dataset in ONE launch (dsp_svm_train_problems_device) ->
        (results: numpy records of SVM_TRAIN_RESULT_DTYPE [P], coef cuda float64 [P][n], dec cuda float64 [P][n] or None).  q_float32:
        the solver rounds its kernel values to float32 as libsvm rounds the Q it caches, which gives libsvm's answer rather than float64's."""
        import torch
        labels = np.ascontiguousarray(labels, np.int32)
        if labels.size != self.n:
            raise ValueError(f"labels must hold the dataset's {self.n} rows")
        keep = [np.ascontiguousarray(p[0], np.int32) for p in problems]
        table = (_lib.SvmTrainProblem * max(1, len(problems)))()
        for k, (p, r) in enumerate(zip(problems, keep)):
            table[k] = _lib.SvmTrainProblem(r.ctypes.data if r.size else None, r.size, float(p[1]), float(p[2]), float(p[3]))
        results = np.zeros(len(problems), _lib.SVM_TRAIN_RESULT_DTYPE)
        dev = torch.device("cuda", self.device)
        coef = torch.empty((len(problems), self.n), dtype=torch.float64, device=dev)
        dec = torch.empty((len(problems), self.n), dtype=torch.float64, device=dev) if decisions else None
        cfg = _lib.SvmTrainConfig(float(eps), int(max_iter), int(bool(q_float32)))
        _lib.check(self._L.dsp_svm_train_problems_device(self._h, table, len(problems), C.byref(cfg), labels.ctypes.data, results.ctypes.data,
                                                         coef.data_ptr(), dec.data_ptr() if decisions else None, self._stream()),
                   "dsp_svm_train_problems_device")
        return results, coef, dec

    def platt(self, dec_cv, labels, rows=None):
        """libsvm's sigmoid_train on (dec_cv[r], labels[r]), dec_cv cuda float64 [n] (dsp_svm_platt_fit_device) -> (A, B, n_iter)."""
        import torch
        if not (isinstance(dec_cv, torch.Tensor) and dec_cv.is_cuda and dec_cv.dtype == torch.float64 and dec_cv.numel() == self.n):
            raise ValueError(f"dec_cv must be a float64 CUDA tensor [{self.n}]")
        labels = np.ascontiguousarray(labels, np.int32)
        if labels.size != self.n:
            raise ValueError(f"labels must hold the dataset's {self.n} rows")
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        a, b, it = C.c_double(), C.c_double(), C.c_int()
        _lib.check(self._L.dsp_svm_platt_fit_device(self._h, dec_cv.contiguous().data_ptr(), labels.ctypes.data, None if rows is None else rows.ctypes.data,
                                                    0 if rows is None else rows.size, C.byref(a), C.byref(b), C.byref(it), self._stream()),
                   "dsp_svm_platt_fit_device")
        return a.value, b.value, it.value

    @staticmethod
    def _box(labels, c, class_weight, rows=None):
        if class_weight == "balanced":
            return svm_balanced_weights(labels, c, rows)
        if class_weight is None:
            return float(c), float(c)
        return float(c) * float(class_weight[0]), float(c) * float(class_weight[1])

    @staticmethod
    def _scale_gamma(z) -> float:
        """sklearn's gamma="scale", 1 / (n_features var(z)) over every element of the standardised training rows, as the float the model holds"""
        return float(np.float32(1.0 / (z.shape[1] * float(z.double().var(unbiased=False)))))

    def fit(self, feat, labels, C=10.0, gamma="scale", class_weight="balanced", probability_folds: int = 5, fold_ids=None, seed: int = 0,
            eps: float = 1e-3, max_iter: int = 0, q_float32: bool = False):
        """The reference's clf.fit (dsp_svm_fit_device): the Scaler on all rows, `probability_folds` inner problems and the final one in one
        launch, the Platt fit -> (attrs: the dict SvmModel takes, report: dict).  gamma "scale" is 1 / (n_features var(z)) computed with
        torch on the standardised rows; every gamma is rounded to the float32 the model holds before it is trained with.  q_float32: the
        solver rounds its kernel values to float32 as libsvm rounds the Q it caches (the answer sklearn gives, not float64's)."""
        import ctypes                                                # (the parameter C, sklearn's name, hides this module's alias)
        import torch
        feat = self._features(feat)
        labels = np.ascontiguousarray(labels, np.int32)
        n, nf = feat.shape
        if labels.size != n:
            raise ValueError("labels must hold one label per row")
        if gamma == "scale":
            x = feat.double()
            mean = x.mean(dim=0)
            std = ((x - mean) ** 2).mean(dim=0).sqrt()
            scl = torch.where(std > 0, 1.0 / torch.where(std > 0, std, torch.ones_like(std)), torch.ones_like(std)).float()
            gamma = self._scale_gamma((feat - mean.float()) * scl)
        else:
            gamma = float(np.float32(gamma))
        c0, c1 = self._box(labels, C, class_weight)
        ids = None if fold_ids is None else np.ascontiguousarray(fold_ids, np.int32)
        if ids is not None and ids.size != n:
            raise ValueError("fold_ids must hold one id per row")
        out = {"offset": np.empty(nf, np.float32), "scale": np.empty(nf, np.float32), "sv": np.empty((n, nf), np.float32), "coef": np.empty(n, np.float32)}
        model = _lib.SvmFitModel(*[out[k].ctypes.data for k in ("offset", "scale", "sv", "coef")])
        cfg = _lib.SvmTrainConfig(float(eps), int(max_iter), int(bool(q_float32)))
        self.n = 0
        _lib.check(self._L.dsp_svm_fit_device(self._h, feat.data_ptr(), n, labels.ctypes.data, None if ids is None else ids.ctypes.data,
                                              int(probability_folds), int(seed) & (2**64 - 1), c0, c1, gamma, ctypes.byref(cfg), ctypes.byref(model),
                                              self._stream()), "dsp_svm_fit_device")
        self.n = n
        n_sv, n0 = int(model.n_sv), int(model.n_sv_label0)
        attrs = {"offset": out["offset"], "scale": out["scale"], "sv": out["sv"][:n_sv].copy(), "coef": out["coef"][:n_sv].copy(),
                 "kernel_params": np.array([model.gamma, 0.0, 3.0], np.float32), "rho": np.array([model.rho], np.float32),
                 "prob_a": np.array([model.prob_a], np.float32), "prob_b": np.array([model.prob_b], np.float32),
                 "vectors_per_class": np.array([n0, n_sv - n0], np.int64)}
        f = model.final
        report = {"gamma": gamma, "C": (c0, c1), "n_sv": n_sv, "n_iter": f.n_iter, "n_bounded": f.n_bounded, "objective": f.objective, "gap": f.gap,
                  "rho": f.rho, "status": _lib.SVM_TRAIN_STATUS[f.status], "platt_iter": int(model.platt_iter)}
        return attrs, report

    def cross_validate(self, feat, labels, fold_ids, Cs, gammas, class_weight="balanced", eps: float = 1e-3, max_iter: int = 0, q_float32: bool = False):
        """The reference's cross-validation over a grid: per outer fold the Scaler is fitted on the fold's training rows, and all
        len(Cs) len(gammas) problems (grid point g = index of C times len(gammas) + index of gamma) run in ONE launch; a row's held-out
        decision comes from the fold it was left out of.  gammas may hold "scale".  -> dict: dec cuda float64 [grid][n], precision,
        recall, f1 cuda float64 [grid] of label 1, status int [folds][grid], grid [(C, gamma)] (gamma "scale" stays "scale")."""
        import torch
        feat = self._features(feat)
        labels = np.ascontiguousarray(labels, np.int32)
        ids = np.ascontiguousarray(fold_ids, np.int32)
        n = feat.shape[0]
        if labels.size != n or ids.size != n:
            raise ValueError("labels and fold_ids must hold one value per row")
        grid = [(c, g) for c in Cs for g in gammas]
        held = torch.zeros((len(grid), n), dtype=torch.float64, device=feat.device)
        status = []
        for f in np.unique(ids):
            train = np.nonzero(ids != f)[0].astype(np.int32)
            test = torch.from_numpy(np.nonzero(ids == f)[0]).to(feat.device)
            self.set(feat, scaler_rows=train)
            scale_gamma = self._scale_gamma(torch.from_numpy(self.rows()[train])) if any(g == "scale" for g in gammas) else None
            problems = []
            for c, g in grid:
                c0, c1 = self._box(labels, c, class_weight, train)
                problems.append((train, c0, c1, scale_gamma if g == "scale" else float(g)))
            results, _coef, dec = self.problems(problems, labels, eps, max_iter, q_float32=q_float32)
            held[:, test] = dec[:, test]
            status.append(results["status"].copy())
        truth = torch.from_numpy(labels).to(feat.device)[None, :] == 1
        pred = held <= 0                                             # label 1 where dec is not above 0 (dsp_svm_predict_device's vote)
        tp = (pred & truth).sum(dim=1).double()
        precision = tp / pred.sum(dim=1).clamp(min=1)
        recall = tp / truth.sum(dim=1).clamp(min=1)
        f1 = 2 * precision * recall / (precision + recall).clamp(min=1e-300)
        return {"dec": held, "precision": precision, "recall": recall, "f1": f1, "status": np.stack(status), "grid": grid}


class ScrubJayScanner(_lib.Handle):
    """dsp_scrubjay_scanner: long recordings back to back in HBM -> label, decision, P(label 1) and the pooled features per window of
    window_frames MFCC rows every hop_frames rows, each equal to ScrubJay.ragged on the window cut out (scan_window_spans).  Borrows
    the ScrubJay's plan and SVM.  One stream at a time per scanner."""

    _destroy = "dsp_scrubjay_scanner_destroy"

    def __init__(self, scrubjay: ScrubJay, window_frames: int = 16, hop_frames: int = 4):
        self.cfg = _scan_config(window_frames, hop_frames)
        self._create("dsp_scrubjay_scanner_create", scrubjay.plan._h, scrubjay.svm._h, C.byref(self.cfg))
        self.scrubjay = scrubjay          # (the scanner borrows its plan and SVM: keep them alive)

    def run(self, signal, offsets, stereo_mode: int = 0):
        """signal: cuda float32 [total], int16 [total] (mono) or int16 [total][2] (interleaved stereo), recording r = samples
        [offsets[r], offsets[r + 1]) per channel -> (window_offsets int64 [n + 1], labels int32, decision float32, prob1 float32 [W],
        feat float32 [W][n_features])."""
        import torch
        off, n, channels, ptr = _lib.ragged_signal(signal, offsets, torch.float32)
        if channels and stereo_mode not in (0, 1):
            raise ValueError("stereo_mode must be 0 (channel 0) or 1 (average)")
        fo = ragged_frame_offsets(self.scrubjay.plan.cfg, (off, n), 2**31 - 1)
        wo = scan_window_offsets(fo, self.cfg.window_frames, self.cfg.hop_frames)
        out = _window_outputs(int(wo[-1]), self.scrubjay.svm.n_features, signal.device)
        st = _lib.current_stream(signal)
        ptrs = [t.data_ptr() for t in out]
        if channels:
            _lib.check(self._L.dsp_scrubjay_scanner_run_pcm16_device(self._h, ptr, n, off, channels, int(stereo_mode), *ptrs, st),
                       "dsp_scrubjay_scanner_run_pcm16_device")
        else:
            _lib.check(self._L.dsp_scrubjay_scanner_run_device(self._h, ptr, n, off, *ptrs, st), "dsp_scrubjay_scanner_run_device")
        return (wo,) + out
