"""ctypes binding of libdsp_amd.so (include/dsp_amd.h).  Fails loudly: there is
no Python/CPU implementation behind these calls."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build


class DspError(RuntimeError):
    pass


class MfccConfig(C.Structure):
    """dsp_mfcc_config (include/dsp_amd.h); defaults = mfcc_params.h:6-12 of the reference."""

    _fields_ = [
        ("sample_rate", C.c_int), ("n_fft", C.c_int), ("frame_length", C.c_int),
        ("hop_length", C.c_int), ("n_mels", C.c_int), ("n_mfcc", C.c_int),
        ("window", C.c_int), ("mel_norm", C.c_int), ("log_mode", C.c_int),
        ("prefilter", C.c_int), ("win_length", C.c_int),
        ("fmin", C.c_float), ("fmax", C.c_float), ("amin", C.c_float), ("top_db", C.c_float),
        ("spectrum", C.c_int), ("framing", C.c_int),
    ]


class LaneTables512(C.Structure):
    """dsp::LaneTables512 (dsp_amd/csrc/tables.hpp): the per-lane kernel layout of the constant tables."""

    _fields_ = [
        ("win", (C.c_float * 64) * 8), ("tw1", (C.c_float * 64) * 6), ("tw2", (C.c_float * 64) * 6),
        ("tw3", (C.c_float * 64) * 6), ("twp", (C.c_float * 64) * 4),
        ("kappa", C.c_int32 * 64), ("partner", C.c_int32 * 64),
        ("mel_k0", C.c_int32 * 64), ("mel_w", (C.c_float * 64) * 12), ("mel_src", (C.c_int32 * 64) * 6),
        ("mel_gather", C.c_int32), ("mel_conflict_free", C.c_int32),
        ("dct_w", (C.c_float * 64) * 20), ("dct_split", C.c_int32), ("dct_len", C.c_int32),
        ("n_mels", C.c_int32), ("n_mfcc", C.c_int32),
        ("dct_a", ((C.c_float * 64) * 16) * 2),
    ]


class GenTables1024(C.Structure):
    """dsp::GenTables1024 (dsp_amd/csrc/tables.hpp): the tables of both 1024-point kernels; dsp_mfcc1024_tables fills it."""

    _fields_ = [
        ("win", (C.c_float * 64) * 16), ("w512", (C.c_float * 512) * 2), ("w1024", (C.c_float * 256) * 2),
        ("mel_k0", (C.c_int32 * 64) * 4), ("mel_w", ((C.c_float * 64) * 12) * 4), ("mel_src", ((C.c_int32 * 64) * 6) * 2),
        ("dct_w", (C.c_float * 64) * 32),
        ("n_chunk_slots", C.c_int32), ("n_mels", C.c_int32), ("n_mfcc", C.c_int32),
        ("tw1", (C.c_float * 64) * 14), ("tw2", (C.c_float * 64) * 14), ("twp", (C.c_float * 64) * 8),
        ("dct_a", (C.c_float * 64) * 32),
    ]


class GenTables2048(C.Structure):
    """dsp::GenTables2048 (dsp_amd/csrc/tables.hpp): the tables of the 2048-point kernel; dsp_mfcc2048_tables fills it."""

    _fields_ = [
        ("win", (C.c_float * 64) * 32), ("w1024", (C.c_float * 1024) * 2), ("w2048", (C.c_float * 512) * 2),
        ("mel_lo", C.c_int32 * 128), ("mel_len", C.c_int32 * 128), ("mel_off", C.c_int32 * 128),
        ("mel_w", C.c_float * 4096), ("dct", (C.c_float * 128) * 32),
        ("n_mels", C.c_int32), ("n_mfcc", C.c_int32),
        ("seg_ok", C.c_int32), ("seg_k0", (C.c_int32 * 64) * 3), ("seg_w", ((C.c_float * 64) * 16) * 3),
        ("mel_s0", C.c_int32 * 128), ("mel_cnt", C.c_int32 * 128),
        ("dct_t", (C.c_float * 64) * 64),
    ]


class StopModelParams(C.Structure):
    """dsp_stop_model_params (include/dsp_amd.h)."""

    _fields_ = [("n_coef", C.c_int), ("max_frames", C.c_int), ("units", C.c_int * 4),
                ("scaler_mean", C.c_void_p), ("scaler_scale", C.c_void_p),
                ("kernel", C.c_void_p * 4), ("bias", C.c_void_p * 4)]


class GmmParams(C.Structure):
    """dsp_gmm_params (include/dsp_amd.h)."""

    _fields_ = [("k", C.c_int), ("d", C.c_int), ("means", C.c_void_p), ("inv_covs", C.c_void_p), ("log_consts", C.c_void_p)]


class GmmFloatParams(C.Structure):
    """dsp_gmm_float_params (include/dsp_amd.h): the float UBM, double arrays."""

    _fields_ = [("k", C.c_int), ("d", C.c_int), ("log_consts", C.c_void_p), ("means", C.c_void_p), ("inv_covs", C.c_void_p)]


class EnrollConfig(C.Structure):
    """dsp_enroll_config (include/dsp_amd.h)."""

    _fields_ = [("map_mode", C.c_int), ("relevance_factor", C.c_float), ("fixed_alpha", C.c_float)]


class UbmInit(C.Structure):
    """dsp_ubm_init (include/dsp_amd.h): the caller's start, double arrays."""

    _fields_ = [("weights", C.c_void_p), ("means", C.c_void_p), ("variances", C.c_void_p)]


class UbmConfig(C.Structure):
    """dsp_ubm_config (include/dsp_amd.h)."""

    _fields_ = [("max_iter", C.c_int), ("tol", C.c_double), ("reg_covar", C.c_double)]


class UbmResult(C.Structure):
    """dsp_ubm_result (include/dsp_amd.h): the caller's double arrays and what the fit did."""

    _fields_ = [("gmm", GmmFloatParams), ("weights", C.c_void_p), ("variances", C.c_void_p), ("lower_bounds", C.c_void_p),
                ("n_iter", C.c_int), ("converged", C.c_int)]


class KmeansConfig(C.Structure):
    """dsp_kmeans_config (include/dsp_amd.h)."""

    _fields_ = [("max_iter", C.c_int), ("tol", C.c_double), ("reg_covar", C.c_double)]


class KmeansResult(C.Structure):
    """dsp_kmeans_result (include/dsp_amd.h): the caller's arrays and how Lloyd stopped."""

    _fields_ = [("centres", C.c_void_p), ("counts", C.c_void_p), ("weights", C.c_void_p), ("means", C.c_void_p), ("variances", C.c_void_p),
                ("d_labels", C.c_void_p), ("inertia", C.c_double), ("n_iter", C.c_int), ("stop", C.c_int), ("n_empty", C.c_int)]


class KmeansUbmConfig(C.Structure):
    """dsp_kmeans_ubm_config (include/dsp_amd.h)."""

    _fields_ = [("n_init", C.c_int), ("seed", C.c_uint64), ("kmeans_max_iter", C.c_int), ("kmeans_tol", C.c_double), ("em", UbmConfig)]


class KmeansRestart(C.Structure):
    """dsp_kmeans_restart (include/dsp_amd.h): what one restart did."""

    _fields_ = [("rows", C.c_long * 64), ("kmeans_n_iter", C.c_int), ("kmeans_stop", C.c_int), ("kmeans_n_empty", C.c_int),
                ("em_n_iter", C.c_int), ("em_converged", C.c_int), ("lower_bound", C.c_double)]


class KmeansUbmReport(C.Structure):
    """dsp_kmeans_ubm_report (include/dsp_amd.h)."""

    _fields_ = [("restarts", C.POINTER(KmeansRestart)), ("winner", C.c_int)]


KMEANS_STOP = ("max_iter", "tol", "strict")      # DSP_KMEANS_STOP_*


class ScanConfig(C.Structure):
    """dsp_scan_config (include/dsp_amd.h): windows of MFCC rows."""

    _fields_ = [("window_frames", C.c_int), ("hop_frames", C.c_int)]


class SegmentConfig(C.Structure):
    """dsp_segment_config (include/dsp_amd.h): thresholds, minimum length, gap and mode of dsp_segments_device."""

    _fields_ = [("on", C.c_float), ("off", C.c_float), ("min_windows", C.c_int), ("max_gap", C.c_int), ("mode", C.c_int)]


class Segment(C.Structure):
    """dsp_segment (include/dsp_amd.h), 32 bytes; SEGMENT_DTYPE is the same as a numpy record."""

    _fields_ = [("recording", C.c_int), ("column", C.c_int), ("first_window", C.c_int), ("n_windows", C.c_int), ("n_active", C.c_int),
                ("peak_window", C.c_int), ("peak", C.c_float), ("mean", C.c_float)]


SEG_INDEPENDENT, SEG_EXCLUSIVE = 0, 1
SEGMENT_DTYPE = [("recording", "<i4"), ("column", "<i4"), ("first_window", "<i4"), ("n_windows", "<i4"), ("n_active", "<i4"), ("peak_window", "<i4"),
                 ("peak", "<f4"), ("mean", "<f4")]


class TrialsConfig(C.Structure):
    """dsp_trials_config (include/dsp_amd.h): the thresholds of the sweep of dsp_trials_evaluate_device."""

    _fields_ = [("n_thresholds", C.c_int)]


class TrialColumn(C.Structure):
    """dsp_trial_column (include/dsp_amd.h), 80 bytes; TRIAL_COLUMN_DTYPE is the same as a numpy record."""

    _fields_ = [("n_target", C.c_long), ("n_nontarget", C.c_long), ("n_nan", C.c_long), ("lo", C.c_double), ("hi", C.c_double),
                ("best_threshold", C.c_double), ("best_correct", C.c_long), ("auc_u2", C.c_long), ("auc", C.c_double), ("best_index", C.c_int),
                ("reserved", C.c_int)]


TRIAL_COLUMN_DTYPE = [("n_target", "<i8"), ("n_nontarget", "<i8"), ("n_nan", "<i8"), ("lo", "<f8"), ("hi", "<f8"), ("best_threshold", "<f8"),
                      ("best_correct", "<i8"), ("auc_u2", "<i8"), ("auc", "<f8"), ("best_index", "<i4"), ("reserved", "<i4")]


class Calibration(C.Structure):
    """dsp_calibration (include/dsp_amd.h): c = a x + b + c log(n_frames); 1, 0, 0 are the reference's constants."""

    _fields_ = [("a", C.c_double), ("b", C.c_double), ("c", C.c_double)]


class CalibrationConfig(C.Structure):
    """dsp_calibration_config (include/dsp_amd.h): the prior, the stopping tolerance and the passes of dsp_calibration_fit_device."""

    _fields_ = [("prior", C.c_double), ("tol", C.c_double), ("max_iter", C.c_int), ("reserved", C.c_int)]


class CalibrationReport(C.Structure):
    """dsp_calibration_report (include/dsp_amd.h), 88 bytes."""

    _fields_ = [("params", Calibration), ("n_target", C.c_long), ("n_nontarget", C.c_long), ("n_excluded", C.c_long), ("objective_start", C.c_double),
                ("objective", C.c_double), ("last_step", C.c_double), ("n_iter", C.c_int), ("n_rejected", C.c_int), ("status", C.c_int), ("reserved", C.c_int)]


CAL_CONVERGED, CAL_MAX_ITER, CAL_STALLED, CAL_SINGULAR, CAL_NO_CLASS = 0, 1, 2, 3, 4
CAL_STATUS = ("converged", "max_iter", "stalled", "singular", "no_class")


class CohortStat(C.Structure):
    """dsp_cohort_stat (include/dsp_amd.h), 32 bytes; COHORT_STAT_DTYPE is the same as a numpy record."""

    _fields_ = [("mean", C.c_double), ("std", C.c_double), ("threshold", C.c_float), ("n_finite", C.c_int), ("n_selected", C.c_int),
                ("n_above", C.c_int)]


class SnormConfig(C.Structure):
    """dsp_snorm_config (include/dsp_amd.h): the mode and the floor of sigma of dsp_score_normalize_device."""

    _fields_ = [("mode", C.c_int), ("reserved", C.c_int), ("std_floor", C.c_double)]


COHORT_STAT_DTYPE = [("mean", "<f8"), ("std", "<f8"), ("threshold", "<f4"), ("n_finite", "<i4"), ("n_selected", "<i4"), ("n_above", "<i4")]
COHORT_PER_ROW, COHORT_PER_COLUMN = 0, 1
NORM_Z, NORM_T, NORM_S = 0, 1, 2
NORM_MODES = {"z": NORM_Z, "t": NORM_T, "s": NORM_S}
COHORT_MAX_LENGTH = COHORT_MAX_TOP_K = 1 << 22


class VadConfig(C.Structure):
    """dsp_vad_config (include/dsp_amd.h), 56 bytes: the framing of the plan whose rows are filtered, and the decision."""

    _fields_ = [("frame_length", C.c_int), ("hop_length", C.c_int), ("framing", C.c_int), ("reference", C.c_int), ("threshold_ratio", C.c_double),
                ("floor_power", C.c_double), ("context_frames", C.c_int), ("proportion", C.c_double), ("pad_frames", C.c_int)]


class VadGeometry(C.Structure):
    """dsp_vad_geometry (include/dsp_amd.h): what dsp_vad_geometry_for reports."""

    _fields_ = [("g", C.c_int), ("m", C.c_int), ("samples_per_tile", C.c_int), ("rows_per_tile", C.c_int), ("halo_rows", C.c_int)]


VAD_CLIP_DTYPE = [("reference", "<f8"), ("threshold", "<f8"), ("n_raw", "<i4"), ("n_kept", "<i4"), ("first_kept", "<i4"), ("last_kept", "<i4")]
VAD_REF_ABSOLUTE, VAD_REF_MAX, VAD_REF_MEAN = 0, 1, 2
VAD_REFERENCES = {"absolute": VAD_REF_ABSOLUTE, "max": VAD_REF_MAX, "mean": VAD_REF_MEAN}


class SvmTrainProblem(C.Structure):
    """dsp_svm_train_problem (include/dsp_amd.h), 40 bytes: rows on the host, a box bound per label, gamma."""

    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_long), ("c_label0", C.c_double), ("c_label1", C.c_double), ("gamma", C.c_double)]


class SvmTrainConfig(C.Structure):
    """dsp_svm_train_config (include/dsp_amd.h)."""

    _fields_ = [("eps", C.c_double), ("max_iter", C.c_int), ("q_float32", C.c_int)]


class SvmTrainResult(C.Structure):
    """dsp_svm_train_result (include/dsp_amd.h), 40 bytes; SVM_TRAIN_RESULT_DTYPE is the same as a numpy record."""

    _fields_ = [("rho", C.c_double), ("objective", C.c_double), ("gap", C.c_double), ("n_iter", C.c_int), ("n_sv", C.c_int),
                ("n_bounded", C.c_int), ("status", C.c_int)]


SVM_TRAIN_RESULT_DTYPE = [("rho", "<f8"), ("objective", "<f8"), ("gap", "<f8"), ("n_iter", "<i4"), ("n_sv", "<i4"), ("n_bounded", "<i4"), ("status", "<i4")]
SVM_TRAIN_CONVERGED, SVM_TRAIN_MAX_ITER, SVM_TRAIN_ONE_CLASS, SVM_TRAIN_EMPTY = 0, 1, 2, 3
SVM_TRAIN_STATUS = ("converged", "max_iter", "one_class", "empty")
SVM_TRAIN_MAX_ROWS = 8192


class SvmFitModel(C.Structure):
    """dsp_svm_fit_model (include/dsp_amd.h), 112 bytes: the caller's arrays and what dsp_svm_fit_device found."""

    _fields_ = [("offset", C.c_void_p), ("scale", C.c_void_p), ("sv", C.c_void_p), ("coef", C.c_void_p), ("n_sv", C.c_long), ("n_sv_label0", C.c_long),
                ("rho", C.c_float), ("prob_a", C.c_float), ("prob_b", C.c_float), ("gamma", C.c_float), ("platt_iter", C.c_int), ("reserved", C.c_int),
                ("final", SvmTrainResult)]


class StopTrainRun(C.Structure):
    """dsp_stop_train_run (include/dsp_amd.h), 88 bytes: the run's rows on the host and its hyperparameters."""

    _fields_ = [("train_rows", C.c_void_p), ("val_rows", C.c_void_p), ("n_train", C.c_long), ("n_val", C.c_long), ("seed", C.c_uint64),
                ("learning_rate", C.c_double), ("dropout", C.c_double * 3), ("batch_size", C.c_int), ("epochs", C.c_int), ("patience", C.c_int),
                ("restore_best", C.c_int)]


class StopTrainResult(C.Structure):
    """dsp_stop_train_result (include/dsp_amd.h), 40 bytes; STOP_TRAIN_RESULT_DTYPE is the same as a numpy record."""

    _fields_ = [("best_val_loss", C.c_double), ("last_loss", C.c_double), ("n_epochs", C.c_int), ("best_epoch", C.c_int), ("status", C.c_int),
                ("val_correct", C.c_int), ("n_dead_units", C.c_int), ("reserved", C.c_int)]


STOP_TRAIN_RESULT_DTYPE = [("best_val_loss", "<f8"), ("last_loss", "<f8"), ("n_epochs", "<i4"), ("best_epoch", "<i4"), ("status", "<i4"),
                           ("val_correct", "<i4"), ("n_dead_units", "<i4"), ("reserved", "<i4")]
STOP_TRAIN_CONVERGED_EARLY, STOP_TRAIN_MAX_EPOCHS, STOP_TRAIN_NO_VALIDATION, STOP_TRAIN_EMPTY = 0, 1, 2, 3
STOP_TRAIN_STATUS = ("converged_early", "max_epochs", "no_validation", "empty")
STOP_TRAIN_CAP_ROWS, STOP_TRAIN_CAP_UNITS, STOP_TRAIN_CAP_BATCH, STOP_TRAIN_CAP_EPOCHS, STOP_TRAIN_CAP_RUNS = 65536, 16, 256, 10000, 4096


class AugmentOp(C.Structure):
    """dsp_augment_op (include/dsp_amd.h), 40 bytes; AUGMENT_OP_DTYPE is the same as a numpy record."""

    _fields_ = [("clip", C.c_long), ("kind", C.c_int), ("rate", C.c_double), ("n_steps", C.c_int), ("sigma", C.c_float), ("key", C.c_uint64)]


AUGMENT_OP_DTYPE = {"names": ["clip", "kind", "rate", "n_steps", "sigma", "key"], "formats": ["<i8", "<i4", "<f8", "<i4", "<f4", "<u8"],
                    "offsets": [0, 8, 16, 24, 28, 32], "itemsize": 40}
PAD_REFLECT, PAD_ZERO = 0, 1
AUGMENT_STRETCH, AUGMENT_PITCH, AUGMENT_NOISE = 0, 1, 2


class HostPipelineConfig(C.Structure):
    """dsp_host_pipeline_config"""
    _fields_ = [("chunk_bytes", C.c_long), ("depth", C.c_int), ("pageable_mode", C.c_int), ("classify_min_clips", C.c_int)]


class HostStats(C.Structure):
    """dsp_host_stats"""
    _fields_ = [("n_chunks", C.c_long), ("depth", C.c_int), ("input_path", C.c_int), ("output_path", C.c_int), ("bytes_h2d", C.c_long),
                ("bytes_d2h", C.c_long), ("peak_staging_bytes", C.c_long), ("pinned_ring_bytes", C.c_long)]


PAGEABLE_STAGE, PAGEABLE_REGISTER, PAGEABLE_DIRECT, PAGEABLE_WHOLE = 0, 1, 2, 3      # DSP_HOST_PAGEABLE_*
HOST_PATHS = ("staged", "pinned", "registered", "direct")      # DSP_HOST_PATH_*


class ClassifyTrace(C.Structure):
    """dsp_classify_trace (include/dsp_amd.h)."""

    _fields_ = [("n_midpoints", C.c_int), ("midpoints", C.c_float * 64), ("sums", (C.c_float * 3) * 64)]


class ClassifyConfig(C.Structure):
    """dsp_classify_config (include/dsp_amd.h): the thresholds the reference's classify() variants differ in."""

    _fields_ = [("keep_lo", C.c_float), ("keep_hi", C.c_float), ("midpoint_db", C.c_float),
                ("middle_max", C.c_float), ("above_min", C.c_float), ("below_min", C.c_float)]


class ClassifyConfigF64(C.Structure):
    """dsp_classify_config_f64: the same thresholds as doubles, for the float64 classifier (donut-classifier/classifier.c)."""

    _fields_ = [(k, C.c_double) for k in ("keep_lo", "keep_hi", "midpoint_db", "middle_max", "above_min", "below_min")]


class ClassifyTraceF64(C.Structure):
    _fields_ = [("n_midpoints", C.c_int), ("midpoints", C.c_double * 64), ("sums", (C.c_double * 3) * 64)]


WINDOW_HANN, WINDOW_HAMMING, WINDOW_RECT = 0, 1, 2
MELNORM_NONE, MELNORM_SLANEY, MELNORM_LIBROSA, MELNORM_AUBIO_SLANEY = 0, 1, 2, 3
LOG_PER_FRAME_MAX, LOG_GLOBAL_REF1, LOG_LOG10_FLOOR = 0, 1, 2
SPECTRUM_POWER, SPECTRUM_MAGNITUDE = 0, 1
FRAMING_COMPLETE, FRAMING_STREAM, FRAMING_CENTER = 0, 1, 2
MAP_RELEVANCE, MAP_FIXED_ALPHA = 0, 1
PREFILTER_NONE, PREFILTER_BUTTER_1000_3000, PREFILTER_BUTTER_3000_7500 = 0, 1, 2

LP = C.POINTER(C.c_long)

# Every function include/dsp_amd.h declares, in the header's order: name -> (restype, [argtypes]).  A new entry point is declared
# here, once; load() applies the table, SYMBOLS is its keys, and tests/test_bindings_cpu.py holds every entry to the header.
# The aliases: scalars (ip is int, lg long, fl float, db double), then pointers to them (ipp, lp, fp, dp) and to the structs above.
P = C.POINTER
vp, ip, lg, fl, db, u64, sz, cp = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double, C.c_uint64, C.c_size_t, C.c_char_p
vpp, ipp, lp, llp, fp, dp = P(vp), P(ip), LP, P(C.c_longlong), P(fl), P(db)
cfgp, scp, sgp, opp, smp, gp, gfp, urp, stcp = (P(MfccConfig), P(ScanConfig), P(SegmentConfig), P(AugmentOp), P(StopModelParams), P(GmmParams),
                                                P(GmmFloatParams), P(UbmResult), P(SvmTrainConfig))
ccfgp, ccfg64p = P(ClassifyConfig), P(ClassifyConfigF64)
PROTOTYPES = {
    "compute_mfcc": (ip, [vp, ip, vp, ip]),
    "dsp_classify": (ip, [vp, ip]),
    "dsp_mfcc_default_config": (None, [cfgp]),
    "dsp_mfcc_scrubjay_infer_config": (None, [cfgp, ip]),
    "dsp_mfcc_speaker_config": (None, [cfgp]),
    "dsp_mfcc_librosa_config": (None, [cfgp, ip, ip]),
    "dsp_mfcc_plan_create": (ip, [cfgp, ip, vpp]),
    "dsp_mfcc_plan_destroy": (None, [vp]),
    "dsp_mfcc_plan_config": (ip, [vp, cfgp]),
    "dsp_mfcc_frames_for": (ip, [cfgp, ip, ip]),
    "dsp_mfcc_frames_device": (ip, [vp, vp, lg, vp, vp]),
    "dsp_mfcc_clips_device": (ip, [vp, vp, lg, ip, lg, vp, ip, vp]),
    "fft_real_forward": (None, [vp, vp]),
    "dsp_fft_real_forward_host": (ip, [vp, lg, ip, lg, ip, vp]),
    "dsp_mfcc_clips_pcm16_device": (ip, [vp, vp, lg, ip, lg, ip, ip, vp, ip, vp]),
    "dsp_mfcc_ragged_frame_offsets": (lg, [cfgp, lp, lg, ip, lp]),
    "dsp_mfcc_clips_ragged_device": (ip, [vp, vp, lg, lp, ip, vp, vp]),
    "dsp_mfcc_clips_ragged_pcm16_device": (ip, [vp, vp, lg, lp, ip, ip, ip, vp, vp]),
    "dsp_mfcc_frames_host": (ip, [vp, vp, lg, vp]),
    "dsp_mfcc_clips_host": (ip, [vp, vp, lg, ip, lg, vp, ip]),
    "dsp_mfcc_clips_pcm16_host": (ip, [vp, vp, lg, ip, lg, ip, ip, vp, ip]),
    "dsp_mfcc_clips_ragged_host": (ip, [vp, vp, lg, lp, ip, vp]),
    "dsp_mfcc_clips_ragged_pcm16_host": (ip, [vp, vp, lg, lp, ip, ip, ip, vp]),
    "dsp_host_alloc": (ip, [ip, sz, vpp]),
    "dsp_host_free": (None, [vp]),
    "dsp_host_pipeline_set": (ip, [ip, P(HostPipelineConfig)]),
    "dsp_host_pipeline_get": (ip, [ip, P(HostPipelineConfig)]),
    "dsp_host_pipeline_release": (ip, [ip]),
    "dsp_host_pipeline_stats": (ip, [ip, P(HostStats)]),
    "dsp_host_plan_chunks": (lg, [lg, lg, lp, lg, lp, lg]),
    "dsp_mfcc_plan_set_launch": (ip, [vp, ip, ip]),
    "dsp_mfcc_plan_set_kernel": (ip, [vp, ip]),
    "dsp_butter_bandpass": (ip, [db, db, dp, dp]),
    "dsp_butter_bandpass_filter_f32": (ip, [vp, lg, ip, lg, vp, vp, vp]),
    "dsp_butter_bandpass_filter_f64": (ip, [vp, lg, ip, lg, vp, vp, vp]),
    "dsp_compute_spectrogram_f32": (ip, [vp, ip, ip, vp, vp, vp]),
    "dsp_compute_spectrogram_f64": (ip, [vp, ip, ip, vp, vp, vp]),
    "dsp_classify_batch_host": (ip, [vp, lg, ip, lg, vp, vp]),
    "dsp_classify_batch_device": (ip, [vp, lg, ip, lg, vp, vp]),
    "dsp_classify_default_config": (None, [ccfgp]),
    "dsp_classify_batch_host_cfg": (ip, [ccfgp, vp, lg, ip, lg, vp, vp]),
    "dsp_classify_batch_device_cfg": (ip, [ccfgp, vp, lg, ip, lg, vp, vp]),
    "dsp_classify_batch_pcm16_host": (ip, [ccfgp, vp, lg, ip, lg, ip, ip, vp, vp]),
    "dsp_classify_batch_pcm16_device": (ip, [ccfgp, vp, lg, ip, lg, ip, ip, vp, vp]),
    "dsp_classify_batch_ragged_device": (ip, [vp, vp, lg, lp, vp, vp]),
    "dsp_classify_batch_ragged_pcm16_device": (ip, [vp, vp, lg, lp, ip, ip, vp, vp]),
    "dsp_classify_batch_ragged_host": (ip, [vp, vp, lg, lp, vp, vp]),
    "dsp_classify_batch_ragged_pcm16_host": (ip, [vp, vp, lg, lp, ip, ip, vp, vp]),
    "dsp_classify_stats": (ip, [ip, lp, lp]),
    "dsp_classify_ctx_create": (ip, [ip, vpp]),
    "dsp_classify_ctx_destroy": (None, [vp]),
    "dsp_classify_batch_device_ctx": (ip, [vp, ccfgp, vp, lg, ip, lg, vp, vp]),
    "dsp_debug_hold_classify_ctx": (ip, [ip, ip]),
    "dsp_classify_release": (ip, [ip]),
    "dsp_classify_default_config_f64": (None, [ccfg64p]),
    "dsp_classify_batch_host_f64": (ip, [ccfg64p, vp, lg, ip, lg, vp, vp]),
    "dsp_classify_batch_device_f64": (ip, [ccfg64p, vp, lg, ip, lg, vp, vp, vp]),
    "dsp_classify_batch_pcm16_host_f64": (ip, [ccfg64p, vp, lg, ip, lg, ip, ip, vp, vp]),
    "dsp_classify_batch_pcm16_device_f64": (ip, [ccfg64p, vp, lg, ip, lg, ip, ip, vp, vp, vp]),
    "dsp_classify_batch_ragged_device_f64": (ip, [vp, vp, lg, lp, vp, vp, vp]),
    "dsp_classify_batch_ragged_pcm16_device_f64": (ip, [vp, vp, lg, lp, ip, ip, vp, vp, vp]),
    "dsp_classify_batch_ragged_host_f64": (ip, [vp, vp, lg, lp, vp, vp]),
    "dsp_classify_batch_ragged_pcm16_host_f64": (ip, [vp, vp, lg, lp, ip, ip, vp, vp]),
    "dsp_classify_stats_f64": (ip, [ip, lp, lp, lp]),
    "dsp_classify_debug_f64": (ip, [ip, ipp, ip]),
    "dsp_classify_release_f64": (ip, [ip]),
    "dsp_sum_intense_f32": (ip, [fl, fl, fl, vp, ip, vp, ip, vp, fl, fp]),
    "dsp_find_midpoints": (ip, [vp, ip, ip, vp, ip]),
    "dsp_gather_create": (ip, [vp, ip, vpp]),
    "dsp_gather_destroy": (None, [vp]),
    "dsp_gather_n_devices": (ip, [vp]),
    "dsp_gather_all": (ip, [vp, vp, vp, sz, vp]),
    "dsp_mfcc_stats_device": (ip, [vp, lg, ip, ip, vp, vp]),
    "dsp_svm_create": (ip, [ip, ip, ip, vp, vp, vp, vp, fl, fl, fl, fl, vpp]),
    "dsp_svm_destroy": (None, [vp]),
    "dsp_svm_predict_device": (ip, [vp, vp, lg, vp, vp, vp, vp]),
    "dsp_scrubjay_fused_device": (ip, [vp, vp, vp, lg, ip, lg, ip, vp, vp, vp, vp, vp]),
    "dsp_scrubjay_fused_pcm16_device": (ip, [vp, vp, vp, lg, ip, lg, ip, ip, ip, vp, vp, vp, vp, vp]),
    "dsp_scrubjay_fused_ragged_device": (ip, [vp, vp, vp, lg, lp, ip, vp, vp, vp, vp, vp]),
    "dsp_scrubjay_fused_ragged_pcm16_device": (ip, [vp, vp, vp, lg, lp, ip, ip, ip, vp, vp, vp, vp, vp]),
    "dsp_debug_fused_spans": (ip, [cfgp, lp, lg, ip, lg, lp]),
    "dsp_stop_model_create": (ip, [smp, ip, vpp]),
    "dsp_stop_model_destroy": (None, [vp]),
    "dsp_stop_predict_device": (ip, [vp, vp, lg, ip, vp, vp]),
    "dsp_classify_signal_batch_device": (ip, [vp, vp, vp, lg, ip, lg, vp, vp]),
    "dsp_classify_signal_batch_pcm16_device": (ip, [vp, vp, vp, lg, ip, lg, ip, ip, vp, vp]),
    "dsp_classify_signal_batch_ragged_device": (ip, [vp, vp, vp, lg, lp, vp, vp]),
    "dsp_classify_signal_batch_ragged_pcm16_device": (ip, [vp, vp, vp, lg, lp, ip, ip, vp, vp]),
    "dsp_classify_signal": (fl, [vp, vp, ip]),
    "dsp_speaker_model_create": (ip, [gp, gp, ip, vpp]),
    "dsp_speaker_model_destroy": (None, [vp]),
    "dsp_speaker_llr_device": (ip, [vp, vp, lg, ip, vp, vp, vp, vp, vp]),
    "dsp_speaker_llr_ragged_device": (ip, [vp, vp, lg, lp, vp, vp, vp, vp, vp]),
    "dsp_scan_window_offsets": (lg, [scp, lp, lg, lp]),
    "dsp_stop_scan_device": (ip, [vp, vp, lg, lp, scp, vp, vp]),
    "dsp_speaker_scan_device": (ip, [vp, vp, lg, lp, scp, vp, vp, vp]),
    "dsp_scanner_create": (ip, [vp, vp, vp, scp, vpp]),
    "dsp_scanner_destroy": (None, [vp]),
    "dsp_scanner_run_device": (ip, [vp, vp, lg, lp, vp, vp, vp, vp]),
    "dsp_scanner_run_pcm16_device": (ip, [vp, vp, lg, lp, ip, ip, vp, vp, vp, vp]),
    "dsp_scan_window_spans": (lg, [cfgp, scp, lp, lg, lp, lp]),
    "dsp_svm_scan_device": (ip, [vp, vp, lg, lp, scp, vp, vp, vp, vp, vp]),
    "dsp_scrubjay_scanner_create": (ip, [vp, vp, scp, vpp]),
    "dsp_scrubjay_scanner_destroy": (None, [vp]),
    "dsp_scrubjay_scanner_run_device": (ip, [vp, vp, lg, lp, vp, vp, vp, vp, vp]),
    "dsp_scrubjay_scanner_run_pcm16_device": (ip, [vp, vp, lg, lp, ip, ip, vp, vp, vp, vp, vp]),
    "dsp_stream_push_plan": (lg, [cfgp, scp, lp, lp, lg, lp, lp]),
    "dsp_stream_session_create": (ip, [vp, vp, vp, scp, lg, ip, ip, ip, vpp]),
    "dsp_stream_session_destroy": (None, [vp]),
    "dsp_stream_session_reset": (ip, [vp, lp, lg, vp]),
    "dsp_stream_session_counts": (ip, [vp, lp, lp, lp]),
    "dsp_stream_push_device": (ip, [vp, vp, lp, vp, vp, vp, vp, lp, lp, vp]),
    "dsp_stream_resample_plan": (lg, [ip, ip, lp, lp, lg, lp]),
    "dsp_stream_resampler_create": (ip, [ip, ip, ip, lg, ip, ip, ip, vpp]),
    "dsp_stream_resampler_destroy": (None, [vp]),
    "dsp_stream_resampler_reset": (ip, [vp, lp, lg, vp]),
    "dsp_stream_resampler_counts": (ip, [vp, lp, lp]),
    "dsp_stream_resample_push_device": (ip, [vp, vp, lp, vp, lp, vp]),
    "dsp_stream_resample_finish_device": (ip, [vp, lp, lg, vp, lp, vp]),
    "dsp_stream_session_attach_resampler": (ip, [vp, vp]),
    "dsp_upsample_linear_device": (ip, [vp, lg, ip, lg, vp, ip, lg, vp]),
    "dsp_upsample_linear_host": (ip, [vp, ip, vp, ip]),
    "dsp_resample_ratio": (ip, [ip, ip, ipp, ipp, ipp]),
    "dsp_resample_geometry": (ip, [ip, ip, ipp, ip]),
    "dsp_resample_taps": (ip, [ip, ip, dp, ip]),
    "dsp_resample_offsets": (lg, [ip, ip, lp, lg, lp]),
    "dsp_resampler_create": (ip, [ip, ip, ip, vpp]),
    "dsp_resampler_destroy": (None, [vp]),
    "dsp_resample_ragged_device": (ip, [vp, vp, lg, lp, vp, vp]),
    "dsp_resample_ragged_pcm16_device": (ip, [vp, vp, lg, lp, ip, ip, vp, vp]),
    "dsp_resample_clips_device": (ip, [vp, vp, lg, ip, lg, vp, lg, vp]),
    "dsp_resample_clips_pcm16_device": (ip, [vp, vp, lg, ip, lg, ip, ip, vp, lg, vp]),
    "dsp_resample_host": (ip, [ip, ip, vp, lg, vp]),
    "dsp_cmvn_create": (ip, [ip, ip, ip, vpp]),
    "dsp_cmvn_destroy": (None, [vp]),
    "dsp_cmvn_ragged_device": (ip, [vp, vp, lg, lp, vp, vp]),
    "dsp_speaker_enroller_create": (ip, [gfp, ip, vpp]),
    "dsp_speaker_enroller_destroy": (None, [vp]),
    "dsp_speaker_enroll_ragged_device": (ip, [vp, vp, lg, lp, P(EnrollConfig), vp, vp, vp, vp, vp, vp]),
    "dsp_ubm_trainer_create": (ip, [ip, ip, ip, vpp]),
    "dsp_ubm_trainer_destroy": (None, [vp]),
    "dsp_ubm_init_rows_device": (ip, [vp, vp, lg, db, vp, vp, vp, vp]),
    "dsp_ubm_train_device": (ip, [vp, vp, lg, P(UbmInit), P(UbmConfig), urp, vp]),
    "dsp_gmm_quantize": (ip, [gfp, vp, vp, vp, ipp]),
    "dsp_kmeans_seed_device": (ip, [vp, vp, lg, u64, vp, vp]),
    "dsp_kmeans_fit_device": (ip, [vp, vp, lg, vp, P(KmeansConfig), P(KmeansResult), vp]),
    "dsp_kmeans_train_ubm_device": (ip, [vp, vp, lg, P(KmeansUbmConfig), urp, P(KmeansUbmReport), vp]),
    "dsp_speaker_verifier_create": (ip, [gfp, ip, vpp]),
    "dsp_speaker_verifier_destroy": (None, [vp]),
    "dsp_speaker_verify_ragged_device": (ip, [vp, vp, lg, lp, vp, lg, vp, vp, vp, vp, vp, vp]),
    "dsp_speaker_float_scan_device": (ip, [vp, vp, lg, lp, scp, vp, lg, vp, vp, vp, vp, vp, vp]),
    "dsp_segmenter_create": (ip, [ip, vpp]),
    "dsp_segmenter_destroy": (None, [vp]),
    "dsp_segments_capacity": (lg, [sgp, lp, lg, lg]),
    "dsp_segments_device": (ip, [vp, vp, lg, lp, lg, sgp, vp, lg, vp, vp, vp]),
    "dsp_segment_sample_spans": (lg, [cfgp, scp, lp, lg, vp, lg, lp, lp]),
    "dsp_trials_target_offsets": (lg, [ipp, lg, lg, lp, lp]),
    "dsp_trials_pairs": (lg, [ipp, lg, lg]),
    "dsp_trial_evaluator_create": (ip, [ip, vpp]),
    "dsp_trial_evaluator_destroy": (None, [vp]),
    "dsp_trials_evaluate_device": (ip, [vp, vp, lg, lg, ipp, P(TrialsConfig), vp, vp, vp, vp, vp, vp]),
    "dsp_calibrator_create": (ip, [ip, vpp]),
    "dsp_calibrator_destroy": (None, [vp]),
    "dsp_calibration_duration_term": (ip, [lp, lg, dp]),
    "dsp_calibration_fit_device": (ip, [vp, vp, lg, lg, ipp, lp, P(CalibrationConfig), P(Calibration), P(CalibrationReport), vp]),
    "dsp_calibration_apply_device": (ip, [vp, vp, lg, lg, lp, P(Calibration), vp, vp]),
    "dsp_cohort_stats_device": (ip, [ip, vp, lg, lg, ip, ip, vp, vp]),
    "dsp_score_normalize_device": (ip, [ip, vp, lg, lg, vp, vp, P(SnormConfig), vp, vp]),
    "dsp_vad_default_config": (None, [cfgp, P(VadConfig)]),
    "dsp_vad_ratio_from_db": (db, [db]),
    "dsp_vad_geometry_for": (ip, [P(VadConfig), P(VadGeometry)]),
    "dsp_vad_workspace_bytes": (lg, [lg, lg]),
    "dsp_vad_frame_power_ragged_device": (ip, [ip, P(VadConfig), vp, lg, lp, lp, vp, vp, lg, vp]),
    "dsp_vad_decide_ragged_device": (ip, [ip, P(VadConfig), vp, lg, lp, vp, vp, vp, lp, vp, lg, vp]),
    "dsp_vad_run_ragged_device": (ip, [ip, P(VadConfig), vp, lg, lp, lp, vp, vp, vp, lp, vp, lg, vp]),
    "dsp_rows_kept_offsets_device": (ip, [ip, vp, lg, lp, lp, vp, lg, vp]),
    "dsp_rows_select_ragged_device": (ip, [ip, vp, ip, vp, lg, lp, lp, vp, vp, vp, lg, vp]),
    "dsp_vad_trim_spans": (lg, [P(VadConfig), lp, lg, vp, lp, lp]),
    "dsp_svm_trainer_create": (ip, [ip, ip, vpp]),
    "dsp_svm_trainer_destroy": (None, [vp]),
    "dsp_svm_train_set_device": (ip, [vp, vp, lg, vp, lg, vp, vp, vp, vp, vp]),
    "dsp_svm_train_problems_device": (ip, [vp, P(SvmTrainProblem), lg, stcp, vp, vp, vp, vp, vp]),
    "dsp_svm_platt_fit_device": (ip, [vp, vp, vp, vp, lg, dp, dp, ipp, vp]),
    "dsp_svm_folds": (ip, [lg, ip, u64, vp]),
    "dsp_svm_balanced_weights": (ip, [vp, vp, lg, db, dp, dp]),
    "dsp_svm_model_from_training": (lg, [vp, vp, vp, lg, ip, vp, vp, lg, lp]),
    "dsp_svm_fit_device": (ip, [vp, vp, lg, vp, vp, ip, u64, db, db, db, stcp, P(SvmFitModel), vp]),
    "dsp_svm_train_rows_host": (ip, [vp, vp, vp]),
    "dsp_stop_trainer_create": (ip, [ip, ip, ip, ipp, vpp]),
    "dsp_stop_trainer_destroy": (None, [vp]),
    "dsp_stop_train_set_device": (ip, [vp, vp, lg, vp, vp, lg, vp, vp, vp, vp, vp]),
    "dsp_stop_train_used_features": (lg, [vp]),
    "dsp_stop_train_rows_host": (ip, [vp, vp, vp]),
    "dsp_stop_train_runs_device": (ip, [vp, P(StopTrainRun), lg, vp, vp, vp, vp, vp, vp]),
    "dsp_stop_train_param_count": (lg, [ip, ip, ipp]),
    "dsp_stop_train_uniform": (db, [u64, u64, u64]),
    "dsp_stop_train_order": (ip, [lg, u64, lg, vp]),
    "dsp_stop_train_init": (ip, [ip, ip, ipp, u64, vp]),
    "dsp_stop_model_from_training": (ip, [ip, ip, ipp, vp, vp, vp, vp, smp]),
    "dsp_stft_frames": (lg, [lg]),
    "dsp_stretch_frames": (lg, [lg, db]),
    "dsp_stretch_length": (lg, [lg, db]),
    "dsp_pitch_ratio": (ip, [ip, ip, ip, ipp, ipp]),
    "dsp_augment_normal": (db, [u64, u64, u64]),
    "dsp_augment_out_offsets": (lg, [lp, lg, opp, lg, lp]),
    "dsp_augment_draw": (lg, [u64, ipp, lg, db, opp, lg]),
    "dsp_augmenter_create": (ip, [ip, ip, ip, vpp]),
    "dsp_augmenter_destroy": (None, [vp]),
    "dsp_stft_ragged_device": (ip, [vp, vp, lg, lp, vp, lp, vp]),
    "dsp_istft_ragged_device": (ip, [vp, vp, lg, lp, lp, vp, lp, vp]),
    "dsp_time_stretch_ragged_device": (ip, [vp, vp, lg, lp, dp, vp, vp]),
    "dsp_augment_ragged_device": (ip, [vp, vp, lg, lp, opp, lg, u64, vp, vp]),
    "dsp_mfcc_tables": (ip, [cfgp, vp, vp, vp]),
    "dsp_mfcc_lane_tables": (ip, [cfgp, vp, ip]),
    "dsp_mfcc400_tables": (ip, [cfgp, vp, ip]),
    "dsp_mfcc1024_tables": (ip, [cfgp, vp, ip]),
    "dsp_mfcc2048_tables": (ip, [cfgp, vp, ip]),
    "dsp_classify_division_check": (ip, [llp]),
    "dsp_prefilter_scan_check": (ip, [ip, ipp]),
    "dsp_last_error": (cp, []),
    "dsp_device_count": (ip, []),
    "dsp_version": (cp, []),
    "dsp_abi_sizeof": (ip, [ip]),
}
SYMBOLS = list(PROTOTYPES)      # (a list: tests pick entries by prefix)

# the reference's own C++-linkage names (sync/lib/classifier.h:14-19, include/dsp_amd_classifier.h), Itanium-mangled
CXX_SYMBOLS = {
    "butter_bandpass": "_Z15butter_bandpassffPfS_",
    "butter_bandpass_filter": "_Z22butter_bandpass_filterPfiS_S_S_",
    "compute_spectrogram": "_Z19compute_spectrogramPfiiPS_S0_PS0_PiS2_",
    "sum_intense": "_Z11sum_intensefffPfiS_iPS_f",
    "find_midpoints": "_Z14find_midpointsPfiiPi",
    "classify": "_Z8classifyPfi",
}

_lib = None


def load() -> C.CDLL:
    """Load (building first if the sources are newer) the in-tree libdsp_amd.so."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    explicit = bool(os.environ.get("DSP_AMD_LIB"))               # an explicit DSP_AMD_LIB is loaded as is
    if not explicit and _build.is_stale():
        try:
            _build.build()
        except Exception as e:  # noqa: BLE001  (never fall back to an older binary: it would pass for the current source)
            raise DspError(f"libdsp_amd.so is stale or missing and could not be rebuilt: {e}") from e
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own
    # libamdhip64.so (SONAME libamdhip64.so.7, the same as /opt/rocm's).  If torch is
    # going to share streams and HBM buffers with this library it must be loaded
    # first, so that our DT_NEEDED libamdhip64.so.7 binds to the runtime torch
    # already brought in instead of a second copy from /opt/rocm.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001  (pure C-ABI use without torch is fine)
        pass
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise DspError(f"cannot load {path}: {e} (the HIP extension is required; there is no fallback)") from e
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    for which, mirror in ((0, MfccConfig), (1, ClassifyTrace), (2, ClassifyTraceF64)):      # the ctypes mirrors against the library's own structs
        if L.dsp_abi_sizeof(which) != C.sizeof(mirror):
            raise DspError(f"{path}: struct {mirror.__name__} is {L.dsp_abi_sizeof(which)} bytes in the library, {C.sizeof(mirror)} in dsp_amd/lib.py")
    if not explicit:
        # the binary says which sources it was built from: a mismatch means the mtime check was fooled (copied tree,
        # clock skew) and the library on disk is not the code in dsp_amd/csrc
        built = L.dsp_version().decode().rsplit("src:", 1)[-1]
        if built != _build.source_hash():
            raise DspError(f"{path} was built from other sources (library {built}, tree {_build.source_hash()}): "
                           "rebuild with `python -m dsp_amd.build`")
    _lib = L
    return L


def last_error() -> str:
    return load().dsp_last_error().decode()


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise DspError(f"{what} failed ({rc}): {last_error()}")
    return rc


def current_stream(where):
    """torch's current stream on `where` -- a CUDA tensor (its device) or a device index -- as the stream argument of the entry points."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(getattr(where, "device", where)).cuda_stream)


class Closing:
    """What every owner of native handles shares: close() when a `with` block ends and when the object is collected."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Handle(Closing):
    """An object that owns one native handle, self._h, of the library self._L: made by a dsp_*_create, destroyed once by the function
    `_destroy` names.  The class defaults leave an object whose constructor raised closable."""

    _destroy = None
    _h = None
    _L = None

    def _create(self, name: str, *args):
        """self._h = the handle `name`(*args, &handle) makes (every create function takes its out-handle last), or DspError"""
        self._L = load()
        h = C.c_void_p()
        check(getattr(self._L, name)(*args, C.byref(h)), name)
        self._h = h

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def _stream(self):
        return current_stream(self.device)


def host_array(x, dtype):
    """A host buffer for a *_host entry: a numpy array or a CPU torch tensor -> a C-contiguous numpy array of `dtype`, the SAME memory
    where x already is one (a pinned tensor stays pinned: the copy engines read it directly), a converted copy otherwise."""
    import numpy as np
    if not isinstance(x, np.ndarray) and hasattr(x, "is_cuda"):
        if x.is_cuda:
            raise ValueError("a host entry takes host memory: a numpy array or a CPU tensor")
        x = x.detach().numpy()
    return np.ascontiguousarray(x, dtype)


def torch_int16():
    """torch.int16, or None where torch is not importable (a dtype to compare a tensor's against)"""
    try:
        import torch
        return torch.int16
    except Exception:  # noqa: BLE001
        return None


def c_offsets(offsets):
    """offsets[n_clips + 1] (any integer sequence) -> (ctypes long array, n_clips) for the *_ragged_* entry points."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if a.ndim != 1 or a.size < 1:
        raise ValueError("offsets must hold n_clips + 1 positions")
    return (C.c_long * a.size)(*a.tolist()), a.size - 1


def clips_device(clips, dtype):
    """Equal clips on the GPU: a `dtype` CUDA tensor [n_clips][n] with unit inner stride, or ValueError."""
    import torch
    if not (isinstance(clips, torch.Tensor) and clips.is_cuda and clips.dtype == dtype and clips.dim() == 2 and clips.stride(1) == 1):
        raise ValueError(f"clips must be a {str(dtype).replace('torch.', '')} CUDA tensor [n_clips][n] with unit inner stride")
    return clips


def pcm_device(pcm):
    """cuda int16 [n_clips][n] or interleaved [n_clips][n][2] -> (channels, clip stride in samples per channel), or ValueError."""
    import torch
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() in (2, 3) and pcm.stride(-1) == 1):
        raise ValueError("pcm must be an int16 CUDA tensor [n_clips][n] or [n_clips][n][2] with unit inner stride")
    channels = 2 if pcm.dim() == 3 else 1
    if channels == 2 and (pcm.shape[2] != 2 or pcm.stride(1) != 2 or pcm.stride(0) % 2):
        raise ValueError("stereo pcm must be interleaved [n_clips][n][2]")
    return channels, pcm.stride(0) // channels


def long_array(a, size, what):
    """Any integer sequence -> a contiguous int64 array of exactly `size` entries, or ValueError."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
    if a.ndim != 1 or a.size != size:
        raise ValueError(f"{what} must hold {size} entries")
    return a


def offsets_array(a, what, unit):
    """The prefix offsets of the recordings of a ragged matrix (`what`: "frame_offsets" in "rows", "window_offsets" in "windows"): any
    integer sequence -> a contiguous int64 array of n_recordings + 1 entries that start at >= 0 and never fall, or ValueError."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
    if a.ndim != 1 or a.size < 1:
        raise ValueError(f"{what} must hold n_recordings + 1 {unit}")
    if a[0] < 0 or (a.size > 1 and (np.diff(a) < 0).any()):
        raise ValueError(f"{what} must be non-negative and non-decreasing")
    return a


def stream_chunks(chunks, chunk_offsets, n_streams, dtype, channels, device):
    """The chunks of one push on the GPU: a contiguous CUDA tensor of `dtype` on cuda:`device`, [total] (channels 1) or interleaved
    [total][2] (channels 2), stream s's chunk = sample frames [chunk_offsets[s], chunk_offsets[s + 1]).  -> chunk_offsets as a contiguous
    int64 array of n_streams + 1, or ValueError."""
    import numpy as np
    import torch
    if not (isinstance(chunks, torch.Tensor) and chunks.is_cuda and chunks.is_contiguous()):
        raise ValueError("chunks must be a contiguous CUDA tensor")
    if chunks.dtype != dtype:
        raise ValueError(f"chunks must be {str(dtype).replace('torch.', '')}, as the object was created")
    if chunks.device.index != device:
        raise ValueError(f"chunks must live on the object's device (cuda:{device})")
    if not (chunks.dim() == 1 if channels == 1 else (chunks.dim() == 2 and chunks.shape[1] == 2)):
        raise ValueError("chunks must be [total] (mono) or [total][2] (interleaved stereo), as the object was created")
    co = long_array(chunk_offsets, n_streams + 1, "chunk_offsets")
    if co[0] < 0 or (np.diff(co) < 0).any():
        raise ValueError("chunk_offsets must be non-negative and non-decreasing")
    if int(co[-1]) > chunks.shape[0]:
        raise ValueError("chunk_offsets run past the end of chunks")
    return co


def stream_format(dtype, channels, stereo_mode, n_streams):
    """The sample format of a stream object: torch.float32 mono, or torch.int16 with 1 or 2 interleaved channels.  -> (dtype, channels,
    stereo_mode, n_streams, pcm16 flag) as ints, or ValueError."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.int16):
        raise ValueError("dtype must be torch.float32 or torch.int16")
    if int(n_streams) < 0:
        raise ValueError("n_streams must be >= 0")
    if channels not in (1, 2) or (channels == 2 and dtype != torch.int16):
        raise ValueError("channels must be 1, or 2 for int16 PCM")
    if stereo_mode not in (0, 1):
        raise ValueError("stereo_mode must be 0 (channel 0) or 1 (average)")
    return dtype, int(channels), int(stereo_mode), int(n_streams), int(dtype == torch.int16)


def ragged_signal(signal, offsets, float_dtype):
    """A ragged batch on the GPU: `signal` a contiguous CUDA tensor -- float_dtype [total], int16 [total] or interleaved int16 [total][2] --
    and clip c = samples [offsets[c], offsets[c + 1]) per channel (offsets as c_offsets takes them, or the (array, n_clips) pair it
    returned: no conversion per call).  -> (offsets array, n_clips, channels (0: float samples), signal pointer), or ValueError."""
    import torch
    off, n = offsets if isinstance(offsets, tuple) else c_offsets(offsets)
    if not (isinstance(signal, torch.Tensor) and signal.is_cuda and signal.is_contiguous()):
        raise ValueError("signal must be a contiguous CUDA tensor")
    if signal.dtype == torch.int16:
        if not (signal.dim() == 1 or (signal.dim() == 2 and signal.shape[1] == 2)):
            raise ValueError("int16 signal must be [total] (mono) or [total][2] (interleaved stereo)")
        channels = signal.dim()
    elif signal.dtype == float_dtype:
        if signal.dim() != 1:
            raise ValueError("float signal must be 1-D [total]")
        channels = 0
    else:
        raise ValueError(f"signal must be {str(float_dtype).replace('torch.', '')} or int16")
    if n and int(off[n]) > signal.shape[0]:
        raise ValueError("offsets run past the end of the signal")
    return off, n, channels, signal.data_ptr()


def scores_device(scores, device: int, who: str = "segmenter"):
    """Window scores on the GPU: a float32 CUDA tensor [Wt] or [Wt][S] (S >= 1) on GPU `device`, made contiguous -> (scores, S), or
    ValueError.  `who` names the owner in the message: the segmenter, or the evaluator, whose rows are trials (Wt = T)."""
    import torch
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32 and scores.dim() in (1, 2)):
        raise ValueError("scores must be a float32 CUDA tensor [Wt] or [Wt][S]")
    if scores.device.index != device:
        raise ValueError(f"scores are on GPU {scores.device.index}, the {who} on GPU {device}")
    n_col = scores.shape[1] if scores.dim() == 2 else 1
    if n_col < 1:
        raise ValueError("scores must have at least one column")
    return scores.contiguous(), n_col
