"""dsp_amd -- MI355X-native MFCC / Butterworth / spectrogram hot path of
cornell-c2s2/dsp behind the reference's C entry points (include/dsp_amd.h).

Python here is plumbing over the C ABI (ctypes) plus torch for HBM buffers,
streams and torch.distributed; all arithmetic runs in the HIP kernels of
dsp_amd/csrc.  Importing the package does not need a GPU; calling into it does.
"""
from .lib import DspError, MfccConfig, load  # noqa: F401
from .classify import (CLASSIFY_DONUT_C, CLASSIFY_MICROPHONE, CLASSIFY_MICROPHONE_C, CLASSIFY_SYNC_LIB, butter_bandpass, butter_bandpass_filter, classify, classify_batch,  # noqa: F401
                       classify_batch_f64, classify_batch_f64_pcm16, classify_batch_pcm16, classify_device_pcm16, classify_release, classify_ragged, classify_device_ragged, classify_ragged_f64, classify_device_ragged_f64, classify_config, classify_device, classify_device_f64, classify_device_f64_pcm16,
                       classify_release_f64, classify_stats_f64, compute_spectrogram, find_midpoints, STEREO_AVERAGE, STEREO_CHANNEL0)
from .mfcc import MfccPlan, compute_mfcc, default_config, frames_for, host_pipeline, host_pipeline_release, host_pipeline_stats, plan_host_chunks, ragged_frame_offsets, speaker_config, librosa_config, tables  # noqa: F401
from .consumers import Cmvn, Scanner, ScoreCalibrator, ScoreNormalizer, Segmenter, segment_sample_spans, segments_capacity, SpeakerEnroller, SpeakerFrontEnd, SpeakerModel, SpeakerVerifier, StopModel, StopTrainer, StreamSession, TrialEvaluator, UbmTrainer, Vad, roc_points, trial_thresholds, quantize_gmm, scan_window_offsets, stop_model_from_training, stop_train_init, stop_train_order, stop_train_param_count, stop_train_uniform, stream_push_plan, upsample_linear  # noqa: F401
from .resample import Resampler, StreamResampler, resample_geometry, resample_offsets, resample_ratio, resample_taps, stream_resample_plan  # noqa: F401
from .augment import Augmenter, augment_draw, augment_normal, augment_out_offsets, pitch_ratio, stft_frames, stretch_frames, stretch_length  # noqa: F401

__all__ = ["DspError", "MfccConfig", "MfccPlan", "compute_mfcc", "default_config", "speaker_config", "librosa_config", "frames_for", "ragged_frame_offsets", "tables", "load", "host_pipeline", "host_pipeline_stats", "host_pipeline_release", "plan_host_chunks",
           "butter_bandpass", "butter_bandpass_filter", "compute_spectrogram", "find_midpoints", "classify", "classify_batch", "classify_batch_f64", "classify_device", "classify_device_f64", "classify_batch_f64_pcm16", "classify_batch_pcm16", "classify_device_pcm16", "classify_release", "classify_ragged", "classify_device_ragged", "classify_ragged_f64", "classify_device_ragged_f64", "classify_device_f64_pcm16", "classify_stats_f64", "classify_release_f64", "STEREO_CHANNEL0", "STEREO_AVERAGE", "classify_config", "CLASSIFY_SYNC_LIB", "CLASSIFY_MICROPHONE", "CLASSIFY_MICROPHONE_C", "CLASSIFY_DONUT_C",
           "StopModel", "SpeakerModel", "Scanner", "StreamSession", "Cmvn", "SpeakerFrontEnd", "SpeakerEnroller", "SpeakerVerifier", "UbmTrainer", "quantize_gmm", "scan_window_offsets", "stream_push_plan", "upsample_linear", "Segmenter", "segments_capacity", "segment_sample_spans", "TrialEvaluator", "trial_thresholds", "roc_points", "ScoreCalibrator", "ScoreNormalizer", "Vad",
           "Resampler", "resample_ratio", "resample_geometry", "resample_taps", "resample_offsets", "StreamResampler", "stream_resample_plan",
           "Augmenter", "augment_draw", "augment_normal", "augment_out_offsets", "pitch_ratio", "stft_frames", "stretch_frames", "stretch_length"]
