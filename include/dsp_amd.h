/*
 * dsp_amd.h -- C ABI of libdsp_amd.so: the MI355X (gfx950) MFCC / Butterworth /
 * spectrogram hot path of cornell-c2s2/dsp behind the reference's own C entry
 * points.  Plain C: pointers and sizes only, no torch / HIP types (streams are
 * passed as void*).
 *
 * Section 1 are the reference's symbols, bit-for-bit the same signatures, so the
 * library links in place of the reference's mfcc.c / classifier.cpp object
 * files.  Section 2 are batch / device-resident extensions the reference does
 * not have; the Section-1 symbols are thin wrappers over them.
 *
 * Reference paths are relative to the upstream repository root.
 * Error convention: Section-1 functions keep the reference's return values
 * (frame count / 0-1 label, 0 on failure) and never change them to signal GPU
 * trouble; the cause is readable through dsp_last_error().  Section-2 functions
 * return >= 0 on success and a negative DSP_E* code on failure.
 */
#ifndef DSP_AMD_H
#define DSP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the functions declared between this push and
 * the matching pop (plus the C++-linkage reference names of dsp_amd_classifier.h) are exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* ===================================================================== */
/* 1. Reference entry points (drop-in)                                    */
/* ===================================================================== */

/* Replaces 2fa/audio/word/c/mfcc.h:16-19 (definition mfcc.c:108-232; identical
 * copy 2fa/audio/pico-audio/src/mfcc.c).  Mono float PCM in [-1,1] at 16 kHz
 * -> frame-major out_mfcc[T][13], T = min(max_frames, 1 + (n-400)/160);
 * returns T, 0 when num_samples < 400 or max_frames <= 0 (mfcc.c:117-119).
 * Caller owns both buffers (host memory); out_mfcc holds max_frames*13 floats. */
int compute_mfcc(const float *signal, int num_samples, float *out_mfcc, int max_frames);

/* Replaces sync/lib/classifier.h:19 (definition classifier.cpp:9-136; fp32 firmware
 * twin of donut-classifier/classifier.c:30-212).  16 kHz mono clip -> 1 if the scrub-jay
 * rule fires, else 0 (also 0 on internal failure, classifier.cpp:87-91).  The reference
 * header is C++ without extern "C": this is the C symbol; the C++-linkage `int classify(float*, int)`
 * that sync.cpp links against is exported too and declared in dsp_amd_classifier.h, next to
 * butter_bandpass, butter_bandpass_filter, compute_spectrogram, sum_intense and find_midpoints
 * (classifier.h:14-18).  Caller owns `data` (host memory); nothing is printed unless the
 * environment variable DSP_AMD_VERBOSE is set.                                      */
int dsp_classify(float *data, int data_size);

/* ===================================================================== */
/* 2. Extensions                                                          */
/* ===================================================================== */

enum {
    DSP_OK = 0,
    DSP_EINVAL = -1,      /* bad argument / unsupported configuration      */
    DSP_ENODEV = -2,      /* no usable HIP device                           */
    DSP_EHIP = -3,        /* a HIP runtime call failed (see dsp_last_error) */
    DSP_ENOMEM = -4
};

enum { DSP_WINDOW_HANN = 0, DSP_WINDOW_HAMMING = 1, DSP_WINDOW_RECT = 2 };
enum { DSP_MELNORM_NONE = 0, DSP_MELNORM_SLANEY = 1,       /* HTK mel scale, triangles of peak 1 / of unit area          */
       DSP_MELNORM_LIBROSA = 2,                             /* Slaney mel scale + unit area: librosa.filters.mel defaults */
       DSP_MELNORM_AUBIO_SLANEY = 3 };                      /* aubio_filterbank_set_mel_coeffs_slaney (what new_aubio_mfcc picks for 40
                                                               filters, cepstrum/scrubjay_infer.c:30): Slaney's Auditory-Toolbox bank, 13
                                                               linear + 27 log-spaced unit-area triangles, 133 Hz .. 6.85 kHz; n_mels must
                                                               be 40, fmin / fmax are not used; n_fft 2048                              */
enum { DSP_LOG_PER_FRAME_MAX = 0,    /* mfcc.c:169-206: reference = the frame's own maximum                                    */
       DSP_LOG_GLOBAL_REF1 = 1,      /* librosa power_to_db(ref = 1, top_db below the CLIP's maximum); n_fft 512 and 2048      */
       DSP_LOG_LOG10_FLOOR = 2 };    /* aubio fvec_log10 (aubio_mfcc_do): plain log10 of each filter output, inputs below 2e-42
                                        count as 2e-42; no dB factor, no reference, no top_db; n_fft 2048                      */
enum { DSP_SPECTRUM_POWER = 0,       /* mfcc.c:151-155: |X[k]|^2 into the filterbank                                             */
       DSP_SPECTRUM_MAGNITUDE = 1 }; /* aubio: the phase vocoder's norm |X[k]| (aubio_fft_get_norm), filterbank power 1; n_fft 2048 */
enum { DSP_FRAMING_COMPLETE = 0,     /* mfcc.c:132-139: frames that lie completely inside the clip, T = 1 + (n - frame) / hop    */
       DSP_FRAMING_STREAM = 1,       /* aubio_source_do + aubio_pvoc_do as cepstrum/scrubjay_infer.c:39-53 drives them: one frame per
                                        hop of NEW samples, T = ceil(n / hop); frame t ends with hop t and starts frame_length - hop
                                        samples earlier (zeros before the clip), the last partial hop is zero padded; clips, n_fft 2048 */
       DSP_FRAMING_CENTER = 2 };     /* librosa's center = True, pad_mode = "constant" (librosa >= 0.10): frame t is samples
                                        [t hop - n_fft / 2, t hop + n_fft / 2) of the clip, zeros outside it, T = 1 + n / hop for n >= 1;
                                        clips, n_fft 400 and 2048.  librosa's older pad_mode = "reflect" is out of scope              */
enum { DSP_PREFILTER_NONE = 0, DSP_PREFILTER_BUTTER_1000_3000 = 1, DSP_PREFILTER_BUTTER_3000_7500 = 2 };

/* Compile-time constants of the reference (mfcc_params.h:6-12, mfcc.c:172-173)
 * turned into a POD; dsp_mfcc_default_config() fills in the reference values. */
typedef struct dsp_mfcc_config {
    int sample_rate;  /* 16000 */
    int n_fft;        /* 512   (supported: 400, 512, 1024, 2048; one wavefront per frame)  */
    int frame_length; /* 400   (<= n_fft) */
    int hop_length;   /* 160 */
    int n_mels;       /* 40 */
    int n_mfcc;       /* 13 */
    int window;       /* DSP_WINDOW_*  (reference: periodic Hann, export_mfcc_params.py:46) */
    int mel_norm;     /* DSP_MELNORM_* (reference: none, export_mfcc_params.py:56) */
    int log_mode;     /* DSP_LOG_*     (reference: per-frame max, mfcc.c:169-206) */
    int prefilter;    /* DSP_PREFILTER_* fp64 Butterworth per frame from zero state */
    int win_length;   /* 0 = frame_length; else window taps centred in the frame (librosa win_length < n_fft) */
    float fmin, fmax; /* 0, 8000 */
    float amin;       /* 1e-10 */
    float top_db;     /* 80 */
    int spectrum;     /* DSP_SPECTRUM_* (reference: power) */
    int framing;      /* DSP_FRAMING_*  (reference: complete frames only) */
} dsp_mfcc_config;

void dsp_mfcc_default_config(dsp_mfcc_config *cfg);
/* The parameterisation of cepstrum/scrubjay_infer.c:9-13,28-30 with aubio 0.4's semantics for the calls it makes:
 * WIN_SIZE 2048 / HOP_SIZE 1024 streaming frames (DSP_FRAMING_STREAM), "hanningz" = periodic Hann, magnitude spectrum,
 * the 40-filter Slaney bank, log10, orthonormal DCT-II, 20 coefficients.  sample_rate: the file's own (aubio_source with
 * samplerate 0).  aubio is an unvendored dependency of the reference: restated from its published algorithm, parity unpinned. */
void dsp_mfcc_scrubjay_infer_config(dsp_mfcc_config *cfg, int sample_rate);
/* The rows the speaker GMMs are trained and scored on (2fa/audio/speaker/gmm_utils.py:8-11,52-58):
 * librosa.feature.mfcc(y, sr = 16000, n_mfcc = 13, n_fft = 400, hop_length = 160) with librosa's defaults -- centred frames of 400
 * samples with zero padding (DSP_FRAMING_CENTER), periodic Hann, a 400-point transform (201 bins), 128 unit-area filters on
 * Slaney's mel scale over 0 - 8 kHz (DSP_MELNORM_LIBROSA), power_to_db(ref = 1, amin = 1e-10, top_db = 80) over the clip
 * (DSP_LOG_GLOBAL_REF1), orthonormal DCT-II.  The sliding CMVN that follows is dsp_cmvn_*.  librosa is an unvendored dependency of
 * the reference: restated from its published algorithm, parity unpinned.
 * A 400-point plan (n_fft = frame_length = 400, win_length 0, n_mels <= 128, n_mfcc <= min(n_mels, 32), mel norm NONE / SLANEY /
 * LIBROSA, log mode PER_FRAME_MAX / GLOBAL_REF1, power spectrum, framing COMPLETE / CENTER, no prefilter) runs float frames, clips
 * and ragged batches and their host forms; PCM16 input, the fused clip kernels, scanners, stream sessions, dsp_mfcc_lane_tables and
 * non-default kernels refuse it (DSP_EINVAL).                                                                                      */
void dsp_mfcc_speaker_config(dsp_mfcc_config *cfg);
/* The rows the keyword net and the scrub-jay SVM are trained on (2fa/audio/keyword_classifier.py:41-44 with sr 22050, n_mfcc 13;
 * cepstrum/train.py:38-40 and run.py:11-14 with n_mfcc 20): librosa.feature.mfcc(y, sr = sample_rate, n_mfcc = n_mfcc) with librosa's
 * defaults -- n_fft = frame_length = 2048, hop_length 512, centred frames with zero padding (DSP_FRAMING_CENTER), periodic Hann, 128
 * unit-area filters on Slaney's mel scale over 0 .. sample_rate / 2 (DSP_MELNORM_LIBROSA), power_to_db(ref = 1, amin = 1e-10,
 * top_db = 80) over the clip (DSP_LOG_GLOBAL_REF1), orthonormal DCT-II.  The pad mode is "constant" (librosa >= 0.10); "reflect" is
 * not built.  librosa is an unvendored dependency of the reference: restated from its published algorithm, parity with librosa's own
 * numbers unpinned.
 * A centred 2048-point plan (n_fft = frame_length = 2048, win_length 0, n_mels <= 128, n_mfcc <= 32, mel norm NONE / SLANEY / LIBROSA,
 * log mode PER_FRAME_MAX / GLOBAL_REF1, power spectrum, no prefilter; any even hop) runs float clips and ragged batches and their host
 * forms, and independent frames (dsp_mfcc_frames_*: whole frames, no padding); PCM16 input, the fused clip kernels, scanners and stream
 * sessions refuse it (DSP_EINVAL naming the framing).  Positions outside a clip read as zero and are never loaded.                   */
void dsp_mfcc_librosa_config(dsp_mfcc_config *cfg, int sample_rate, int n_mfcc);

typedef struct dsp_mfcc_plan dsp_mfcc_plan; /* opaque: device tables for one config on one GPU */

/* Builds the constant tables (window, FFT twiddles, sparse HTK-mel chunks,
 * DCT-II basis; formulas of 2fa/audio/word/python/export_mfcc_params.py:27-60)
 * on the host and uploads them to `device`.                                   */
int dsp_mfcc_plan_create(const dsp_mfcc_config *cfg, int device, dsp_mfcc_plan **out);
void dsp_mfcc_plan_destroy(dsp_mfcc_plan *plan);
int dsp_mfcc_plan_config(const dsp_mfcc_plan *plan, dsp_mfcc_config *cfg);

/* Number of frames compute_mfcc produces for an n-sample clip (mfcc.c:132-139); under DSP_FRAMING_STREAM / _CENTER that framing's
 * count (see the enum).  Host only.                                              */
int dsp_mfcc_frames_for(const dsp_mfcc_config *cfg, int num_samples, int max_frames);

/* --- device-resident entry points: pointers are HBM addresses on the plan's
 * device, work is enqueued on `stream` (a hipStream_t, NULL = default stream)
 * and the call returns without synchronising.                                 */

/* n_frames independent frames, d_frames[n_frames][frame_length] back to back
 * -> d_out[n_frames][n_mfcc]  (BASELINE configs 2/3).                          */
int dsp_mfcc_frames_device(dsp_mfcc_plan *plan, const float *d_frames, long n_frames,
                           float *d_out, void *stream);

/* n_clips clips of samples_per_clip floats, clip c starting at
 * d_signal + c*clip_stride; each framed like compute_mfcc (frame_length/hop)
 * and capped at max_frames -> d_out[n_clips][T][n_mfcc]; returns T.           */
int dsp_mfcc_clips_device(dsp_mfcc_plan *plan, const float *d_signal, long n_clips,
                          int samples_per_clip, long clip_stride, float *d_out,
                          int max_frames, void *stream);

/* fft_real_forward (2fa/audio/word/c/mfcc.c:16-95; non-static there, so callers may link it): 400 real samples, zero-padded to 512,
 * forward transform, all 512 complex bins interleaved [re0, im0, re1, im1, ...].  Host pointers; void like the reference (a failure:
 * zeros out, reason in dsp_last_error()).  dsp_fft_real_forward_host: the same for a batch and any power-of-two n_fft <= 4096.    */
void fft_real_forward(const float *in_time, float *out_freq);
int dsp_fft_real_forward_host(const float *in_time, long n_frames, int frame_length, long in_stride, int n_fft, float *out_freq);

/* PCM16 ingestion on the device: the same framing on interleaved int16 PCM,
 * converted in the load exactly like the reference's WAV readers: mono s/32768
 * (2fa/audio/word/c/main_test.c:198-203); stereo channel 0 (donut-classifier/classifier.c:292-297)
 * or the channel average 0.5(L/32768 + R/32768) (main_test.c:205-217).  samples_per_clip and
 * clip_stride count samples PER CHANNEL.  Halves (mono) the HBM bytes of the float path.
 * Plans: dsp_mfcc_scrubjay_infer_config (n_fft 2048), and n_fft 512 on the default kernel in the
 * per-frame log mode where the kernel's shape has an int16 form: n_mfcc <= 16 with n_mels <= 40 and
 * no mel filter wider than 36 FFT bins (dsp_mfcc_default_config's shape).  Elsewhere DSP_EINVAL.  */
enum { DSP_STEREO_CHANNEL0 = 0, DSP_STEREO_AVERAGE = 1 };
int dsp_mfcc_clips_pcm16_device(dsp_mfcc_plan *plan, const int16_t *d_pcm, long n_clips, int samples_per_clip,
                                long clip_stride, int channels, int stereo_mode, float *d_out, int max_frames,
                                void *stream);

/* RAGGED MFCC matrices: clips of different lengths in ONE launch (the reference's callers run compute_mfcc once per file:
 * 2fa/audio/word/c/main_test.c:254-331, cepstrum/scrubjay_infer.c:158-176).  offsets is a HOST array of n_clips + 1 sample positions
 * (per channel) into the device buffer, the contract of dsp_scrubjay_fused_ragged_device: clip c is [offsets[c], offsets[c + 1]),
 * non-decreasing, any parity (the buffer itself 8-byte aligned, 4 for mono int16), read before the call returns.  Clip c gets the
 * frames its own length gives; clips with ZERO frames are legal (compute_mfcc returns 0 for them, mfcc.c:117-119) and add no rows.
 * The matrices lie back to back, frame-major: clip c's frames are d_out[frame_offsets[c] .. frame_offsets[c + 1])[n_mfcc], each row
 * bit for bit what dsp_mfcc_clips_device (_pcm16_device) returns for that clip alone with the same plan and max_frames; under
 * DSP_LOG_GLOBAL_REF1 the top_db floor is taken over each clip's own frames.  Plans: n_fft 512 (wave-per-frame kernels, both log
 * modes), n_fft 2048 (dsp_mfcc_scrubjay_infer_config and the variants dsp_mfcc_clips_device accepts) and n_fft 400; PCM16 on exactly
 * the plans dsp_mfcc_clips_pcm16_device takes it on (the kernel shape included).  n_fft 1024 and prefilter plans: DSP_EINVAL.  Returns
 * the frame count of the longest clip.
 *
 * dsp_mfcc_ragged_frame_offsets (host only, no GPU): frame_offsets[n_clips + 1] = prefix sums of
 * dsp_mfcc_frames_for(cfg, offsets[c + 1] - offsets[c], max_frames); returns the total frame count (>= 0) or a negative DSP_E* code. */
long dsp_mfcc_ragged_frame_offsets(const dsp_mfcc_config *cfg, const long *offsets, long n_clips, int max_frames, long *frame_offsets);
int dsp_mfcc_clips_ragged_device(dsp_mfcc_plan *plan, const float *d_signal, long n_clips, const long *offsets,
                                 int max_frames, float *d_out, void *stream);
int dsp_mfcc_clips_ragged_pcm16_device(dsp_mfcc_plan *plan, const int16_t *d_pcm, long n_clips, const long *offsets,
                                       int channels, int stereo_mode, int max_frames, float *d_out, void *stream);

/* --- host-pointer entries: the batch STREAMS through the GPU, the call is blocking. --------
 * The arguments of the device entries with host pointers.  A batch in pinned memory larger than the host pipeline's chunk (below) is cut
 * into chunks -- whole frames, whole clips -- that travel through a ring of staging buffers: the copy in of one chunk runs under the
 * kernels and the copy out of the one before.  Device staging is then bounded by depth x chunk, never by the batch.  A batch that fits
 * one chunk is one pass.  Every row is bit for bit the device entry's, wherever the cuts fall (under DSP_LOG_GLOBAL_REF1 the floor is
 * per clip, and no clip is cut).  Memory from dsp_host_alloc (or any pinned / registered memory: hipHostMalloc, hipHostRegister, torch's
 * pin_memory()) is read and written by the copy engines directly; what is done with pageable memory is the pipeline's pageable_mode
 * (by default such a batch is not cut).  When the call returns every output byte is in `out` and nothing of the call is in flight.
 * The ragged entries: out[frame_offsets[n_clips]][n_mfcc] with the frame_offsets of dsp_mfcc_ragged_frame_offsets.                      */
int dsp_mfcc_frames_host(dsp_mfcc_plan *plan, const float *frames, long n_frames, float *out);
int dsp_mfcc_clips_host(dsp_mfcc_plan *plan, const float *signal, long n_clips,
                        int samples_per_clip, long clip_stride, float *out, int max_frames);
int dsp_mfcc_clips_pcm16_host(dsp_mfcc_plan *plan, const int16_t *pcm, long n_clips, int samples_per_clip, long clip_stride,
                              int channels, int stereo_mode, float *out, int max_frames);
int dsp_mfcc_clips_ragged_host(dsp_mfcc_plan *plan, const float *signal, long n_clips, const long *offsets, int max_frames, float *out);
int dsp_mfcc_clips_ragged_pcm16_host(dsp_mfcc_plan *plan, const int16_t *pcm, long n_clips, const long *offsets, int channels,
                                     int stereo_mode, int max_frames, float *out);

/* Pinned host memory for C callers: what the host entries (these, and dsp_classify_batch*_host*) copy from and to without a bounce.
 * dsp_host_alloc: bytes > 0 of page-locked memory, usable from every device; dsp_host_free(NULL) does nothing.                        */
int dsp_host_alloc(int device, size_t bytes, void **out);
void dsp_host_free(void *p);

/* The host pipeline of a device (one per device, shared by every host entry that runs there; calls on one device queue).
 * chunk_bytes >= 4096: the input bytes of one chunk; depth 1 .. 4: the ring's slots (1: copy, run and copy back strictly in turn);
 * pageable_mode: what a call does with a batch in PAGEABLE memory that is larger than a chunk --
 *   DSP_HOST_PAGEABLE_WHOLE     the batch is not cut: one chunk, as a batch that fits (a classifier: its sub-batches, copied _DIRECT)
 *   DSP_HOST_PAGEABLE_REGISTER  page-locks the caller's input and output arrays for the duration of the call and copies as from pinned
 *                               memory (where the runtime refuses: the input as _DIRECT, the output through the pinned ring)
 *   DSP_HOST_PAGEABLE_DIRECT    hands the input to the runtime's own pageable copy chunk by chunk
 *   DSP_HOST_PAGEABLE_STAGE     packs each chunk by memcpy into the ring's pinned buffer
 * classify_min_clips >= 1: the fewest clips of a chunk of a classifier's batch, whatever chunk_bytes says (a pass walks each clip's
 * recurrence in sequence, so a pass of few clips costs nearly what a pass of thousands does).  No setting changes a result bit.
 * dsp_host_pipeline_set(device, NULL) puts the defaults back: chunk_bytes 64 MiB, depth 2, DSP_HOST_PAGEABLE_WHOLE, 65536 clips (a classifier's chunk is then a whole
 * pass through its workspace; ragged batches: the bytes of that many seconds of audio)
 * (DESIGN.md has the measurements behind them).  A batch of ONE chunk is copied, run and copied back on the null stream straight from
 * and to the caller's arrays, as one pass.  _set, _get and _stats touch no device; dsp_host_pipeline_release returns the ring's pinned
 * and device memory and its copy stream (they come back with the next call that needs them).
 * dsp_host_pipeline_stats: what the LAST host call on that device did -- its chunks, the ring depth it used (1 for a single chunk), the
 * bytes copied each way, the path the input and the output took (DSP_HOST_PATH_*: _DIRECT is the caller's array handed to the runtime's
 * copy as it is), the most device staging the ring held during the call and the ring's pinned bytes after it.                      */
enum { DSP_HOST_PATH_STAGED = 0, DSP_HOST_PATH_PINNED = 1, DSP_HOST_PATH_REGISTERED = 2, DSP_HOST_PATH_DIRECT = 3 };
enum { DSP_HOST_PAGEABLE_STAGE = 0, DSP_HOST_PAGEABLE_REGISTER = 1, DSP_HOST_PAGEABLE_DIRECT = 2, DSP_HOST_PAGEABLE_WHOLE = 3 };
typedef struct {
    long chunk_bytes;
    int depth;
    int pageable_mode;
    int classify_min_clips;
} dsp_host_pipeline_config;
typedef struct {
    long n_chunks;
    int depth;
    int input_path, output_path;
    long bytes_h2d, bytes_d2h;
    long peak_staging_bytes;
    long pinned_ring_bytes;
} dsp_host_stats;
int dsp_host_pipeline_set(int device, const dsp_host_pipeline_config *cfg);
int dsp_host_pipeline_get(int device, dsp_host_pipeline_config *cfg);
int dsp_host_pipeline_release(int device);
int dsp_host_pipeline_stats(int device, dsp_host_stats *out);
/* The pipeline's chunk planner, host only (no device is touched).  offsets == NULL: n_items uniform items of item_bytes each, floor(
 * chunk_bytes / item_bytes) per chunk, at least 1.  offsets given (n_items + 1, non-decreasing): a ragged batch of samples of
 * item_bytes bytes each, cut at clip boundaries only and filled greedily up to chunk_bytes; a clip longer than chunk_bytes is the only
 * clip with samples of its chunk; empty clips never open a chunk of their own.  Chunk k is items [first[k], first[k + 1]); the chunks
 * tile the batch in order.  Returns the number of chunks (0 for an empty batch); first (may be NULL: count only) gets the returned
 * count + 1 entries and must have room for max_first, else DSP_EINVAL.                                                              */
long dsp_host_plan_chunks(long n_items, long item_bytes, const long *offsets, long chunk_bytes, long *first, long max_first);

/* Launch geometry knobs for tuning / profiling (0 = library default). */
int dsp_mfcc_plan_set_launch(dsp_mfcc_plan *plan, int blocks_per_cu, int frames_per_chunk);
/* Kernel form: DSP_KERNEL_WAVE = one wavefront per frame, log + DCT once per 16-frame tile
 * (default); DSP_KERNEL_WAVE_FRAME = one wavefront per frame with the per-frame log + DCT epilogue (what
 * DSP_LOG_GLOBAL_REF1 plans always run); DSP_KERNEL_ROW = on a 1024-point plan, the general Stockham kernel
 * instead of the register-resident wave kernel.  Same results to rounding; DESIGN.md has the numbers.
 * The 512-point forms that DSP_KERNEL_ROW (one 16-lane row per frame) and DSP_KERNEL_PAIR (two frames per
 * wavefront step) named were measured slower than the default and removed: the ids keep their values,
 * DSP_KERNEL_PAIR on any plan and DSP_KERNEL_ROW on a plan whose n_fft is not 1024 return DSP_EINVAL. */
enum { DSP_KERNEL_WAVE = 0, DSP_KERNEL_ROW = 1, DSP_KERNEL_WAVE_FRAME = 2, DSP_KERNEL_PAIR = 3 };
int dsp_mfcc_plan_set_kernel(dsp_mfcc_plan *plan, int kernel);

/* --- Butterworth band-pass (donut-classifier/classifier.c:319-446) ---------- */

/* Literal 9-tap tables of classifier.c:342-360 / 383-401; returns 1, or 0 for
 * any other band (the reference prints "invalid bandpass range").              */
int dsp_butter_bandpass(double lowcut, double highcut, double *b, double *a);

/* butter_bandpass_filter (sync/lib/classifier.cpp:193-219 fp32, donut-classifier/
 * classifier.c:420-446 fp64): direct form II from zero state over n_clips rows of n
 * samples (row stride in elements), bit-identical to the reference's operation order.
 * Host pointers; b and a hold 9 taps each.                                        */
int dsp_butter_bandpass_filter_f32(const float *data, long n_clips, int n, long stride,
                                   const float *b, const float *a, float *output);
int dsp_butter_bandpass_filter_f64(const double *data, long n_clips, int n, long stride,
                                   const double *b, const double *a, double *output);

/* compute_spectrogram (sync/lib/classifier.cpp:221-368): nperseg 256, hop 224, detrend,
 * periodic Tukey(0.25), PSD.  Flat outputs instead of the reference's malloc'd rows:
 * frequencies[129], times[T], sxx[129][T]; returns T = (n-256)/224+1 (0 if n < 256).
 * Host pointers; frequencies / times may be NULL.                                 */
int dsp_compute_spectrogram_f32(const float *signal, int signal_length, int fs,
                                float *frequencies, float *times, float *sxx);
/* The float64 twin, compute_spectrogram of donut-classifier/classifier.c:448-592 (FFTW r2c there; here a float64 DFT per
 * frame, the same transform -- parity by tolerance, FFTW is unvendored).  Same flat layout in double.                  */
int dsp_compute_spectrogram_f64(const double *signal, int signal_length, int fs,
                                double *frequencies, double *times, double *sxx);

/* Per-clip trace of classify() for parity tests: midpoints (classifier.cpp:433-598) and
 * the three band sums per midpoint (classifier.cpp:99-101).                       */
typedef struct dsp_classify_trace {
    int n_midpoints;
    float midpoints[64];
    float sums[64][3];   /* above (5-7 kHz), middle (2.5-5 kHz), below (0.5-2.5 kHz); rows after the
                          * first midpoint that fires the rule are 0 (the reference stops there)  */
} dsp_classify_trace;

/* classify() over n_clips clips of n samples (row stride in floats).  labels[n_clips];
 * trace may be NULL.  _host: host pointers, blocking.  _device: HBM pointers, STREAM-ORDERED: the call returns once
 * its work is enqueued on `stream`; the labels are valid when the stream reaches that point.  The library keeps one
 * grow-only workspace per device (42 KB per one-second clip of the largest pass; dsp_classify_release frees it): calls
 * on one device are ordered one behind the other whatever their streams, calls on different devices share nothing.  */
int dsp_classify_batch_host(const float *signal, long n_clips, int n, long stride, int *labels,
                            dsp_classify_trace *trace);
int dsp_classify_batch_device(const float *d_signal, long n_clips, int n, long stride, int *d_labels,
                              void *stream);

/* The thresholds the reference's variants of classify() hard-code, as a POD (everything else in
 * those files is identical, `diff sync/lib/classifier.cpp microphone/src/classifier.cpp`):
 *                                   keep band      midpoint dB   rule  middle <  above >  below >
 *   sync/lib/classifier.cpp         0.65 / 0.80    70            100 / 200 / 80    (:67-68, :436, :109)  default
 *   microphone/src/classifier.cpp   0.70 / 0.85    45            100 / 200 / 150   (:79-80, :448, :123)
 *   microphone/src/classifier.c     0.70 / 0.85    45            50 / 200 / 200    (:120-121, :608, :164)   float64 file
 *   donut-classifier/classifier.c   0.70 / 0.85    45            75 / 300 / 100    (:141-142, :660, :184)   float64 file
 * (the two float64 files: their THRESHOLDS on this library's fp32 arithmetic, which is sync/lib's)
 * The _cfg entry points take a NULL cfg for the default set.                          */
typedef struct dsp_classify_config {
    float keep_lo, keep_hi;        /* normalised-dB band kept in the 3000-7500 Hz map            */
    float midpoint_db;             /* lower_threshold_dB of find_midpoints                        */
    float middle_max, above_min, below_min;   /* sum_middle < . && sum_above > . && sum_below > . */
} dsp_classify_config;
void dsp_classify_default_config(dsp_classify_config *cfg);
int dsp_classify_batch_host_cfg(const dsp_classify_config *cfg, const float *signal, long n_clips, int n, long stride,
                                int *labels, dsp_classify_trace *trace);
int dsp_classify_batch_device_cfg(const dsp_classify_config *cfg, const float *d_signal, long n_clips, int n, long stride,
                                  int *d_labels, void *stream);
/* The same on int16 PCM, mono or interleaved stereo (DSP_STEREO_CHANNEL0 / DSP_STEREO_AVERAGE as dsp_mfcc_clips_pcm16_device),
 * converted in the kernels' loads exactly like the reference's capture loop and readers (sync/sync.cpp:237-242 pcmSample / 32768.0,
 * donut-classifier/classifier.c:55-59, :286-297; the average as main_test.c:205-217): bit-identical to the float entry points on the
 * same samples at half the input bytes.  n and stride count samples PER CHANNEL.                                              */
int dsp_classify_batch_pcm16_host(const dsp_classify_config *cfg, const int16_t *pcm, long n_clips, int n, long stride, int channels,
                                  int stereo_mode, int *labels, dsp_classify_trace *trace);
int dsp_classify_batch_pcm16_device(const dsp_classify_config *cfg, const int16_t *d_pcm, long n_clips, int n, long stride, int channels,
                                    int stereo_mode, int *d_labels, void *stream);
/* RAGGED batches: clips of different lengths in one call (donut-classifier/classifier.c:286-297 reads a file of any length; its callers
 * loop over files).  offsets is a HOST array of n_clips + 1 sample positions (per channel) into the buffer: clip c is
 * [offsets[c], offsets[c + 1]), non-decreasing, any parity; a clip shorter than 256 samples holds no spectrogram segment and gets label
 * 0, one of more than 13.4 s is refused like in the uniform entry points.  Every clip gets the label (and trace record) of a one-clip
 * call on it, bit for bit.  The array is read before the call returns.  _device: the whole buffer in HBM, stream-ordered; _host: the
 * buffer signal[offsets[n_clips]] is copied to the GPU once, trace may be NULL.                                                       */
int dsp_classify_batch_ragged_device(const dsp_classify_config *cfg, const float *d_signal, long n_clips, const long *offsets,
                                     int *d_labels, void *stream);
int dsp_classify_batch_ragged_pcm16_device(const dsp_classify_config *cfg, const int16_t *d_pcm, long n_clips, const long *offsets,
                                           int channels, int stereo_mode, int *d_labels, void *stream);
int dsp_classify_batch_ragged_host(const dsp_classify_config *cfg, const float *signal, long n_clips, const long *offsets, int *labels,
                                   dsp_classify_trace *trace);
int dsp_classify_batch_ragged_pcm16_host(const dsp_classify_config *cfg, const int16_t *pcm, long n_clips, const long *offsets,
                                         int channels, int stereo_mode, int *labels, dsp_classify_trace *trace);
/* What the LAST pass (sub-batch) of the shared context on `device` did (blocks until it has finished): segments of the 1000-3000 Hz
 * output the energy gate left to the flag transform, clips that had midpoints.  Either pointer may be NULL.                           */
int dsp_classify_stats(int device, long *gated_segments, long *listed_clips);
/* A classifier context of the caller's own (tables + workspace on `device`).  The entry points above share one context per device, so
 * two calls on one device run one behind the other; calls through different contexts, on different streams, may overlap.            */
typedef struct dsp_classify_ctx dsp_classify_ctx;
int dsp_classify_ctx_create(int device, dsp_classify_ctx **out);
void dsp_classify_ctx_destroy(dsp_classify_ctx *ctx);
int dsp_classify_batch_device_ctx(dsp_classify_ctx *ctx, const dsp_classify_config *cfg, const float *d_signal, long n_clips, int n,
                                  long stride, int *d_labels, void *stream);
/* test hook, no GPU call: holds the default context of `device` for hold_ms milliseconds (two devices overlap, one device queues) */
int dsp_debug_hold_classify_ctx(int device, int hold_ms);
/* frees the float32 classifier's tables and workspace on `device` (-1: every device) after its pending work has finished */
int dsp_classify_release(int device);

/* The float64 classifier, donut-classifier/classifier.c (the file's per-clip body :83-192, sum_intense :594-653,
 * find_midpoints :655-830): both Butterworth filters, both spectrograms, dB maps, 45 dB midpoints, normalisation, keep band,
 * band sums and rule in double on the GPU.  Thresholds are doubles as in the file; cfg NULL = its own
 * (0.70 / 0.85 :141-142, 45 dB :660, middle < 75 && above > 300 && below > 100 :184).  fs is 16000 (the rate butter_bandpass has
 * coefficients for).  The reference transforms with FFTW (unvendored): the spectrogram is a float64 transform of its own (a
 * 128-point complex FFT per half-wavefront; DSP_AMD_F64_DFT=1: the direct DFT of dsp_compute_spectrogram_f64), so parity is by
 * tolerance (labels and midpoints equal, band sums to ~1e-9 relative).  Neither filtered signal is written to HBM: one pass keeps the
 * filters' restart states (36 KB per one-second clip) and settles the loud time bins with a bounded screening transform; only
 * undecided segments and the clips with midpoints are recomputed and transformed in float64.  The library keeps one grow-only workspace
 * PER DEVICE (112 KB per one-second clip of the largest pass, passes of at most 49 152 clips on 256 CUs; DSP_AMD_F64_SUB_BATCH lowers
 * that; dsp_classify_release_f64 frees it).
 * _host: host pointers, blocking.  _device: HBM pointers (d_trace may be NULL), STREAM-ORDERED: the call returns once its work is
 * enqueued on `stream`; results are valid when the stream reaches that point.  Calls on one device share its workspace and are
 * ordered one behind the other (whatever their streams); calls on different devices share nothing.
 * _pcm16_: int16 PCM, mono or interleaved stereo (channel 0, or the average of the two channels), converted in the kernels' loads
 * exactly like the reference's readers: s / 32768.0 (classifier.c:55-59, channel 0 of a stereo file :286-297; sync/sync.cpp:237-242;
 * the average as main_test.c:205-217) -- bit-identical to the float64 entry points on the same samples, at a quarter of the input bytes.
 * n and stride count samples PER CHANNEL.                                                                                  */
typedef struct dsp_classify_config_f64 {
    double keep_lo, keep_hi, midpoint_db, middle_max, above_min, below_min;
} dsp_classify_config_f64;
typedef struct dsp_classify_trace_f64 {
    int n_midpoints;
    double midpoints[64];
    double sums[64][3];
} dsp_classify_trace_f64;
void dsp_classify_default_config_f64(dsp_classify_config_f64 *cfg);
int dsp_classify_batch_host_f64(const dsp_classify_config_f64 *cfg, const double *signal, long n_clips, int n, long stride,
                                int *labels, dsp_classify_trace_f64 *trace);
int dsp_classify_batch_device_f64(const dsp_classify_config_f64 *cfg, const double *d_signal, long n_clips, int n, long stride,
                                  int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream);
int dsp_classify_batch_pcm16_host_f64(const dsp_classify_config_f64 *cfg, const int16_t *pcm, long n_clips, int n, long stride, int channels,
                                      int stereo_mode, int *labels, dsp_classify_trace_f64 *trace);
int dsp_classify_batch_pcm16_device_f64(const dsp_classify_config_f64 *cfg, const int16_t *d_pcm, long n_clips, int n, long stride, int channels,
                                        int stereo_mode, int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream);
/* RAGGED batches (offsets as dsp_classify_batch_ragged_device: a HOST array of n_clips + 1 sample positions per channel): the float64
 * classify() of donut-classifier/classifier.c on clips of different lengths in one call -- the files its reader (:286-297) takes one per
 * run.  Labels and trace records of a one-clip call on every clip, bit for bit.  d_trace / trace may be NULL.                          */
int dsp_classify_batch_ragged_device_f64(const dsp_classify_config_f64 *cfg, const double *d_signal, long n_clips, const long *offsets,
                                         int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream);
int dsp_classify_batch_ragged_pcm16_device_f64(const dsp_classify_config_f64 *cfg, const int16_t *d_pcm, long n_clips, const long *offsets,
                                               int channels, int stereo_mode, int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream);
int dsp_classify_batch_ragged_host_f64(const dsp_classify_config_f64 *cfg, const double *signal, long n_clips, const long *offsets, int *labels,
                                       dsp_classify_trace_f64 *trace);
int dsp_classify_batch_ragged_pcm16_host_f64(const dsp_classify_config_f64 *cfg, const int16_t *pcm, long n_clips, const long *offsets,
                                             int channels, int stereo_mode, int *labels, dsp_classify_trace_f64 *trace);
/* What the LAST pass of the float64 classifier on `device` did (blocks until it has finished): spectrogram segments of the
 * 1000-3000 Hz output, how many of them the screening left to the float64 transform, clips that had midpoints.  Any pointer may be NULL. */
int dsp_classify_stats_f64(int device, long *segments, long *undecided, long *listed_clips);
/* Diagnostic builds of the library only (-DSC_DIAG): the screening kernel's per-block records of the last pass (16 ints per block).  */
int dsp_classify_debug_f64(int device, int *out, int n_ints);
/* frees the float64 classifier's workspace on `device` (-1: on every device) after its pending work has finished */
int dsp_classify_release_f64(int device);

/* sum_intense (sync/lib/classifier.h:17, classifier.cpp:370-431) on a flat matrix: db[freq_bins][time_bins] (NaN = dropped
 * cell), the reference's index searches and its (row, column) summation order.  Host pointers; *out receives the sum.   */
int dsp_sum_intense_f32(float lower, float upper, float half_range, const float *frequencies, int freq_bins,
                        const float *times, int time_bins, const float *db, float midpoint, float *out);

/* find_midpoints (sync/lib/classifier.h:18, classifier.cpp:433-598): the 1000-3000 Hz filter, its spectrogram,
 * time bins above 70 dB, greedy clusters of at least 0.15 s -> their mean times, in seconds.  Host pointers.
 * Returns the number of midpoints (the first max_midpoints are written) or a negative error; fs must be 16000
 * (the only rate butter_bandpass has coefficients for).  Clips are limited to 957 spectrogram columns (13.4 s):
 * a cluster needs 12 columns and a 4-column gap, so no such clip has more than the 64 midpoints a trace record
 * holds; longer clips are rejected (DSP_EINVAL) rather than truncated.                 */
int dsp_find_midpoints(const float *data, int num_frames, int fs, float *midpoints, int max_midpoints);

/* --- several GPUs from one C process ---------------------------------------
 * Clips shard without any exchange: give device d the clips [d * ceil(N / D), ...) through the entry points above (plans, models and
 * classifier contexts are per device; calls on different devices share no lock).  The path's one exchange step is the gather of the
 * per-clip results: one RCCL communicator per listed device (ncclCommInitAll) and ONE grouped all-gather per call over xGMI -- rank r
 * (= devices[r]) contributes bytes_per_rank bytes at d_send[r] and receives every rank's block, in rank order, at d_recv[r]
 * (n_devices * bytes_per_rank bytes; pad the last shard so the counts are equal).  Stream-ordered on streams[r] (NULL: the device's
 * null stream), so the gather of batch k can cross xGMI while batch k + 1 is computed on another stream.  RCCL is loaded at the first
 * dsp_gather_create (dlopen of librccl.so.1): hosts that never gather do not need it.  INTEGRATION.md, "8 GPUs from C".       */
typedef struct dsp_gather dsp_gather;
int dsp_gather_create(const int *devices, int n_devices, dsp_gather **out);
void dsp_gather_destroy(dsp_gather *g);
int dsp_gather_n_devices(const dsp_gather *g);
int dsp_gather_all(dsp_gather *g, const void *const *d_send, void *const *d_recv, size_t bytes_per_rank, void *const *streams);

/* --- pooling + SVM (cepstrum/scrubjay_infer.c:36-66, 105-141; scrubjay_svm.onnx) ------ */

/* mfcc_stats pooling: feat[c][2*n_coef] = per-coefficient mean | population std over the T
 * frames of clip c, float64 accumulators in frame order.  HBM pointers.            */
int dsp_mfcc_stats_device(const float *d_mfcc, long n_clips, int n_frames, int n_coef, float *d_feat, void *stream);

typedef struct dsp_svm dsp_svm;   /* opaque: Scaler + RBF SVMClassifier + Platt on one GPU */
/* Attributes as stored in the ONNX graph (Scaler.offset/scale, SVMClassifier.support_vectors
 * [n_sv][n_features], coefficients[n_sv], kernel_params[0] = gamma, rho[0], prob_a[0], prob_b[0]). */
int dsp_svm_create(int device, int n_features, int n_sv, const float *offset, const float *scale,
                   const float *support_vectors, const float *coefficients, float gamma, float rho,
                   float prob_a, float prob_b, dsp_svm **out);
void dsp_svm_destroy(dsp_svm *svm);
/* labels, decision values and P(label 1) for n_clips feature rows; HBM pointers, d_decision / d_prob1 may be NULL.
 * libsvm's rules (sklearn's SVC is libsvm; pinned by tests/golden/svm_libsvm_ref.npz): decision = sum_i coef_i K(x, sv_i) +
 * rho; label = the pairwise vote, decision > 0 -> class 0 else class 1 (what .predict returns in cepstrum/run.py, and ONNX
 * Runtime's output_label in SVC mode); P(label 1) from svm_predict_probability (Platt pair -> multiclass_probability's
 * iteration, which is NOT the plain sigmoid: exactly 0.5 in a dead zone around decision = 0).                      */
int dsp_svm_predict_device(dsp_svm *svm, const float *d_feat, long n_clips, int *d_labels, float *d_decision,
                           float *d_prob1, void *stream);

/* BASELINE config 5 in ONE kernel: clip -> MFCC(n_mfcc) -> mean | std -> Scaler -> RBF-SVM -> label, the MFCC
 * matrix never leaves the chip (one wavefront walks one clip; pooling in the kernel's tile epilogue).  The plan's
 * 2 * n_mfcc must equal the SVM's n_features (<= 64) and, at n_fft = 512, the SVM may have at most 2048 support vectors (its
 * coefficients ride in the kernel's LDS; a larger model is refused with DSP_EINVAL on this entry, its int16 and its ragged forms, and
 * takes the three calls or the 2048-point plans); equal results to dsp_mfcc_clips_device +
 * dsp_mfcc_stats_device + dsp_svm_predict_device.  Plans with n_fft = 512 (BASELINE config 5) or n_fft = 2048 (the framing
 * of scrubjay_infer.c:10-14 itself: 2048 / 1024 / 40 filters / 20 coefficients).  d_decision, d_prob1, d_feat ([n_clips][2 n_mfcc]) may be NULL. */
int dsp_scrubjay_fused_device(dsp_mfcc_plan *plan, dsp_svm *svm, const float *d_signal, long n_clips,
                              int samples_per_clip, long clip_stride, int max_frames, int *d_labels,
                              float *d_decision, float *d_prob1, float *d_feat, void *stream);
/* The same from int16 PCM (mono / interleaved stereo, as dsp_mfcc_clips_pcm16_device), converted in the kernel's load: bit-identical
 * to the float entry point on the same samples.  Plans of the reference framing (n_fft 512, frame 400, 40 mel filters) and of
 * dsp_mfcc_scrubjay_infer_config (the 2048-point front end cepstrum/scrubjay_infer.c itself runs).                                 */
int dsp_scrubjay_fused_pcm16_device(dsp_mfcc_plan *plan, dsp_svm *svm, const int16_t *d_pcm, long n_clips, int samples_per_clip,
                                    long clip_stride, int channels, int stereo_mode, int max_frames, int *d_labels,
                                    float *d_decision, float *d_prob1, float *d_feat, void *stream);
/* RAGGED batches -- clips of different lengths in ONE launch (the reference's callers loop over files: cepstrum/scrubjay_infer.c:158-176,
 * 2fa/audio/word/c/main_test.c:254-331).  offsets is a HOST array of n_clips + 1 sample positions (per channel) into the device buffer:
 * clip c is [offsets[c], offsets[c + 1]), non-decreasing, any parity (the buffer itself 8-byte aligned, 4 for mono int16); every clip
 * must hold at least one frame (DSP_EINVAL names the first that does not).  Clip c gets the frames ITS length gives
 * (dsp_mfcc_frames_for(cfg, offsets[c + 1] - offsets[c], max_frames)) and the results of a one-clip call on it, bit for bit.  The array
 * is read before the call returns.  Returns the frame count of the longest clip.                                                        */
int dsp_scrubjay_fused_ragged_device(dsp_mfcc_plan *plan, dsp_svm *svm, const float *d_signal, long n_clips, const long *offsets,
                                     int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream);
int dsp_scrubjay_fused_ragged_pcm16_device(dsp_mfcc_plan *plan, dsp_svm *svm, const int16_t *d_pcm, long n_clips, const long *offsets,
                                           int channels, int stereo_mode, int max_frames, int *d_labels, float *d_decision,
                                           float *d_prob1, float *d_feat, void *stream);

/* Test hook, host only (no GPU call): the order a ragged batch of the fused clip kernels runs in.  out4[4 * pos .. + 3] = start, samples,
 * frames, caller's index of the clip at position pos; wavefront w of n_waves walks positions w, w + n_waves, ...  Returns the longest
 * clip's frame count.                                                                                                                 */
int dsp_debug_fused_spans(const dsp_mfcc_config *cfg, const long *offsets, long n_clips, int max_frames, long n_waves, long *out4);

/* --- consumers of the MFCC matrix and the resampler (8f-4) ------- */

/* The stop-word net behind classify_signal (2fa/audio/word/c/stop_detector.h:10,
 * stop_detector.c:12-55; audio_classifier_inference.c:38-90).  The trained parameters are the
 * arrays of the reference's model_params.h, handed over by the caller (never compiled in here). */
typedef struct dsp_stop_model dsp_stop_model;
typedef struct dsp_stop_model_params {
    int n_coef;                  /* 13   MFCC_N_MFCC                              */
    int max_frames;              /* 500  MAX_FRAMES (stop_detector.c:9)           */
    int units[4];                /* 4, 2, 2, 1  DENSE1..4_UNITS (model_params.h:7-10), each <= 16, last = 1 */
    const float *scaler_mean;    /* SCALER_MEAN  [n_coef * max_frames], coefficient-major */
    const float *scaler_scale;   /* SCALER_SCALE [n_coef * max_frames]            */
    const float *kernel[4];      /* DENSEn_KERNEL, (in, out) row-major             */
    const float *bias[4];        /* DENSEn_BIAS                                    */
} dsp_stop_model_params;
int dsp_stop_model_create(const dsp_stop_model_params *params, int device, dsp_stop_model **out);
void dsp_stop_model_destroy(dsp_stop_model *model);
/* audio_classifier_predict over a batch: d_mfcc[n_clips][frames_per_clip][n_coef] frame-major (what
 * compute_mfcc writes), viewed coefficient-major and zero-padded / truncated at max_frames as
 * stop_detector.c:36-50 does; d_prob[n_clips] = P("stop").  HBM pointers.                       */
int dsp_stop_predict_device(dsp_stop_model *model, const float *d_mfcc, long n_clips, int frames_per_clip,
                            float *d_prob, void *stream);
/* classify_signal over a batch of equally long clips resident in HBM: plan (reference defaults,
 * n_mfcc = n_coef) -> MFCC matrices in a workspace -> the net.                                  */
int dsp_classify_signal_batch_device(dsp_mfcc_plan *plan, dsp_stop_model *model, const float *d_signal, long n_clips,
                                     int samples_per_clip, long clip_stride, float *d_prob, void *stream);
/* ... and from the int16 PCM main_test.c:198-217 decodes in front of classify_signal (mono s / 32768, stereo average or channel 0). */
int dsp_classify_signal_batch_pcm16_device(dsp_mfcc_plan *plan, dsp_stop_model *model, const int16_t *d_pcm, long n_clips,
                                           int samples_per_clip, long clip_stride, int channels, int stereo_mode, float *d_prob,
                                           void *stream);
/* Ragged batches (offsets as dsp_scrubjay_fused_ragged_device): one launch of the fused clip -> probability kernel, every clip with its
 * own frame count (capped at the model's max_frames, stop_detector.c:26-30).  Plans of the reference's shape only (the fused kernel's).   */
int dsp_classify_signal_batch_ragged_device(dsp_mfcc_plan *plan, dsp_stop_model *model, const float *d_signal, long n_clips,
                                            const long *offsets, float *d_prob, void *stream);
int dsp_classify_signal_batch_ragged_pcm16_device(dsp_mfcc_plan *plan, dsp_stop_model *model, const int16_t *d_pcm, long n_clips,
                                                  const long *offsets, int channels, int stereo_mode, float *d_prob, void *stream);
/* classify_signal's own contract (stop_detector.h:10) with host buffers: probability in [0, 1];
 * a failure returns 0 with the reason in dsp_last_error().                                       */
float dsp_classify_signal(dsp_stop_model *model, const float *signal, int num_samples);

/* Speaker verification: max-component log-likelihood ratio of a target GMM against a UBM in the
 * reference's fixed point (2fa/audio/pico-audio/src/speaker_gmm.h:11-38, speaker_gmm.c:29-141;
 * parameters gmm_params.inc: means Q6 int8, inverse covariances Q11 int32, log constants Q8 int16). */
typedef struct dsp_gmm_params {
    int k, d;                    /* 32 mixtures, 13 dimensions (k <= 64, d <= 16) */
    const int8_t *means;         /* [k][d] */
    const int32_t *inv_covs;     /* [k][d] */
    const int16_t *log_consts;   /* [k]    */
} dsp_gmm_params;
typedef struct dsp_speaker_model dsp_speaker_model;
int dsp_speaker_model_create(const dsp_gmm_params *target, const dsp_gmm_params *ubm, int device, dsp_speaker_model **out);
void dsp_speaker_model_destroy(dsp_speaker_model *model);
/* mfcc_target_speaker_llr_mean (:127-136) and classify_speaker (:138-141) per clip of
 * d_mfcc[n_clips][frames_per_clip][d]: d_llr_mean[n_clips] (Q8, integer mean over the frames),
 * d_labels[n_clips] = llr_mean > (int64)(-0.7 * 256); optional per-frame log-likelihoods
 * d_ll_target / d_ll_ubm [n_clips][frames_per_clip] (target_gmm_log_likelihood / ubm_..., :84-102).
 * Bit-exact integer results.  HBM pointers; d_labels, d_ll_* may be NULL.                        */
int dsp_speaker_llr_device(dsp_speaker_model *model, const float *d_mfcc, long n_clips, int frames_per_clip,
                           int64_t *d_llr_mean, int *d_labels, int64_t *d_ll_target, int64_t *d_ll_ubm, void *stream);
/* The same per clip of a ragged MFCC matrix (dsp_mfcc_clips_ragged_device): clip c is rows [frame_offsets[c], frame_offsets[c + 1])
 * of d_mfcc[..][d], frame_offsets a HOST array of n_clips + 1 rows as dsp_mfcc_ragged_frame_offsets returns it, read before the call
 * returns.  Every clip must hold at least one frame (the reference would divide by zero, speaker_gmm.c:135): DSP_EINVAL names the
 * first that does not.  d_ll_target / d_ll_ubm, if given, are [frame_offsets[n_clips]], by row.                                  */
int dsp_speaker_llr_ragged_device(dsp_speaker_model *model, const float *d_mfcc, long n_clips, const long *frame_offsets,
                                  int64_t *d_llr_mean, int *d_labels, int64_t *d_ll_target, int64_t *d_ll_ubm, void *stream);

/* SCANNING LONG RECORDINGS: P("stop") and the speaker LLR per sliding window (the firmware scores one 1 s buffer at a time,
 * sync/sync.cpp:188-213).  Windows are runs of MFCC rows: recording r is rows [frame_offsets[r], frame_offsets[r + 1]) of a ragged
 * MFCC matrix (dsp_mfcc_clips_ragged_device, no frame cap), R rows.  R >= window_frames: W = 1 + (R - window_frames) / hop_frames
 * windows, window w = rows [w hop_frames, w hop_frames + window_frames); R < window_frames (R = 0 included): one window of all R rows.
 * In samples, window w is the clip [w hop_frames hop_length, + frame_length + (window_frames - 1) hop_length), clipped to the
 * recording when W = 1: each result is the per-clip entry's on that clip -- classify_signal (rows past max_frames dropped, missing
 * rows zero-padded), mfcc_target_speaker_llr_mean / classify_speaker (Q8 int64 mean, C truncating division by the window's rows).
 * The windows of all recordings lie back to back: window_offsets[n_recordings + 1] = prefix sums of W.
 *
 * dsp_scan_window_offsets (host only, no GPU): fills window_offsets, returns the total window count or a negative DSP_E* code
 * (window_frames, hop_frames >= 1; frame_offsets non-negative, non-decreasing); n_recordings = 0 returns 0.                          */
typedef struct dsp_scan_config {
    int window_frames;           /* rows per window (98: one second of the reference's framing) */
    int hop_frames;              /* rows between window starts (10: 100 ms)                    */
} dsp_scan_config;
long dsp_scan_window_offsets(const dsp_scan_config *cfg, const long *frame_offsets, long n_recordings, long *window_offsets);
/* The stop-word net on every window: d_mfcc[..][n_coef] the ragged matrix, frame_offsets a HOST array of n_recordings + 1 rows (read
 * before the call returns), d_prob[total windows].  Each MFCC row is read once per tile of consecutive windows.  Uses a ring of
 * upload buffers in the model, no workspace: any stream.                                                                           */
int dsp_stop_scan_device(dsp_stop_model *model, const float *d_mfcc, long n_recordings, const long *frame_offsets,
                         const dsp_scan_config *cfg, float *d_prob, void *stream);
/* The speaker LLR on every window, bit-exact: d_llr_mean[total windows] (Q8), d_labels (may be NULL) = llr_mean > (int64)(-0.7 * 256).
 * Every recording must hold at least one row: DSP_EINVAL names the first that does not.  The per-row LLR is scanned into a grow-only
 * workspace of the model (8 bytes per row): calls on one speaker model serve ONE stream at a time.                                 */
int dsp_speaker_scan_device(dsp_speaker_model *model, const float *d_mfcc, long n_recordings, const long *frame_offsets,
                            const dsp_scan_config *cfg, int64_t *d_llr_mean, int *d_labels, void *stream);
/* A scanner runs the whole chain: recordings back to back in HBM (offsets as dsp_mfcc_clips_ragged_device: a HOST array of
 * n_recordings + 1 sample positions per channel; a recording longer than INT_MAX samples is DSP_EINVAL) -> ragged MFCC matrix in the
 * scanner's grow-only workspace (DSP_ENOMEM if it cannot grow) -> the scans of the models it was given, all enqueued on `stream`
 * without a host synchronisation.  The plan must be n_fft 512, DSP_LOG_PER_FRAME_MAX, DSP_FRAMING_COMPLETE, no prefilter, with n_mfcc
 * equal to the models' n_coef / d (elsewhere rows depend on the window: DSP_EINVAL); stop and speaker may each be NULL, not both.
 * The outputs of a model not given may be NULL.  The scanner borrows plan and models (destroy it first) and owns its workspace: ONE
 * stream at a time per scanner (and per speaker model), as for the stop model's own workspace.  Zero recordings: DSP_OK, no launch.  */
typedef struct dsp_scanner dsp_scanner;
int dsp_scanner_create(dsp_mfcc_plan *plan, dsp_stop_model *stop, dsp_speaker_model *speaker, const dsp_scan_config *cfg,
                       dsp_scanner **out);
void dsp_scanner_destroy(dsp_scanner *scanner);
int dsp_scanner_run_device(dsp_scanner *scanner, const float *d_signal, long n_recordings, const long *offsets, float *d_prob,
                           int64_t *d_llr_mean, int *d_labels, void *stream);
int dsp_scanner_run_pcm16_device(dsp_scanner *scanner, const int16_t *d_pcm, long n_recordings, const long *offsets, int channels,
                                 int stereo_mode, float *d_prob, int64_t *d_llr_mean, int *d_labels, void *stream);
/* SCRUB-JAY SCANS: the SVM's label, decision value, P(label 1) and the 2 n_mfcc pooled features (mean | std) per sliding window of
 * MFCC rows, the windows as above.  Each window's results equal, bit for bit, dsp_scrubjay_fused_ragged_device (same plan, same SVM)
 * on the window cut out as its own clip, on the plans whose rows do not depend on the window: the fused kernel's front ends on
 * DSP_KERNEL_WAVE, log mode DSP_LOG_PER_FRAME_MAX or DSP_LOG_LOG10_FLOOR, no prefilter, n_fft 512 or 2048 (DSP_LOG_GLOBAL_REF1: its
 * top_db floor spans the window; prefilter and n_fft 1024 plans: the ragged matrix refuses them -- DSP_EINVAL).
 * In samples, window w of recording r starts at offsets[r] + w hop_frames hop_length; it is frame_length + (window_frames - 1)
 * hop_length samples long under DSP_FRAMING_COMPLETE, window_frames hop_length under DSP_FRAMING_STREAM, clipped to the recording.
 * Under DSP_FRAMING_STREAM the first H = ceil((frame_length - hop_length) / hop_length) rows of a cut-out window see zeros before it: the
 * scanner computes each window's own min(H, rows) head rows (from a span of that many hops at its start) and takes the rest from the
 * recording's matrix.  Every recording must hold at least one row (mfcc_stats pools a window's rows): DSP_EINVAL names the first that
 * does not.  d_labels is required; d_decision, d_prob1 and d_feat[total windows][n_features] may be NULL.  Zero recordings: DSP_OK.
 *
 * dsp_scan_window_spans (host only, no GPU): starts / lengths[total windows] = each window's clip in samples (absolute positions in the
 * buffer; either may be NULL), for any valid MFCC config -- the 2fa scanner's windows included; returns the total window count or a
 * negative DSP_E* code (offsets as dsp_mfcc_clips_ragged_device).                                                                   */
long dsp_scan_window_spans(const dsp_mfcc_config *mfcc, const dsp_scan_config *cfg, const long *offsets, long n_recordings,
                           long *starts, long *lengths);
/* Matrix level, like dsp_stop_scan_device: windows = runs of rows of a ragged matrix d_mfcc[..][n_features / 2], frame_offsets a HOST
 * array (read before the call returns).  No head rows: under DSP_FRAMING_STREAM use the scanner for per-clip equality.  Uses a ring of
 * upload buffers in the SVM, no workspace: any stream.                                                                               */
int dsp_svm_scan_device(dsp_svm *svm, const float *d_mfcc, long n_recordings, const long *frame_offsets, const dsp_scan_config *cfg,
                        int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream);
/* The whole chain: recordings back to back in HBM (offsets, channels and stereo_mode as dsp_mfcc_clips_ragged_device / _pcm16_device)
 * -> the ragged MFCC matrix and the windows' head rows in the scanner's grow-only workspace -> the scan, all enqueued on `stream`.  The
 * scanner borrows plan and SVM (destroy it first; the SVM's n_features must be 2 n_mfcc) and serves ONE stream at a time.  int16
 * input: the dsp_mfcc_scrubjay_infer_config front end and the 512-point framing's 13-coefficient shape (elsewhere DSP_EINVAL).     */
typedef struct dsp_scrubjay_scanner dsp_scrubjay_scanner;
int dsp_scrubjay_scanner_create(dsp_mfcc_plan *plan, dsp_svm *svm, const dsp_scan_config *cfg, dsp_scrubjay_scanner **out);
void dsp_scrubjay_scanner_destroy(dsp_scrubjay_scanner *scanner);
int dsp_scrubjay_scanner_run_device(dsp_scrubjay_scanner *scanner, const float *d_signal, long n_recordings, const long *offsets,
                                    int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream);
int dsp_scrubjay_scanner_run_pcm16_device(dsp_scrubjay_scanner *scanner, const int16_t *d_pcm, long n_recordings, const long *offsets,
                                          int channels, int stereo_mode, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                                          void *stream);

/* LIVE STREAMS: audio that is still arriving (the firmware's capture loop, sync/sync.cpp:188-213, for many feeds at once).  A stream
 * session holds N independent streams on one GPU.  Each push hands over the next chunk of every stream -- any length, zero included --
 * and returns the MFCC rows that became complete with it and the scores of the windows that became complete with those rows.
 * Concatenated over all pushes a stream's outputs are, bit for bit, what the entries above give on the whole recording: the rows of
 * dsp_mfcc_clips_ragged_device (no frame cap), and P("stop"), the Q8 speaker LLR mean and the label of dsp_scanner_run_device for every
 * stream that holds at least one full window.  How the audio was cut into chunks shows in no output bit.
 *
 * With FL = frame_length, H = hop_length, WF = window_frames, HF = hop_frames, per stream:
 *   N samples received so far give R(N) = N >= FL ? 1 + (N - FL) / H : 0 rows; row k is samples [k H, k H + FL) of the stream.  A push
 *   emits rows R(N before) .. R(N after) - 1.  The session carries the samples from R(N) H on to the next push: N - R(N) H of them,
 *   fewer than FL.
 *   E rows give W(E) = E >= WF ? 1 + (E - WF) / HF : 0 windows; window w is rows [w HF, w HF + WF).  A push emits windows
 *   W(E before) .. W(E after) - 1.  The session carries the rows from W(E) HF on: fewer than WF.
 * ONE DIFFERENCE from the scanner: a finished recording with fewer than WF rows gets one short window; a stream never ends, so it has
 * no window until it holds WF rows.  There is no "finish" call.
 *
 * Accepted: the plans dsp_scanner_create accepts (n_fft 512, DSP_LOG_PER_FRAME_MAX, DSP_FRAMING_COMPLETE, no prefilter; DSP_EINVAL with
 * the scanner's wording otherwise) with hop_length <= frame_length; hop_frames <= window_frames (a stream skips no input); stop model,
 * speaker model, both (n_coef / d = the plan's n_mfcc, on the plan's device, a stop window that fits the scan kernel) or neither -- then
 * the session yields rows only and `scan` is not read.  pcm16 = 0: float samples (channels must be 1); pcm16 != 0: int16 PCM, channels
 * and stereo_mode as dsp_mfcc_clips_ragged_pcm16_device (mono, stereo channel 0, stereo average), on the plans that entry takes int16
 * on (DSP_EINVAL here otherwise, not at the first push).  The format is fixed at creation: the carried samples stay in the caller's
 * format and are decoded by the kernel that decodes a whole recording.
 *
 * dsp_stream_push_plan (host only, no GPU, no session): what a push would emit.  received[n_streams] = samples per stream before the
 * push (NULL: all zero), chunk_offsets[n_streams + 1] = the chunks back to back (as dsp_mfcc_clips_ragged_device's offsets).  Fills
 * row_offsets and window_offsets [n_streams + 1], the prefix sums of the new rows / new windows (scan NULL: no windows; window_offsets
 * may be NULL).  Returns the new rows in total or a negative DSP_E* code.
 *
 * dsp_stream_push_device: d_chunks float or int16 (interleaved if stereo) as the session was created, chunk c = sample frames
 * [chunk_offsets[c], chunk_offsets[c + 1]).  d_mfcc[new rows][n_mfcc] in stream order, may be NULL when the caller wants scores only.
 * d_prob / d_llr_mean / d_labels[new windows] as dsp_scanner_run_device.  row_offsets / window_offsets: HOST arrays of n_streams + 1,
 * filled before a successful call returns (may be NULL).  Everything is enqueued on `stream`, no host synchronisation.  A refused push
 * leaves the session exactly as it was.  If a HIP call fails behind a push's first launch the session is broken: every later push
 * returns DSP_EHIP until dsp_stream_session_reset(session, NULL, ...).  Zero streams, or a push that completes no row and no window:
 * DSP_OK, no MFCC and no scan launch.
 * dsp_stream_session_reset: streams == NULL: all; else streams[n] name the streams whose samples, rows and counters are forgotten (a
 * new feed takes the slot).  Ordered with the pushes like any call on the session.  dsp_stream_session_counts: the host counters per
 * stream -- samples received, rows emitted, windows emitted; any may be NULL.
 * The session borrows plan and models (destroy it first) and owns its buffers; ONE stream at a time per session (and per speaker
 * model), as for a scanner.                                                                                                        */
typedef struct dsp_stream_session dsp_stream_session;
long dsp_stream_push_plan(const dsp_mfcc_config *mfcc, const dsp_scan_config *scan, const long *received, const long *chunk_offsets,
                          long n_streams, long *row_offsets, long *window_offsets);
int dsp_stream_session_create(dsp_mfcc_plan *plan, dsp_stop_model *stop, dsp_speaker_model *speaker, const dsp_scan_config *scan,
                              long n_streams, int channels, int stereo_mode, int pcm16, dsp_stream_session **out);
void dsp_stream_session_destroy(dsp_stream_session *session);
int dsp_stream_session_reset(dsp_stream_session *session, const long *streams, long n, void *stream);
int dsp_stream_session_counts(const dsp_stream_session *session, long *samples, long *rows, long *windows);
int dsp_stream_push_device(dsp_stream_session *session, const void *d_chunks, const long *chunk_offsets, float *d_mfcc, float *d_prob,
                           int64_t *d_llr_mean, int *d_labels, long *row_offsets, long *window_offsets, void *stream);

/* LIVE STREAMS AT ANOTHER RATE: the polyphase resampler below ("recordings at another rate") for feeds that are still arriving, on its
 * own or in front of a stream session.  With (up, down, half) as dsp_resample_ratio gives them, T = (2 half + up) / up
 * the taps of one polyphase branch, and N the sample frames a stream has received so far:
 *   output k reads input samples up to i_max(k) = (k down + half) div up, and no sample before i_max(k) - (T - 1);
 *   the stream has emitted K(N) = N up - 1 - half >= 0 ? (N up - 1 - half) div down + 1 : 0 outputs: exactly the k with i_max(k) <= N - 1.
 *   A push emits outputs K(N before) .. K(N after) - 1.  The stream carries the input frames from max(0, i_max(K(N)) - (T - 1)) on to
 *   the next push: at most T - 1 of them, in the caller's own format.
 * up = down = 1 copies: K(N) = N, nothing is carried, float bits pass through.
 * THE CONTRACT: concatenated over the pushes a stream's outputs are, bit for bit, the first K(N) outputs dsp_resample_ragged_device /
 * dsp_resample_ragged_pcm16_device give on the whole feed, for finite samples, whatever the chunk lengths, the other streams or the
 * batch.  (Both sum one float32 FMA chain per output in ascending input sample.  The chain's last slots multiply samples behind i_max
 * by zero taps; a stream that does not hold them yet uses 0.0 there, which changes no bit of a finite sum -- the one exception being a
 * sum every product of which underflows to -0.0, out of reach of int16 input.)
 * dsp_stream_resample_finish_device ends the named streams: it emits their outputs K(N) .. ceil(N up / down) - 1, with zeros for the
 * samples past the end as on a whole recording, and forgets the streams; pushes plus finish give the one-shot output in full.
 *
 * dsp_stream_resample_plan (host only, no GPU, no object): received[n_streams] (NULL: all zero) and chunk_offsets[n_streams + 1] (the
 * chunks back to back, as dsp_stream_push_plan's) -> out_offsets[n_streams + 1], the prefix sums of the new outputs; returns their total
 * or a negative DSP_E* code.  n_streams = 0: chunk_offsets may be NULL.
 * dsp_stream_resampler_create refuses, in this order and before it touches a GPU: out NULL; a bad PCM layout (pcm16 = 0: float
 * samples, channels must be 1; pcm16 != 0: channels and stereo_mode as dsp_resample_ragged_pcm16_device); rates below 1 or up / down
 * above 1024; a ratio whose branch is too long for the kernel to stage (down past ~450 with up = 1: thousands of carried samples per
 * stream are no live-feed shape; the one-shot entries take such ratios); n_streams outside [0, 2^31); then the device index.
 * dsp_stream_resample_push_device: d_chunks float or int16 (interleaved if stereo; int16 needs 2-byte alignment only), chunk c = sample
 * frames [chunk_offsets[c], chunk_offsets[c + 1]) -> the new outputs at d_out + out_offsets[c], back to back.  out_offsets: a HOST array
 * of n_streams + 1, filled before a successful call returns (may be NULL).  Everything is enqueued on `stream`, no host synchronisation:
 * one filter launch that reads each chunk byte once (the carried samples in front of it from the carry, never a stitched copy), one
 * copy launch that writes the new carry.  A refused push leaves the object as it was; a HIP failure behind the first launch breaks it
 * until dsp_stream_resampler_reset(rs, NULL, ...).  Zero streams, or a push that completes no output: DSP_OK, no filter launch.
 * _finish_device: streams[n] (each at most once), d_out / out_offsets[n + 1] in the order named.  _reset and _counts as the session's;
 * samples_out[s] = K(samples_in[s]); either may be NULL.  ONE stream at a time per object.
 *
 * dsp_stream_session_attach_resampler: DSP_EINVAL unless it is called before the session's first push, the session takes float mono
 * samples, n_streams and the device are equal and rate_out is the plan's sample_rate.  From then on dsp_stream_push_device takes chunks
 * at rate_in in the RESAMPLER's format, resamples them into a buffer the session owns and runs the push it always ran on the result;
 * dsp_stream_session_reset resets the same streams of the resampler, dsp_stream_session_counts keeps counting samples at the models'
 * rate.  The session borrows the resampler (destroy the session first); do not push to an attached resampler directly.            */
typedef struct dsp_stream_resampler dsp_stream_resampler;
long dsp_stream_resample_plan(int rate_in, int rate_out, const long *received, const long *chunk_offsets, long n_streams, long *out_offsets);
int dsp_stream_resampler_create(int device, int rate_in, int rate_out, long n_streams, int channels, int stereo_mode, int pcm16,
                                dsp_stream_resampler **out);
void dsp_stream_resampler_destroy(dsp_stream_resampler *rs);
int dsp_stream_resampler_reset(dsp_stream_resampler *rs, const long *streams, long n, void *stream);
int dsp_stream_resampler_counts(dsp_stream_resampler *rs, long *samples_in, long *samples_out);
int dsp_stream_resample_push_device(dsp_stream_resampler *rs, const void *d_chunks, const long *chunk_offsets, float *d_out,
                                    long *out_offsets, void *stream);
int dsp_stream_resample_finish_device(dsp_stream_resampler *rs, const long *streams, long n, float *d_out, long *out_offsets, void *stream);
int dsp_stream_session_attach_resampler(dsp_stream_session *session, dsp_stream_resampler *rs);

/* upsampleLinear (sync/particle/main.cpp:62-77) over a batch: d_out[c][i] for i < new_size from
 * d_in[c][0..old_size), the reference's fp32 operation order (bit-identical).  new_size >= 2.     */
int dsp_upsample_linear_device(const float *d_in, long n_clips, int old_size, long in_stride, float *d_out,
                               int new_size, long out_stride, void *stream);
int dsp_upsample_linear_host(const float *in, int old_size, float *out, int new_size);

/* --- recordings at another rate: rational-ratio polyphase FIR resampling ---
 * What scipy.signal.resample_poly(x, up, down) computes at its defaults (Kaiser beta = 5 window, zero padding, zero phase), so that audio
 * captured at 9 / 10 / 44.1 / 48 / 96 kHz reaches the 16 kHz the models run at without a host pass per file.  With g = gcd(rate_in,
 * rate_out): up = rate_out / g, down = rate_in / g, m = max(up, down), half = 10 m, and 2 half + 1 taps
 *   h[n] = up v[n] / sum_j v[j],   v[n] = sinc((n - half) / m) / m * I0(5 sqrt(1 - ((n - half) / half)^2)) / I0(5),   sinc(t) = sin(pi t) / (pi t)
 * (= firwin(2 half + 1, 1 / m, window=("kaiser", 5.0)) * up).  A recording x[0..n) gives ceil(n up / down) outputs
 *   y[k] = sum_i x[i] h[k down + half - i up]      over 0 <= i < n, 0 <= k down + half - i up <= 2 half.
 * The taps are computed in float64 on the host and rounded once to float32; products and sums are float32 (FMA), in ascending i -- an
 * order that depends on the recording and k only, never on the batch, the launch or the entry point.  up = down = 1 copies the input bit
 * for bit; n = 0 gives no output.  After reduction up and down must each be <= 1024 (DSP_EINVAL otherwise); a recording holds at most
 * INT_MAX samples.  Live feeds at another rate: dsp_stream_resample* above, which carry the filter's history between pushes.
 *
 * Host only, no GPU: dsp_resample_ratio (any pointer may be NULL); dsp_resample_taps (returns 2 half + 1; h may be NULL, else n >= that);
 * dsp_resample_offsets: offsets[n + 1] as dsp_mfcc_clips_ragged_device takes them -> out_offsets[n + 1], the prefix sums of the output
 * lengths from 0; returns their total.  Each returns a negative DSP_E* code on error.
 * dsp_resample_geometry (diagnostic, for tests): the block geometry the kernels run this ratio with, a function of (up, down) alone, as
 * ints in this order: up, down, half, taps (of one polyphase branch, T), row (T rounded up to 4), tile (consecutive outputs per block),
 * items (lane work items per block, tile / 4), span (input samples a tile reads), staged (1: the span is staged in LDS; 0: a branch too
 * long for it, samples read from global memory -- the ratios dsp_stream_resampler_create refuses), lds_bytes.  Returns the field count
 * (10); fields NULL asks for the count only, else n >= that.
 *
 * A dsp_resampler holds the taps of one ratio on one GPU.  dsp_resample_ragged_device: recording c = samples [offsets[c], offsets[c + 1])
 * per channel of d_in (`offsets` a HOST array, read before the call returns) -> d_out + out_offsets[c], back to back: d_out and those
 * offsets go unchanged into every *_ragged_* entry, scanner and per-clip entry above.  The pcm16 forms decode int16 in the load (mono
 * s / 32768; interleaved stereo: DSP_STEREO_CHANNEL0 / DSP_STEREO_AVERAGE as dsp_mfcc_clips_pcm16_device) and give, bit for bit, what
 * the float form gives on the decoded samples.  dsp_resample_clips_*: equal clips `stride` samples (per channel) apart ->
 * d_out[c * out_stride + k]; returns the output length of a clip.  Everything is enqueued on `stream`, no host synchronisation; ONE
 * stream at a time per resampler.  Zero recordings (or none with a sample): DSP_OK, no launch.
 * dsp_resample_host: one recording from host memory on GPU 0 (copy in, run, copy out); out holds ceil(n up / down) floats.            */
int dsp_resample_ratio(int rate_in, int rate_out, int *up, int *down, int *half_len);
int dsp_resample_geometry(int rate_in, int rate_out, int *fields, int n);
int dsp_resample_taps(int rate_in, int rate_out, double *h, int n);
long dsp_resample_offsets(int rate_in, int rate_out, const long *offsets, long n, long *out_offsets);
typedef struct dsp_resampler dsp_resampler;
int dsp_resampler_create(int device, int rate_in, int rate_out, dsp_resampler **out);
void dsp_resampler_destroy(dsp_resampler *r);
int dsp_resample_ragged_device(dsp_resampler *r, const float *d_in, long n, const long *offsets, float *d_out, void *stream);
int dsp_resample_ragged_pcm16_device(dsp_resampler *r, const int16_t *d_pcm, long n, const long *offsets, int channels, int stereo_mode,
                                     float *d_out, void *stream);
int dsp_resample_clips_device(dsp_resampler *r, const float *d_in, long n_clips, int samples, long stride, float *d_out, long out_stride,
                              void *stream);
int dsp_resample_clips_pcm16_device(dsp_resampler *r, const int16_t *d_pcm, long n_clips, int samples, long stride, int channels,
                                    int stereo_mode, float *d_out, long out_stride, void *stream);
int dsp_resample_host(int rate_in, int rate_out, const float *in, long n, float *out);

/* --- enrolling speakers: sliding CMVN and MAP-adapted GMM means ---
 * The step in front of dsp_speaker_model_create: a person's speech -> the target GMM's int8 means.  Both entries work on a ragged MFCC
 * matrix as dsp_mfcc_clips_ragged_device writes it, whatever front end produced it; frame_offsets is a HOST array of n + 1 rows, read
 * before the call returns.  Everything is enqueued on `stream`.
 *
 * Sliding CMVN (sliding_cmvn of the reference's speaker/gmm_utils.py:14-25, the feature space its UBM was trained in): recording r is
 * rows [frame_offsets[r], frame_offsets[r + 1]) of d_in[..][d], n rows.  With half = window / 2, row t uses rows [s, e) =
 * [max(0, t - half), min(n, t + half)) of its own recording -- rows t - 150 .. t + 149 at window 300 -- and, per coefficient j, in float32:
 *   mu = mean of x[s..e)[j],  sigma = sqrt(mean of (x[.][j] - mu)^2)  (two passes),  y[t][j] = (x[t][j] - mu) / (sigma + 1e-8)
 * A one-row recording and all-zero rows give exact zeros; recordings without rows give nothing; a row's output depends on its own
 * recording only.  d <= 16; window 2 .. 2048 (what one block's LDS image holds, 135 184 bytes at d = 16: DSP_EINVAL names the limit).  d_out must not be d_in.
 * No workspace and no host synchronisation: any stream.  Zero recordings: DSP_OK.                                                      */
typedef struct dsp_cmvn dsp_cmvn;
int dsp_cmvn_create(int device, int d, int window, dsp_cmvn **out);
void dsp_cmvn_destroy(dsp_cmvn *c);
int dsp_cmvn_ragged_device(dsp_cmvn *c, const float *d_in, long n_recordings, const long *frame_offsets, float *d_out, void *stream);

/* MAP enrolment of many speakers against one UBM (map_adapt_gmm of the reference's 2fa/audio/speaker/adapt_ubm.py:72-86 and
 * 2fa/audio/adapt_ubm.py:97-110; means only).  The float UBM is handed over once, as the DOUBLE_GMM arrays of gmm_params.inc:
 * log_consts[k] = log w_k - 0.5 sum_d log(2 pi var_kd), means[k][d], inv_covs[k][d] = 1 / var_kd; each is rounded once to float32.
 * Speaker s is rows [frame_offsets[s], frame_offsets[s + 1]) of d_feats[..][d] (CMVN'd rows: the offsets of several recordings of one
 * person are a subset of the recordings' boundaries).  Per row, in float32:
 *   l_k = log_const_k - 0.5 sum_d (x_d - mu_kd)^2 inv_cov_kd,   m = max_k l_k,  e_k = exp(l_k - m),  S = sum_k e_k,  p_k = e_k / S,  ll = m + log S
 * per speaker N_k = sum_t p_k, F_kd = sum_t p_k x_d, N'_k = N_k + 1e-8, alpha_k = N'_k / (N'_k + relevance_factor) or fixed_alpha, and
 *   mean_kd = alpha_k F_kd / N'_k + (1 - alpha_k) mu_kd.
 * Outputs (device pointers; any may be NULL, not all): d_means[S][k][d] float32; d_means_q6[S][k][d] = rint(mean * 64), ties to even,
 * saturated to [-128, 127] -- the Q6 means dsp_gmm_params takes, the target's inv_covs and log_consts being the UBM's own;
 * d_saturated[S] the entries so clamped; d_counts[S][k] = N_k; d_ll_mean[S] the mean of ll over the speaker's rows (sklearn's score).
 * A speaker without rows: DSP_EINVAL naming the first.  Zero speakers: DSP_OK, no launch.  There are no float atomics: a speaker's rows
 * are summed in chunks of 256 rows cut by its own row count and combined in a fixed order, so every output of a speaker is bit-identical
 * whatever the batch around it.  The enroller owns a grow-only workspace: ONE stream at a time per enroller.
 * Not covered: variance or weight adaptation, CMVN inside scanners or stream sessions (the UBM itself is trained by
 * dsp_ubm_train_device below, and the enrolled float means are scored by dsp_speaker_verify_ragged_device below that). */
typedef struct dsp_gmm_float_params {
    int k, d;                    /* k <= 64, d <= 16, as dsp_gmm_params */
    const double *log_consts;    /* [k]    */
    const double *means;         /* [k][d] */
    const double *inv_covs;      /* [k][d] */
} dsp_gmm_float_params;
enum { DSP_MAP_RELEVANCE = 0, DSP_MAP_FIXED_ALPHA = 1 };
typedef struct dsp_enroll_config {
    int map_mode;                /* DSP_MAP_RELEVANCE (alpha_k = N'_k / (N'_k + r)) or DSP_MAP_FIXED_ALPHA */
    float relevance_factor;      /* r > 0 (read in DSP_MAP_RELEVANCE); 16 in 2fa/audio/adapt_ubm.py        */
    float fixed_alpha;           /* in [0, 1] (read in DSP_MAP_FIXED_ALPHA); 0.7 in speaker/adapt_ubm.py   */
} dsp_enroll_config;
typedef struct dsp_speaker_enroller dsp_speaker_enroller;
int dsp_speaker_enroller_create(const dsp_gmm_float_params *ubm, int device, dsp_speaker_enroller **out);
void dsp_speaker_enroller_destroy(dsp_speaker_enroller *e);
int dsp_speaker_enroll_ragged_device(dsp_speaker_enroller *e, const float *d_feats, long n_speakers, const long *frame_offsets,
                                     const dsp_enroll_config *cfg, float *d_means, int8_t *d_means_q6, float *d_counts, float *d_ll_mean,
                                     int *d_saturated, void *stream);

/* --- training the UBM: EM for a diagonal GMM, and its integer tables ---
 * The step in front of dsp_speaker_enroller_create and dsp_speaker_model_create: feature rows of a population -> the float UBM the
 * enroller takes and the Q6 / Q11 / Q8 tables the integer scorer takes.  GaussianMixture(covariance_type="diag") of the reference's
 * 2fa/audio/speaker/train_ubm.py: sklearn's M-step (_estimate_gaussian_parameters) and its stopping rule, from a start the caller gives
 * or the library's deterministic one.
 *
 * Input: rows d_feats[n][d], float32 on the device, one flat matrix (CMVN'd rows of all recordings, stacked); k <= 64, d <= 16, n >= k.
 * The parameters w[k], mu[k][d], var[k][d] are float64 on the device between iterations.  Iteration i = 1, 2, ...:
 *   1. the E-step model, rounded once to float32: log_const_k = log w_k - 0.5 sum_d log(2 pi var_kd) (float64, then rounded),
 *      c_kd = float32(mu_kd), ic_kd = float32(1 / var_kd);
 *   2. per row, in float32, as the enroller: l_k = log_const_k - 0.5 sum_d (x_d - c_kd)^2 ic_kd (ascending d), m = max_k l_k,
 *      e_k = exp(l_k - m), S = sum_k e_k, p_k = e_k / S, ll = m + log S;
 *   3. over all rows, centred on c: N_k = sum_t p_k, F_kd = sum_t p_k (x_d - c_kd), G_kd = sum_t p_k (x_d - c_kd)^2, L = sum_t ll;
 *   4. in float64: N'_k = N_k + 10 DBL_EPSILON, r_k = N_k / N'_k, delta_kd = F_kd / N'_k, mean_kd = r_k c_kd + delta_kd,
 *      E2_kd = G_kd / N'_k + 2 c_kd delta_kd + r_k c_kd^2, var_kd = E2_kd - mean_kd^2 + reg_covar, w_k = N'_k / sum_j N'_j
 *      (a component no row visits gets mean 0, variance reg_covar and a weight of about 1e-15 / n, as in sklearn);
 *   5. lower_bound_i = L / n; stop after iteration i when | lower_bound_i - lower_bound_(i-1) | < tol (lower_bound_0 = -inf): converged = 1,
 *      n_iter = i; otherwise after max_iter iterations with converged = 0.  The model returned is the one AFTER the last M-step.
 * Sums: float32 inside a chunk of 256 rows (chunk c = rows [256 c, min(n, 256 c + 256)), the four waves' interleaved rows combined in
 * wave order), float64 above it in a fixed tree -- 16 consecutive chunks to a group, 32 consecutive groups to a super, the supers in
 * ascending order, every level in ascending order.  The tree depends on n alone: there are no float atomics, and a fit is bit-identical
 * whatever the grid, the device's CU count, the rows' address or what the workspace held before.  L is summed in float64 throughout.
 * The iterations are enqueued on `stream` without a host round trip each (every launch tests a stop flag on the device first); the host
 * looks at the flag every 32 iterations, and the call returns when the result is in the caller's arrays: dsp_ubm_train_device waits
 * for the stream, and so does dsp_ubm_init_rows_device, whose results are HOST arrays too.
 *
 * The start: dsp_ubm_init (weights > 0 that sum to 1 within 1e-6, means, variances > 0, all finite), or DSP_UBM_INIT_ROWS (NULL) for
 * the library's own, which dsp_ubm_init_rows_device also writes out: means_i = row floor((i + 0.5) n / k), variances = the rows' global
 * variance per dimension + reg_covar (one k = 1 iteration of the same kernels from mean = row floor(n / 2), variance 1), weights 1 / k.
 * sklearn's own start -- k-means++ seeding, Lloyd, the GMM of the labels, and n_init restarts of all of it -- is dsp_kmeans_* below, on
 * the same trainer: dsp_kmeans_train_ubm_device is the reference's whole GaussianMixture(...).fit call.
 *
 * dsp_ubm_result: the caller's arrays.  gmm is the dsp_gmm_float_params of the trained model (k and d are set, log_consts[k], means[k][d]
 * and inv_covs[k][d] = 1 / variances are written through the pointers, which must point at writable doubles): &result.gmm goes to
 * dsp_speaker_enroller_create and dsp_gmm_quantize unchanged.  lower_bounds[max_iter]: entries [0, n_iter) are written, the rest untouched.
 * dsp_ubm_trainer_create touches no device and allocates nothing; the trainer's workspace is grow-only: ONE stream at a time per trainer.
 *
 * dsp_gmm_quantize (host only, no GPU): any float GMM -> the tables of dsp_gmm_params in the integer scorer's formats,
 *   means = rint(64 mean) -> int8,  inv_covs = rint(2048 inv_cov) -> int32,  log_consts = rint(256 log_const) -> int16,
 * ties to even, each table saturated to its type; saturated[3] = the entries clamped in means, inv_covs, log_consts.  2048 / 1e-6 fits
 * int32; a reg_covar below about 9.6e-7 may not, which is what the count is for.
 * Covered below (dsp_kmeans_*): the k-means start and the n_init restarts.  Not covered: sklearn's random stream (the seeding draws
 * are this library's own, defined below), relocation of empty clusters, init_params="random", sample weights, mini-batch k-means,
 * full or tied covariances, variance and weight adaptation at enrolment, multi-GPU training (the statistics are summable, the tree is
 * not defined across devices), CMVN inside scanners or streams.  (The rows the reference trains on come from dsp_mfcc_speaker_config.) */
typedef struct dsp_ubm_init {
    const double *weights;       /* [k]    */
    const double *means;         /* [k][d] */
    const double *variances;     /* [k][d] */
} dsp_ubm_init;
#define DSP_UBM_INIT_ROWS ((const dsp_ubm_init *)0)
typedef struct dsp_ubm_config {
    int max_iter;                /* >= 1; 300 in train_ubm.py            */
    double tol;                  /* >= 0; sklearn's default 1e-3         */
    double reg_covar;            /* >= 0, finite; sklearn's default 1e-6 */
} dsp_ubm_config;
typedef struct dsp_ubm_result {
    dsp_gmm_float_params gmm;    /* k, d (set), log_consts[k], means[k][d], inv_covs[k][d] (written) */
    double *weights;             /* [k]        */
    double *variances;           /* [k][d]     */
    double *lower_bounds;        /* [max_iter] */
    int n_iter, converged;
} dsp_ubm_result;
typedef struct dsp_ubm_trainer dsp_ubm_trainer;
int dsp_ubm_trainer_create(int device, int k, int d, dsp_ubm_trainer **out);
void dsp_ubm_trainer_destroy(dsp_ubm_trainer *t);
int dsp_ubm_init_rows_device(dsp_ubm_trainer *t, const float *d_feats, long n, double reg_covar, double *weights, double *means,
                             double *variances, void *stream);
int dsp_ubm_train_device(dsp_ubm_trainer *t, const float *d_feats, long n, const dsp_ubm_init *init, const dsp_ubm_config *cfg,
                         dsp_ubm_result *result, void *stream);
int dsp_gmm_quantize(const dsp_gmm_float_params *g, int8_t *means, int32_t *inv_covs, int16_t *log_consts, int saturated[3]);

/* --- the k-means start of UBM training: k-means++ seeding, Lloyd, n_init restarts ---
 * What GaussianMixture(n_components=32, covariance_type="diag", max_iter=300, n_init=2) of the reference's train_ubm.py does before and
 * around EM (sklearn: init_params="kmeans"): three steps on a dsp_ubm_trainer, each usable on its own.  Rows, k, d and n as above; ONE
 * stream at a time per trainer.  The sums of all three go through the tree of dsp_ubm_train_device: chunk c = rows [256 c, 256 c + 256),
 * 16 consecutive chunks to a group, 32 consecutive groups to a super, the supers in ascending order -- a function of n alone, no float
 * atomics: every result below is the same bits whatever the grid, the CU count, the rows' address or what the workspace held before.
 *
 * 1. dsp_kmeans_seed_device: greedy k-means++, deterministic from a 64-bit seed -> rows[k], the chosen rows in the order chosen.
 *   Draws (counter-based: no state, recomputable anywhere):  mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
 *     0x94D049BB133111EB, z ^ z >> 31 (splitmix64's finaliser, 64-bit wrap-around);  u(seed, j, t) = (mix(seed + (8 j + t + 1) *
 *     0x9E3779B97F4A7C15) >> 11) * 2^-53, in [0, 1): j the step, t the trial.
 *   Trials: T = 2 + floor(ln k) per step (sklearn's n_local_trials; at most 6).
 *   Step 0: row floor(u(seed, 0, 0) n).
 *   m_i: the float32 squared distance of row i to the nearest chosen centre, sum_d (x_d - c_d)^2 over ascending d by fused
 *     multiply-add, kept in a device array.
 *   Sums of m: float64 from the row up.  Inside a chunk 16 segments of 16 consecutive rows, ascending in a segment and over the
 *     segments; then the tree above.
 *   Step j >= 1: pot = sum m_i.  Trial t proposes a row by walking r = u(seed, j, t) pot down the tree -- supers, then the super's
 *     groups, the group's chunks, the chunk's rows, each level ascending: the first child whose sum v exceeds r, else r -= v; a child
 *     with v = 0 is never taken (so never a row with m_i = 0, never a chosen row or a copy of one); where rounding walks r past the last
 *     child, the last child with v > 0, and likewise below it.  The trial whose new potential sum_i min(m_i, |x_i - x_cand|^2) is
 *     smallest wins, ties to the lowest t.
 *   pot = 0 with centres left to choose: the matrix has fewer than k distinct rows; the call fails with DSP_EINVAL and a message that
 *     says so (a flag on the device, read at the end), and the trainer stays usable.
 *   The whole seeding is enqueued without a host round trip; per step one pass over the rows (fold the last winner into m, evaluate
 *   the T proposals, leave T sets of sums) and one small launch (the winner; its sums are the next step's tree; the next proposals).
 *
 * 2. dsp_kmeans_fit_device: Lloyd from centres0[k][d] (host float64, finite; typically the seed rows), and the GMM the labels give.
 *   Iteration i = 1, 2, ... from the float64 centres:
 *   1. c = float32(centre), rounded once;
 *   2. per row, in float32: s_k = sum_d (x_d - c_kd)^2 (ascending d, fused multiply-add); label = the k of the smallest s_k, ties to
 *      the lowest k;
 *   3. over the rows labelled k, centred on c: N_k, F_kd = sum (x_d - c_kd), G_kd = sum (x_d - c_kd)^2; the inertia sum s_label;
 *      and the number of rows whose label differs from the previous iteration's (all of them in iteration 1).  float32 inside a chunk
 *      (the four waves' interleaved rows combined in wave order), float64 above it, as EM's;
 *   4. in float64: centre'_kd = c_kd + F_kd / N_k.  A cluster with N_k = 0 keeps its centre: sklearn relocates such a cluster to the
 *      row farthest from its centre, this library does not (n_empty reports them);
 *   5. stop after iteration i when no label changed (DSP_KMEANS_STOP_STRICT, tested first, as in sklearn), else when
 *      sum_kd (centre' - centre)^2 <= tol * mean_d var_d(x) (DSP_KMEANS_STOP_TOL; var_d: the rows' global variance, computed once per
 *      call as dsp_ubm_init_rows_device does), else after max_iter iterations (DSP_KMEANS_STOP_MAX_ITER);
 *   6. after the stop one more pass labels the rows against the final centres (sklearn does so unless the stop was strict, where it
 *      changes nothing) and takes N, F, G and the inertia; step 4 of dsp_ubm_train_device on them, with p in {0, 1}, gives the GMM
 *      start: weights, means and variances + reg_covar -- sklearn's _initialize for init_params="kmeans".  An empty cluster is that
 *      step's component no row visits.
 *   The iterations are enqueued as EM's are: every launch tests a stop flag first, the host looks every 32 iterations.
 *   dsp_kmeans_result: centres[k][d] (the final centres, float64), counts[k], the GMM start weights[k], means[k][d], variances[k][d]
 *   (the caller's arrays, none NULL; the three are a dsp_ubm_init as they are), inertia, n_iter, stop, n_empty;  d_labels[n] (int32
 *   on the device) may be NULL.
 *
 * 3. dsp_kmeans_train_ubm_device: the reference's call.  For r = 0 .. n_init - 1: seed with seed_r = mix((seed ^ 0xD1B54A32D192ED03)
 *   + (r + 1) * 0x9E3779B97F4A7C15); Lloyd from those rows (kmeans_max_iter, kmeans_tol, em.reg_covar), whose final pass writes the
 *   GMM start straight into the trainer's device parameters and float32 model -- no host copy between k-means and EM; EM exactly as
 *   dsp_ubm_train_device runs it (em).  The model returned in dsp_ubm_result (unchanged) is the restart whose last lower bound is the
 *   largest, ties to the first: sklearn's rule.  report->restarts[n_init] (the caller's array) says what each restart did,
 *   report->winner which one was kept.
 *
 * Every result of the three calls that is not marked "on the device" is a HOST value: each call waits for the stream before it returns. */
#define DSP_KMEANS_STOP_MAX_ITER 0
#define DSP_KMEANS_STOP_TOL 1
#define DSP_KMEANS_STOP_STRICT 2
typedef struct dsp_kmeans_config {
    int max_iter;                /* >= 1; sklearn's default 300          */
    double tol;                  /* >= 0, finite; sklearn's default 1e-4 */
    double reg_covar;            /* >= 0, finite; of the GMM start       */
} dsp_kmeans_config;
typedef struct dsp_kmeans_result {
    double *centres;             /* [k][d] */
    long *counts;                /* [k]    */
    double *weights;             /* [k]    the GMM start */
    double *means;               /* [k][d] */
    double *variances;           /* [k][d] */
    int *d_labels;               /* [n] on the device, may be NULL */
    double inertia;
    int n_iter, stop, n_empty;
} dsp_kmeans_result;
typedef struct dsp_kmeans_ubm_config {
    int n_init;                  /* >= 1; 2 in train_ubm.py */
    uint64_t seed;
    int kmeans_max_iter;         /* >= 1; sklearn's 300     */
    double kmeans_tol;           /* >= 0, finite; 1e-4      */
    dsp_ubm_config em;
} dsp_kmeans_ubm_config;
typedef struct dsp_kmeans_restart {
    long rows[64];               /* the seed rows, [0, k) written */
    int kmeans_n_iter, kmeans_stop, kmeans_n_empty;
    int em_n_iter, em_converged;
    double lower_bound;          /* EM's last */
} dsp_kmeans_restart;
typedef struct dsp_kmeans_ubm_report {
    dsp_kmeans_restart *restarts;        /* [n_init], the caller's */
    int winner;
} dsp_kmeans_ubm_report;
int dsp_kmeans_seed_device(dsp_ubm_trainer *t, const float *d_feats, long n, uint64_t seed, long *rows, void *stream);
int dsp_kmeans_fit_device(dsp_ubm_trainer *t, const float *d_feats, long n, const double *centres0, const dsp_kmeans_config *cfg,
                          dsp_kmeans_result *result, void *stream);
int dsp_kmeans_train_ubm_device(dsp_ubm_trainer *t, const float *d_feats, long n, const dsp_kmeans_ubm_config *cfg, dsp_ubm_result *result,
                                dsp_kmeans_ubm_report *report, void *stream);

/* --- verifying speakers with the float GMMs: every clip against every speaker ---
 * The step behind enrolment: target.score(feats) - ubm.score(feats) of the reference's 2fa/audio/speaker/gmm_utils.py:99-126
 * (score_models, evaluate_dir) and evaluate_gmm.py, both terms the mean log-sum-exp log-likelihood of a float GMM -- for C clips against
 * S speakers in one call, in the arithmetic the models were trained and adapted in.
 *
 * Inputs: the float UBM (handed over once, each value rounded once to float32: lc[k], mu[k][d], ic[k][d]); clip c = rows
 * [frame_offsets[c], frame_offsets[c + 1]) of d_feats[..][d], rows that are already CMVN'd (frame_offsets: a HOST array of n_clips + 1
 * rows, read before the call returns); d_means[S][k][d], the float32 means of S enrolled speakers on the device, exactly what
 * dsp_speaker_enroll_ragged_device writes.  Speaker s is the model (lc, d_means[s], ic): mean-only MAP shares the UBM's log_consts and
 * inv_covs.  k <= 64, d <= 16.
 *
 * Per row x and model with centres c (the UBM: c = mu), in float32:
 *   s = 0; for ascending j: dv = x_j - c_kj, s = fma(dv * dv, ic_kj, s);   l_k = fma(-0.5, s, lc_k)       (the enroller's l_k, bit for bit)
 *   m = max_k l_k,   S = sum_k expf(l_k - m) over ASCENDING k,   ll = m + logf(S)
 * Per clip of n rows and model, L = sum_t (double) ll_t in an order fixed by n alone: the rows are cut into tiles of 64 from the clip's
 * first row; inside a tile the sum is the adjacent pairwise tree (1, 2, 4, ... 32 apart, absent rows 0); the tiles are added in
 * ascending order.  There are no atomics.  With L_u the UBM's sum and L_s speaker s's:
 *   d_ll_ubm[c] = float(L_u / n),  d_ll_target[c][s] = float(L_s / n),  d_llr[c][s] = float((L_s - L_u) / n)   (the difference in float64)
 *   d_best[c] = the smallest s with the largest d_llr[c][s],  d_best_llr[c] = that value
 * Every output of a (clip, speaker) pair is bit-identical whatever the batch around the clip, the other speakers of the call, the
 * speaker's position in d_means, the grid and what the workspace held before.
 *
 * Any output may be NULL, not all.  A clip without rows: DSP_EINVAL naming the first.  n_clips == 0 or n_speakers == 0: DSP_OK, no
 * launch.  At most 2^30 clips and 2^19 speakers per call.  Every argument check comes before a device is touched;
 * dsp_speaker_verifier_create touches none (the UBM is uploaded by the first call that scores).  The verifier owns a grow-only
 * workspace of tile sums, [tiles][1 + S] doubles: ONE stream at a time per verifier.  A call whose workspace would pass 256 MiB is split
 * over runs of clips internally, on the same stream; the outputs do not change.
 * Not covered: per-speaker variances or weights (mean-only MAP is what enrolment writes), a trial LIST instead of the full C x S
 * matrix, CMVN inside the call (dsp_cmvn_ragged_device in front), multi-GPU (split the clips or the speakers across verifiers).  Long
 * recordings are scanned window by window by dsp_speaker_float_scan_device below. */
typedef struct dsp_speaker_verifier dsp_speaker_verifier;
int dsp_speaker_verifier_create(const dsp_gmm_float_params *ubm, int device, dsp_speaker_verifier **out);
void dsp_speaker_verifier_destroy(dsp_speaker_verifier *v);
int dsp_speaker_verify_ragged_device(dsp_speaker_verifier *v, const float *d_feats, long n_clips, const long *frame_offsets,
                                     const float *d_means, long n_speakers,
                                     float *d_llr,        /* [C][S]                       */
                                     float *d_ll_ubm,     /* [C]      may be NULL         */
                                     float *d_ll_target,  /* [C][S]   may be NULL         */
                                     int *d_best,         /* [C]      may be NULL         */
                                     float *d_best_llr,   /* [C]      may be NULL         */
                                     void *stream);

/* SCANNING LONG RECORDINGS with the float GMMs: the same scores per sliding window and speaker -- who speaks when.
 * Recording r is rows [frame_offsets[r], frame_offsets[r + 1]) of d_feats[..][d] (frame_offsets: a HOST array of n_recordings + 1 rows,
 * read before the call returns), rows that are already CMVN'd over the RECORDING, not over a window (dsp_cmvn_ragged_device in front).
 * The windows are those of dsp_scan_config / dsp_scan_window_offsets above: R >= window_frames rows give 1 + (R - window_frames) /
 * hop_frames windows, window w = rows [w hop_frames, w hop_frames + window_frames); fewer rows one window of all R.  The windows of all
 * recordings lie back to back, Wt in all.  d_means[S][k][d] as dsp_speaker_verify_ragged_device takes them.
 *
 * Per row and model, ll is dsp_speaker_verify_ragged_device's, bit for bit, computed ONCE per row of a run (not once per window it
 * lies in).  Per window of n rows and model, L is the float64 sum of the window's ll in the per-clip entry's order, applied to the
 * window as if it were a clip: tiles of 64 rows cut from the WINDOW's first row, the adjacent pairwise tree inside a tile (absent rows
 * 0), the tiles added in ascending order.  The five outputs are formed from L_u, L_s and n as above.  So every output of window w
 * equals, bit for bit, what dsp_speaker_verify_ragged_device gives for the same rows handed over as a clip of their own -- whatever the
 * batch, the other speakers, a speaker's position, the grid, the split and what the workspace held.  There are no atomics.
 *
 * Any output may be NULL, not all.  DSP_EINVAL, before a device is touched: cfg NULL or window_frames / hop_frames < 1; a NULL d_feats,
 * d_means or frame_offsets; offsets that are negative or decrease; a recording without rows (the first is named); more than 2^19
 * speakers or 2^30 recordings.  n_recordings == 0 or n_speakers == 0: DSP_OK, no launch, no device.  The verifier's grow-only
 * workspace, shared with the per-clip entry, holds float ll[1 + S][rows of a run]: ONE stream at a time per verifier.  A call whose
 * ll would pass 256 MiB is cut into runs of consecutive windows (a window is never cut; rows shared by two runs are scored in both),
 * on the same stream; the outputs do not change.  Rows that lie in no window (hop_frames > window_frames, the tail behind a
 * recording's last window) are not scored.
 * Not covered: stream sessions (sliding CMVN looks ahead) and a scanner from audio (under the speaker plan a recording's rows depend
 * on the whole recording: compute its features, then scan -- INTEGRATION.md 6i).  Thresholds and segments on top of the scores:
 * dsp_segments_device below. */
int dsp_speaker_float_scan_device(dsp_speaker_verifier *v, const float *d_feats, long n_recordings, const long *frame_offsets,
                                  const dsp_scan_config *cfg, const float *d_means, long n_speakers,
                                  float *d_llr,        /* [Wt][S]                 */
                                  float *d_ll_ubm,     /* [Wt]     may be NULL    */
                                  float *d_ll_target,  /* [Wt][S]  may be NULL    */
                                  int *d_best,         /* [Wt]     may be NULL    */
                                  float *d_best_llr,   /* [Wt]     may be NULL    */
                                  void *stream);

/* SEGMENTS FROM WINDOW SCORES: hysteresis, gap merge, minimum length -- "speaker 17, recording 4, windows 7510 .. 7780" instead of one
 * number per window.  Every scan above feeds it unchanged: d_scores[Wt][S] float32, row-major, the
 * windows of all recordings back to back as window_offsets (the HOST array dsp_scan_window_offsets fills, read before the call returns)
 * says -- S = 1 for d_prob of the stop scans and d_prob1 / d_decision of the SVM scan, S = n_speakers for d_llr of the float scan.
 *
 * A track is one (recording r, column s): x[w], w = 0 .. W_r - 1.
 *   1. e[w] = x[w] (DSP_SEG_INDEPENDENT), or x[w] where s is the row's best column and -inf elsewhere (DSP_SEG_EXCLUSIVE).  The best
 *      column is the smallest that attains the maximum of the row's non-NaN entries -- the scan's d_best; a row of NaN has none.
 *   2. state[-1] = 0; state[w] = 1 if e[w] >= on; 0 if !(e[w] >= off) (NaN lands here); else state[w - 1].
 *   3. A run is a maximal stretch of state 1.
 *   4. Consecutive runs with at most max_gap windows between them are joined, the gap included -- once, before anything is dropped.
 *   5. What spans n_windows = last - first + 1 < min_windows is dropped; its neighbours are not joined again.
 *   6. Per survivor, over its ACTIVE windows (state 1: never NaN, never masked): n_active, peak = max x, peak_window = the first window
 *      that attains it (an index within the recording), mean = (float)(float64 sum of x / n_active).
 * The output is ordered by (recording, column, first_window) through prefix sums of the per-track counts: no atomic places a segment,
 * and every field of every segment is the same bits whatever the batch, the recording's position in it, the other columns
 * (DSP_SEG_INDEPENDENT), max_segments, the outputs asked for, the stream and what the workspace held.  The float64 sum is taken in an
 * order that depends on the segment alone.
 *
 * d_segments may be NULL (max_segments ignored): count only.  When more segments are found than max_segments, the first max_segments
 * in output order are written and nothing behind them; d_total[0] = segments found, d_total[1] = segments written, both on the device.
 * d_track_counts[n_recordings][n_columns] (may be NULL) = survivors per track.  Everything is enqueued on `stream`; nothing waits.
 * The segmenter owns a grow-only workspace (Wt S / 4 bytes and 24 bytes per 512 windows of a track): ONE stream at a time per segmenter.
 *
 * DSP_EINVAL, before a device is touched: cfg NULL; on or off NaN, or off > on; min_windows < 1; max_gap < 0; an unknown mode; a NULL
 * d_scores, window_offsets or d_total; offsets that are negative or decrease; n_columns < 1 or > 2^19; a non-NULL d_segments with
 * max_segments < 0; a recording of 2^31 windows or more; 2^31 tracks or more.  n_recordings == 0: DSP_OK, no launch, and d_total is
 * NOT written (nothing is enqueued: zero it beforehand where it is read regardless).  A recording without windows is legal and
 * yields nothing.
 *
 * dsp_segments_capacity (host only): the most segments a call can find, sum over recordings of S floor((W_r + max_gap + 1) /
 * (min_windows + max_gap + 1)) -- k survivors of one track need k min_windows + (k - 1) (max_gap + 1) <= W_r windows; < 0: DSP_E*.
 * dsp_segment_sample_spans (host only): starts / lengths[n_segments] (either may be NULL) = each segment in samples, from the start of
 * its first window to the end of its last, absolute positions in the buffer (offsets as dsp_mfcc_clips_ragged_device).  The windows
 * are dsp_scan_window_spans' under DSP_FRAMING_COMPLETE and DSP_FRAMING_STREAM; under DSP_FRAMING_CENTER (the speaker plan, which
 * dsp_scan_window_spans refuses) row i covers samples [i hop_length - frame_length / 2, i hop_length + frame_length / 2) and a window its
 * rows' union, clipped to the recording.  A segment outside its recording's windows is DSP_EINVAL; returns n_segments.
 * Not covered: a threshold per column, int64 Q8 scores (dsp_speaker_scan_device's: convert to float, exact below 2^24), segments
 * carried across the pushes of a stream session.                                                                                    */
#define DSP_SEG_INDEPENDENT 0
#define DSP_SEG_EXCLUSIVE 1
typedef struct dsp_segment_config {
    float on;            /* a window with score >= on switches its track on                          */
    float off;           /* a window with !(score >= off) switches it off; off <= on                 */
    int   min_windows;   /* >= 1: segments spanning fewer windows are dropped                        */
    int   max_gap;       /* >= 0: runs of one track separated by <= max_gap off windows are joined   */
    int   mode;          /* DSP_SEG_INDEPENDENT | DSP_SEG_EXCLUSIVE                                  */
} dsp_segment_config;
typedef struct dsp_segment {          /* 32 bytes */
    int recording, column, first_window, n_windows, n_active, peak_window;
    float peak, mean;
} dsp_segment;
typedef struct dsp_segmenter dsp_segmenter;
int dsp_segmenter_create(int device, dsp_segmenter **out);
void dsp_segmenter_destroy(dsp_segmenter *s);
long dsp_segments_capacity(const dsp_segment_config *cfg, const long *window_offsets, long n_recordings, long n_columns);
int dsp_segments_device(dsp_segmenter *s, const float *d_scores, long n_recordings, const long *window_offsets, long n_columns,
                        const dsp_segment_config *cfg,
                        dsp_segment *d_segments, long max_segments,   /* may be NULL / 0: count only            */
                        int *d_track_counts,                          /* [n_recordings][n_columns], may be NULL */
                        long *d_total,                                /* [2]: segments found, segments written  */
                        void *stream);
long dsp_segment_sample_spans(const dsp_mfcc_config *mfcc, const dsp_scan_config *scan, const long *offsets, long n_recordings,
                              const dsp_segment *segments, long n_segments, long *starts, long *lengths);

/* LABELLED TRIALS: threshold sweep, ROC counts, AUC -- the number every consumer of the scores above needs and none of them produces
 * (2fa/audio/speaker/evaluate_gmm.py:73-81, generate_charts.py:52-54,68-69).  d_scores[T][S]
 * float32, row-major, on the device: d_llr of dsp_speaker_verify_ragged_device (T clips) or of dsp_speaker_float_scan_device (T = Wt).
 * truth[T] is a HOST array read before the call returns: truth[r] = the column that is row r's true speaker, -1: none of the enrolled.
 *
 * Trial (r, s) is a target trial when truth[r] == s and a non-target trial otherwise.  A NaN score takes its trial out of everything
 * (it is counted in n_nan).  Per column s, P targets and N non-targets, both without the NaN ones:
 *   1. Sweep.  lo / hi = min / max of the column's FINITE scores as float64, NaN without one (of -0 and +0, lo takes -0 and hi +0).
 *      step = (hi - lo) / (n - 1); t_i = i step + lo for i < n - 1, two roundings, never a fused multiply-add; t_(n-1) = hi --
 *      np.linspace(lo, hi, n), n = n_thresholds.  tp_i = the targets with (double)x > t_i, fp_i the non-targets (NaN thresholds:
 *      zeros; +inf is above every threshold, -inf above none).  correct_i = tp_i + (N - fp_i); best_index = the smallest i that
 *      attains the maximum (np.argmax), best_threshold = t_best_index, best_correct = that maximum.
 *   2. ROC counts.  The target trials of all columns lie back to back in (column, row) order, column s at [target_offsets[s],
 *      target_offsets[s + 1]) (dsp_trials_target_offsets; a NaN target keeps its place).  For target j of column s: fa_above[j] =
 *      the non-targets of the column with x > x_j, fa_equal[j] = those with x == x_j; -1 and -1 for a NaN target.  That is the
 *      exact step curve: at "accept when x >= x_j" the false accepts are above + equal.
 *   3. AUC.  auc_u2 = sum over the non-NaN targets of 2 (N - above - equal) + equal -- twice the wins plus the ties, an int64;
 *      auc = (double)auc_u2 / (double)(2 P N), NaN when P N == 0.
 * Row S of d_columns and of the sweep is the POOLED row: lo / hi over every finite score of the matrix and the sweep over all T S
 * trials (one threshold for the whole system); auc_u2 = the sum of the columns', auc = auc_u2 / (2 sum_s P_s N_s), the within-speaker
 * AUC weighted by pairs.
 *
 * Every output is an integer count or one correctly rounded float64 operation on such counts and on lo / hi: all of them are the
 * same bits whatever the other columns, the batch, the grid, the outputs asked for, the stream and what the workspace held.  The
 * kernels add with integer atomics only.
 *
 * Any output may be NULL, not all of them; what no output needs is not launched: the sweep outputs alone count no pairs, the ROC
 * arrays alone take no min / max and no histogram, d_columns needs both (and fills auc without the ROC arrays).  Everything is
 * enqueued on `stream`; nothing waits.  The evaluator owns a grow-only workspace (32 bytes and 8 (n + 1) + 16 bytes per column, 12
 * bytes per target): ONE stream at a time per evaluator.  dsp_trial_evaluator_create touches no device.
 *
 * DSP_EINVAL, before a device is touched, the first of: e NULL; cfg NULL; n_thresholds outside 2 .. 1024; n_columns outside
 * 1 .. 2^19; n_rows < 0 or >= 2^31; every output NULL; (n_rows == 0: DSP_OK here, no launch, nothing written;) d_scores NULL; truth
 * NULL; the first truth[r] < -1 or >= n_columns, named; 2^45 trials or more; and, where d_columns or a ROC array is asked for, more
 * than 2^46 pairs of a target and a non-target (sum_s P_s (T - P_s), dsp_trials_pairs), with the number.  Pair counting is exact and
 * its time grows with the pairs: the cap only bounds it, and nobody has measured a call at the cap -- tools/time_trials.py records
 * the time per pair at the sizes it runs.
 *
 * dsp_trials_target_offsets (host only): target_offsets[S + 1] and target_rows[targets] (either may be NULL), the rows of column
 * s's targets ascending; returns the number of targets (rows with truth >= 0).  dsp_trials_pairs (host only): sum_s P_s N_s before
 * any NaN is known.  Both < 0: DSP_E*.
 * The caps above bound the kernels' indices, not the memory a call takes; that is the caller's to size.  Per call the workspace holds
 * and clears 8 S (n + 1) bytes of histograms -- 1.6 MB at 1 000 speakers and 200 thresholds, but 4.3 GB at S = 2^19 with n = 1024 --
 * and the labels travel through 4 (T + targets) + 8 (S + 1) bytes of pinned host memory and as many on the device: 0.8 MB at 100 000
 * clips, 16 GB near T = 2^31.  A workspace the device cannot give is DSP_ENOMEM, a pinned buffer the host cannot give DSP_EHIP.
 * Not covered: a threshold per column in the segmenter, the equal error rate, pair counts pooled across columns.                   */
typedef struct dsp_trials_config { int n_thresholds; } dsp_trials_config;           /* 2 .. 1024; 200 = evaluate_gmm.py */
typedef struct dsp_trial_column {                                                   /* 80 bytes: one per column, and one pooled */
    long n_target, n_nontarget, n_nan;
    double lo, hi, best_threshold;
    long best_correct, auc_u2;
    double auc;
    int best_index, reserved;
} dsp_trial_column;
typedef struct dsp_trial_evaluator dsp_trial_evaluator;
long dsp_trials_target_offsets(const int *truth, long n_rows, long n_columns, long *target_offsets, long *target_rows);
long dsp_trials_pairs(const int *truth, long n_rows, long n_columns);
int dsp_trial_evaluator_create(int device, dsp_trial_evaluator **out);
void dsp_trial_evaluator_destroy(dsp_trial_evaluator *e);
int dsp_trials_evaluate_device(dsp_trial_evaluator *e, const float *d_scores, long n_rows, long n_columns, const int *truth,
                               const dsp_trials_config *cfg,
                               dsp_trial_column *d_columns,           /* [S + 1]                        may be NULL */
                               long *d_sweep_tp, long *d_sweep_fp,    /* [S + 1][n_thresholds]          may be NULL */
                               int *d_fa_above, int *d_fa_equal,      /* [targets in all]               may be NULL */
                               void *stream);

/* SCORE CALIBRATION: fit c = A x + B + C log(n_frames) on labelled trials, apply it -- the duration calibration of
 * 2fa/audio/speaker/adapt_ubm.py:97-99, whose constants (CAL_A, CAL_B, CAL_C = 1, 0, 0, "to be learned on dev set", :27-28) the
 * reference never learns.  d_scores[T][S] and truth[T] are those of dsp_trials_evaluate_device;
 * n_frames[T] is a HOST array, the rows a trial's score was averaged over (the differences of frame_offsets behind
 * dsp_speaker_verify_ragged_device, the window length behind dsp_speaker_float_scan_device), or NULL: the two-parameter model, C = 0
 * and not fitted.  truth and n_frames are read before the call returns.
 *
 * Duration term.  l_r = log((double)n_frames[r] + 1e-8), the C library's log on the host; dsp_calibration_duration_term (host only)
 * writes exactly the values the library uses to out[T].
 * Model.  For trial (r, s) with score x: c = A x + B + C l_r.  A trial whose score is NaN or +-inf takes no part in the fit and is
 * counted in n_excluded; P targets and N non-targets remain.
 * Objective.  With tau = log(prior / (1 - prior)):
 *   J = prior / P sum_targets softplus(-(c + tau)) + (1 - prior) / N sum_nontargets softplus(c + tau)
 * (softplus(z) = max(z, 0) + log1p(exp(-|z|)); at prior = 0.5, J / ln 2 is Cllr).
 * Iteration.  Damped Newton; one pass over the matrix gives J, the gradient g and the Hessian H at theta = (A, B[, C]).
 *   1. theta = init (NULL: 1, 0, 0); no step is pending.
 *   2. After a pass at theta: if a step is pending and !(J <= J_base), the pass is rejected: h += 1, theta = base - d / 2^h; more than
 *      30 halvings end the fit, DSP_CAL_STALLED, theta = base.
 *   3. Else the pass is accepted.  If a step was pending and max |theta - base| <= tol: DSP_CAL_CONVERGED at this theta.
 *   4. Else base = theta, J_base = J, h = 0, and H d = g is solved by Cholesky in float64.  A pivot <= 0 or a non-finite J, g, H or d:
 *      DSP_CAL_SINGULAR, theta = base.
 *   5. Else theta = base - d, which is pending.
 *   6. Rejected passes count among max_iter; running out: DSP_CAL_MAX_ITER, theta = base.
 *   7. P == 0 or N == 0 after the first pass: DSP_CAL_NO_CLASS, theta = init, objective and objective_start NaN.
 * The report: params = theta at the end; objective = J there; objective_start = J at init; last_step = max |theta - base| of the last
 * accepted step (NaN: none); n_iter = passes made, n_rejected those rejected.
 * Every sum is float64 over a tree that depends on (T, S) alone, without float atomics: a report is the same bits whatever the
 * stream, the repeats and what the workspace held.
 *
 * dsp_calibration_fit_device enqueues max_iter passes without a host round trip (those behind the end leave at once), waits for the
 * stream ONCE and returns with *report filled.  dsp_calibration_apply_device only enqueues:
 *   d_out[r][s] = (float)(A (double)x + B + C l_r), float64 products and sums from left to right, never fused, rounded once;
 * without n_frames the last term is left out.  NaN stays NaN.  d_out == d_scores is allowed.  The output is a score matrix like its
 * input: dsp_trials_evaluate_device and dsp_segments_device take it unchanged.
 * The calibrator owns a grow-only workspace (184 bytes per 1 024 trials of a matrix below 32 columns, per 16 384 from there on) and
 * the labels travel through 12 T bytes of pinned host memory and as many on the device: ONE stream at a time per calibrator.
 * dsp_calibrator_create touches no device.
 *
 * DSP_EINVAL, before a device is touched, the first of -- fit: c NULL; cfg NULL; prior not inside (0, 1); tol not > 0; max_iter
 * outside 1 .. 10 000; report NULL; n_columns outside 1 .. 2^19; n_rows < 0 or >= 2^31; a non-finite init; init->c != 0 without
 * n_frames; (n_rows == 0: DSP_OK here, no launch, the report DSP_CAL_NO_CLASS with n_iter 0;) d_scores NULL; truth NULL; the first
 * truth[r] < -1 or >= n_columns, named; the first n_frames[r] < 0, named; 2^45 trials or more.  apply: c NULL; params NULL or
 * non-finite; n_columns, n_rows as above; params->c != 0 without n_frames; (n_rows == 0: DSP_OK, no launch;) d_scores NULL; d_out
 * NULL; the first n_frames[r] < 0, named; 2^45 trials or more.  dsp_calibration_duration_term: n_rows < 0; n_frames or out NULL with
 * n_rows > 0; the first n_frames[r] < 0, named.
 * Not covered: a calibration per column (one theta serves the matrix), regularisation of theta (separable scores end
 * DSP_CAL_SINGULAR or DSP_CAL_MAX_ITER with a large finite A), the equal error rate.                                              */
#define DSP_CAL_CONVERGED 0
#define DSP_CAL_MAX_ITER 1
#define DSP_CAL_STALLED 2
#define DSP_CAL_SINGULAR 3
#define DSP_CAL_NO_CLASS 4
typedef struct dsp_calibration { double a, b, c; } dsp_calibration;                 /* 1, 0, 0: the reference's constants */
typedef struct dsp_calibration_config {
    double prior;        /* inside (0, 1): the weight of the target class; 0.5 = Cllr */
    double tol;          /* > 0: the fit ends when an accepted step moves no parameter by more */
    int    max_iter;     /* 1 .. 10 000 passes over the matrix */
    int    reserved;
} dsp_calibration_config;
typedef struct dsp_calibration_report {                                             /* 88 bytes */
    dsp_calibration params;
    long n_target, n_nontarget, n_excluded;
    double objective_start, objective, last_step;
    int n_iter, n_rejected, status, reserved;
} dsp_calibration_report;
typedef struct dsp_calibrator dsp_calibrator;
int dsp_calibrator_create(int device, dsp_calibrator **out);
void dsp_calibrator_destroy(dsp_calibrator *c);
int dsp_calibration_duration_term(const long *n_frames, long n_rows, double *out);
int dsp_calibration_fit_device(dsp_calibrator *c, const float *d_scores, long n_rows, long n_columns, const int *truth,
                               const long *n_frames,                  /* [T] on the host, may be NULL: A and B only */
                               const dsp_calibration_config *cfg,
                               const dsp_calibration *init,           /* may be NULL: 1, 0, 0 */
                               dsp_calibration_report *report,        /* on the HOST */
                               void *stream);
int dsp_calibration_apply_device(dsp_calibrator *c, const float *d_scores, long n_rows, long n_columns, const long *n_frames,
                                 const dsp_calibration *params, float *d_out, void *stream);

/* COHORT NORMALISATION: Z-, T- and S-norm of a score matrix, and their adaptive forms that keep the K closest cohort members
 * (INTEGRATION.md 6p).  The reference has no such step: it compares the raw target.score - ubm.score with one
 * threshold (DEFAULT_SPEAKER_THRESHOLD, 2fa/audio/audio_driver.py:10; the sweep of evaluate_gmm.py), though that score shifts with the
 * enrolled model and with the test clip.  Everything is float32, row-major, on GPU `device`, as
 * dsp_speaker_verify_ragged_device writes it: d_scores[T][S], clip t against enrolled speaker s; a row cohort [T][N], clip t against N
 * cohort speakers (the same call with the cohort speakers' means), which gives one statistic per row; a column cohort [M][S], M cohort
 * clips against the S enrolled speakers (the same call with the cohort clips as d_feats), which gives one statistic per column -- the
 * columns are read where they lie, the caller transposes nothing.  Keeping a speaker's own clips out of the cohort is the caller's job.
 *
 * Statistic of one cohort vector v[0 .. n) with top_k = K (0: the whole cohort).  Values are ordered by their keys: an unsigned that
 * grows with the float, -0 before +0.
 *   1. Only finite values take part; n_finite is their number.  n_finite == 0: mean = std = threshold = NaN, n_selected = n_above = 0.
 *   2. n_selected K' = (K == 0 || K > n_finite) ? n_finite : K.
 *   3. threshold = the finite value with the K'-th largest key; n_above = the finite values whose key is above the threshold's.
 *   4. e = K' - n_above >= 1 copies of the threshold belong to the selection (which of several equal values never matters).
 *   5. The sums are float64 over a tree that n alone fixes: leaf i is the term of v[i] where v[i] is finite and its key is above the
 *      threshold's, else +0.0; the indices are cut into chunks of 4096 from index 0; inside a chunk the sum is the adjacent pairwise
 *      tree (1, 2, 4 ... 2048 apart, absent leaves +0.0); the chunks are added in ascending order.  No float atomics.
 *        A = tree((double)v[i]);                        mean = (A + (double)e * (double)threshold) / (double)K'
 *        Q = tree(d * d), d = (double)v[i] - mean;      p = dt * dt, dt = (double)threshold - mean
 *        std = sqrt((Q + (double)e * p) / (double)K')   -- the population standard deviation, np.std
 *      Every product and sum is rounded on its own, as written, from left to right; none is fused.
 * A vector's record is the same bits whatever the other vectors of the call, its position, the axis it lay along (per row of a matrix =
 * per column of its transpose), the grid and the stream.
 *
 * dsp_score_normalize_device: float64, never fused.  sigma' = (std > std_floor) ? std : std_floor;
 *   z = ((double)x - mean_col[s]) / sigma'_col[s], t = ((double)x - mean_row[t]) / sigma'_row[t]; d_out[t][s] = (float) of z
 * (DSP_NORM_Z), t (DSP_NORM_T) or 0.5 * (z + t) (DSP_NORM_S), rounded once.  A NaN score, or a statistic with n_finite == 0, gives NaN.
 * d_out == d_scores is allowed.  The output is a score matrix like its input: dsp_calibration_*, dsp_trials_evaluate_device and
 * dsp_segments_device take it unchanged.
 * Both calls only enqueue on `stream` of GPU `device`; nothing waits on the host.  The kernels keep what they need in LDS: there is no
 * workspace and no state between calls, hence no handle to create or destroy.  As for the other stages, ONE stream at a time is all
 * that is promised to a caller.
 *
 * DSP_EINVAL, before a device is touched, the first of -- dsp_cohort_stats_device: device < 0; an unknown axis; top_k outside 0 .. 2^22;
 * n_rows or n_cols < 0; more than 2^30 vectors; (no vector: DSP_OK here, no launch;) a cohort length (the reduced axis: n_cols per
 * row, n_rows per column) outside 1 .. 2^22; d_cohort NULL; d_stats NULL.  dsp_score_normalize_device: device < 0; cfg NULL; an unknown
 * mode; std_floor negative or not finite; n_rows or n_cols < 0; more than 2^30 rows or columns; (no row or no column: DSP_OK here, no
 * launch;) d_scores NULL; d_out NULL; d_row_stats NULL under DSP_NORM_T or DSP_NORM_S; d_col_stats NULL under DSP_NORM_Z or
 * DSP_NORM_S.
 * Not covered: choosing the cohort (and keeping a speaker's own clips out of it); cohorts selected per trial from the other side's
 * scores (the adaptive forms here select inside each cohort vector); a median or trimmed statistic.                                 */
#define DSP_COHORT_PER_ROW 0
#define DSP_COHORT_PER_COLUMN 1
#define DSP_NORM_Z 0
#define DSP_NORM_T 1
#define DSP_NORM_S 2
typedef struct dsp_cohort_stat {                                                    /* 32 bytes */
    double mean, std;
    float threshold;
    int n_finite, n_selected, n_above;
} dsp_cohort_stat;
typedef struct dsp_snorm_config {
    int    mode;         /* DSP_NORM_Z, DSP_NORM_T or DSP_NORM_S */
    int    reserved;
    double std_floor;    /* finite, >= 0: the least sigma a score is divided by */
} dsp_snorm_config;
int dsp_cohort_stats_device(int device, const float *d_cohort, long n_rows, long n_cols,
                            int axis,              /* DSP_COHORT_PER_ROW: n_rows records over n_cols values; DSP_COHORT_PER_COLUMN: n_cols records over n_rows values */
                            int top_k, dsp_cohort_stat *d_stats, void *stream);
int dsp_score_normalize_device(int device, const float *d_scores, long n_rows, long n_cols,
                               const dsp_cohort_stat *d_row_stats,    /* [T], needed by DSP_NORM_T and DSP_NORM_S */
                               const dsp_cohort_stat *d_col_stats,    /* [S], needed by DSP_NORM_Z and DSP_NORM_S */
                               const dsp_snorm_config *cfg, float *d_out, void *stream);

/* VOICE ACTIVITY DETECTION: frame power, speech flags and row selection between the front end and the models (DESIGN.md 3.25,
 * INTEGRATION.md 6q).  The reference has no such step: extract_features_from_array (2fa/audio/speaker/gmm_utils.py:28-62) keeps every
 * row, so the room noise that opens and closes a recording goes into the UBM, every MAP mean and both terms of every LLR.  This is
 * Kaldi's compute-vad-energy + select-voiced-frames and librosa's effects.split / trim, restated; librosa is not pinned.
 *
 * Rows.  Clip c is samples [offsets[c], offsets[c + 1]) of d_signal (float32) and rows [frame_offsets[c], frame_offsets[c + 1]) of
 * every per-row array (d_power, d_flags, d_level_db, a matrix to select from), as dsp_mfcc_ragged_frame_offsets gives them for a plan
 * of the same frame_length, hop_length and framing: row t is samples [t hop - lead, t hop - lead + frame_length) of its clip, zeros
 * outside it, lead = 0 (DSP_FRAMING_COMPLETE), frame_length - hop (DSP_FRAMING_STREAM, hop <= frame_length) or frame_length / 2
 * (DSP_FRAMING_CENTER, frame_length even).  Positions outside the clip are never loaded.  A clip may bring fewer rows than
 * dsp_mfcc_frames_for gives its length (a max_frames cap), never more.  Both offset arrays are HOST arrays, read before a call returns.
 *
 * Frame power.  g = gcd(hop, frame_length, lead) (lead left out when 0), m = frame_length / g <= 64, frame_length <= 4096.  Sub-block b
 * of a clip is its samples [b g, b g + g), the last one zero-extended; its sum s[b] of squares is float64 (a float32's square is
 * exact there) over a tree g alone fixes: sample e of the sub-block belongs to quad e / 4 and partial (e / 4) mod W, W the least
 * power of two >= ceil(g / 4), at most 64; a partial adds its samples in ascending order; the partials are halved, p[l] += p[l + off]
 * for off = W / 2 ... 1.  Frame t adds s[b0] ... s[b0 + m - 1], b0 = (t hop - lead) / g, in ascending order, sub-blocks outside the
 * clip skipped, and P[t] = that sum / frame_length.  Against np.mean(frame ** 2) in float64: within 2 frame_length 2^-53 relative.
 *
 * Decision, per clip, over its rows with finite P:
 *   reference  DSP_VAD_REF_ABSOLUTE 1.0; DSP_VAD_REF_MAX the largest (threshold_ratio 1e-6 = librosa's top_db 60 with ref = np.max);
 *              DSP_VAD_REF_MEAN their mean: finite rows as they are and the others as +0.0 over tiles of 256 rows from row 0, each
 *              tile's 256 leaves halved (v[i] += v[i + off], off = 128 ... 1), the tiles added in ascending order, / the finite count.
 *              No finite row: 0.
 *   threshold  s = reference * threshold_ratio; threshold = (s >= floor_power) ? s : floor_power.  Both numbers are linear powers
 *              (dsp_vad_ratio_from_db(db) = pow(10, db / 10) on the host): no log or pow runs on the device before the decision.
 *   raw[t]     isfinite(P[t]) && P[t] > threshold.  Strict: an all-zero clip keeps nothing (librosa's power_to_db clamps at amin
 *              and would keep every row of such a clip).
 *   sm[t]      Kaldi's smoothing, c = context_frames 0 .. 64, p = proportion in (0, 1]: over rows [max(0, t - c), min(T - 1, t + c)]
 *              of the clip, (double)(raw flags set) >= (double)(rows in the window) * p.  c = 0: sm = raw.
 *   keep[t]    the hangover, pad_frames 0 .. 64: any sm[u] with |u - t| <= pad_frames inside the clip.
 * d_flags[row] = keep as 0 / 1.  d_level_db[row] (may be NULL) = (float)(10 log10(P / threshold)), whatever IEEE gives for 0 and
 * non-finite operands: a score track that dsp_segments_device takes as one column (hysteresis, gap merge, minimum length in dB).
 * d_clips[c] (may be NULL) = {reference, threshold, raw rows, kept rows, first and last kept row (-1: none)}.  kept_offsets[n_clips + 1]
 * is a HOST array, the prefix sums of the kept rows, because every consumer takes host offsets: dsp_vad_decide_ragged_device,
 * dsp_vad_run_ragged_device and dsp_rows_kept_offsets_device return when it is filled: each waits for the stream, ONCE.
 *
 * Selection.  dsp_rows_select_ragged_device copies the rows of d_in[..][d] (float32, d 1 .. 64) whose flag is not 0 to d_out, order
 * kept: output row kept_offsets[c] + (rank of t among clip c's kept rows) is input row frame_offsets[c] + t, which d_row_index (int64,
 * may be NULL) records.  The flags may come from anywhere; dsp_rows_kept_offsets_device counts them.  d_out holds kept_offsets[n_clips]
 * rows and must not overlap the rows of d_in it reads.  Only enqueues.
 *
 * No handle: the stage keeps nothing between calls, so there is nothing to create or destroy.  What a call needs on the device lies
 * in the caller's d_workspace of at least dsp_vad_workspace_bytes(n_clips, rows) bytes, rows = frame_offsets[n_clips] -
 * frame_offsets[0], 256-byte aligned (hipMalloc's alignment), whose contents before the call do not matter and which one stream
 * at a time may use.  dsp_vad_run_ragged_device keeps the power there.  Every output is the same bits whatever the batch around a
 * clip, its position, the grid, the stream and the workspace's contents.
 *
 * DSP_EINVAL, before a device is touched, the first of: cfg NULL; hop_length < 1; frame_length outside 1 .. 4096; an unknown
 * framing; an odd frame_length under DSP_FRAMING_CENTER; hop_length > frame_length under DSP_FRAMING_STREAM; more than 64 sub-blocks
 * per frame; an unknown reference; threshold_ratio or floor_power negative or NaN (or threshold_ratio infinite); context_frames or
 * pad_frames outside 0 .. 64; proportion outside (0, 1]; device < 0; n_clips < 0 or >= 2^31; (n_clips == 0: DSP_OK, kept_offsets[0]
 * = 0;) an offsets array NULL; sample offsets negative, decreasing or a clip of 2^31 samples or more; frame_offsets negative or
 * decreasing; a clip with more rows than dsp_mfcc_frames_for gives it (the message names the clip); a NULL buffer that is not
 * optional; a workspace NULL, misaligned or too small; d outside 1 .. 64; kept_offsets that do not start at 0, decrease or give a
 * clip more rows than it has; d_out overlapping d_in.  Clips without rows are legal everywhere.
 * dsp_vad_trim_spans (host only, librosa's trim): clip c with a kept row is cut to [first_kept hop, min(n, (last_kept + 1) hop)),
 * starts[c] in absolute positions (offsets[c] + ...) and lengths[c]; a clip that keeps nothing gets starts[c] = offsets[c], lengths[c]
 * = 0.  Returns the number of clips that keep something.
 * Not covered: PCM16 input; scanners and stream sessions; Kaldi's log-energy mean (it needs a device log before the decision);
 * spectral or model-based VAD; librosa's own numbers.                                                                              */
#define DSP_VAD_REF_ABSOLUTE 0
#define DSP_VAD_REF_MAX 1
#define DSP_VAD_REF_MEAN 2
typedef struct dsp_vad_config {
    int frame_length, hop_length, framing;      /* those of the MFCC plan whose rows are filtered */
    int reference;                              /* DSP_VAD_REF_* */
    double threshold_ratio, floor_power;        /* linear powers */
    int context_frames;
    double proportion;
    int pad_frames;
} dsp_vad_config;
typedef struct dsp_vad_clip {                                                       /* 32 bytes */
    double reference, threshold;
    int n_raw, n_kept, first_kept, last_kept;
} dsp_vad_clip;
typedef struct dsp_vad_geometry {
    int g, m;                /* samples per sub-block, sub-blocks per frame */
    int samples_per_tile;    /* the samples a tile's frames span */
    int rows_per_tile;       /* rows a block takes at a time: results must not depend on where a clip's rows fall in them */
    int halo_rows;           /* context_frames + pad_frames: rows on either side of a tile whose raw flags are computed again */
} dsp_vad_geometry;
/* framing from the plan's config; DSP_VAD_REF_MAX, ratio 1e-6, floor 0, context 0, proportion 0.6 (Kaldi's), pad 0 */
void dsp_vad_default_config(const dsp_mfcc_config *mfcc, dsp_vad_config *cfg);
double dsp_vad_ratio_from_db(double db);
int dsp_vad_geometry_for(const dsp_vad_config *cfg, dsp_vad_geometry *out);        /* host only */
long dsp_vad_workspace_bytes(long n_clips, long n_rows);                            /* host only; enough for every entry below */
int dsp_vad_frame_power_ragged_device(int device, const dsp_vad_config *cfg, const float *d_signal, long n_clips, const long *offsets,
                                      const long *frame_offsets, double *d_power, void *d_workspace, long workspace_bytes, void *stream);
int dsp_vad_decide_ragged_device(int device, const dsp_vad_config *cfg, const double *d_power, long n_clips, const long *frame_offsets,
                                 uint8_t *d_flags, float *d_level_db, dsp_vad_clip *d_clips, long *kept_offsets, void *d_workspace,
                                 long workspace_bytes, void *stream);
int dsp_vad_run_ragged_device(int device, const dsp_vad_config *cfg, const float *d_signal, long n_clips, const long *offsets,
                              const long *frame_offsets, uint8_t *d_flags, float *d_level_db, dsp_vad_clip *d_clips, long *kept_offsets,
                              void *d_workspace, long workspace_bytes, void *stream);
int dsp_rows_kept_offsets_device(int device, const uint8_t *d_flags, long n_clips, const long *frame_offsets, long *kept_offsets,
                                 void *d_workspace, long workspace_bytes, void *stream);
int dsp_rows_select_ragged_device(int device, const float *d_in, int d, const uint8_t *d_flags, long n_clips, const long *frame_offsets,
                                  const long *kept_offsets, float *d_out, long *d_row_index, void *d_workspace, long workspace_bytes,
                                  void *stream);
long dsp_vad_trim_spans(const dsp_vad_config *cfg, const long *offsets, long n_clips, const dsp_vad_clip *clips, long *starts, long *lengths);

/* SVM TRAINING: the scrub-jay RBF-SVM from pooled features -- cepstrum/train.py:66-85 (StandardScaler, SVC(kernel="rbf",
 * probability=True, class_weight="balanced"), cross-validation) as batched SMO on the GPU.
 * d_feat[n][n_features] is float32 on the trainer's device (what dsp_mfcc_stats_device writes); labels[n] is a HOST array of 0 / 1,
 * read before a call returns.  Label 0 is libsvm's positive side, y = +1, as dsp_svm_predict_device votes (label 0 where dec > 0).
 *
 * Dataset.  dsp_svm_train_set_device fits the Scaler -- offset = mean, scale = 1 / population std (std 0: scale 1) per feature over
 * scaler_rows[n_scaler_rows] (HOST, NULL: all n rows), float64 sums, written as float32 -- or takes the caller's offset and scale (both
 * given: nothing is fitted), standardises z = fl32(fl32(x - offset) * scale) and builds D2[n][n] = sum_f ((double)z_if - (double)z_jf)^2
 * in float64, features ascending, symmetric bit for bit.  The trainer keeps z and D2 until the next dataset: every problem on this
 * Scaler shares them, across all gammas.  offset_out / scale_out (HOST [n_features], may be NULL) receive the Scaler; with either given
 * the call waits for the stream.  n is 2 .. 8192 (DSP_SVM_TRAIN_MAX_ROWS: D2 takes 8 n^2 bytes, 512 MB at the cap).
 *
 * Problems.  A problem is rows[n_rows] of the dataset (HOST, strictly ascending), a box bound per label and gamma; with K_ij =
 * exp(-gamma D2_ij) it is libsvm's C-SVC dual: min 1/2 a'Qa - e'a, Q_ij = y_i y_j K_ij, 0 <= a_i <= C(label_i), y'a = 0.
 * dsp_svm_train_problems_device solves n_problems of them in ONE launch, one workgroup each, by libsvm's Solver without shrinking:
 *   i = the member maximising -y G over I_up = {y = +1, a < C} u {y = -1, a > 0};
 *   j = the member of I_low = {y = +1, a > 0} u {y = -1, a < C} with -y_j G_j < -y_i G_i minimising -(b^2) / max(K_ii + K_jj - 2 K_ij,
 *       1e-12 where that is <= 0), b = -y_i G_i + y_j G_j;
 *   of equal candidates the one earliest in rows[] wins, in both selections (libsvm keeps the latest);
 *   the analytic two-variable step with libsvm's box clipping; G += Q_i da_i + Q_j da_j;
 *   stop when max over I_up of -y G plus max over I_low of y G is < eps (no j: stop), or after max_iter steps.
 * Q is float64 throughout; libsvm rounds the rows of Q it caches to float32 (svm.cpp Qfloat), and cfg->q_float32 = 1 does the same to
 * every kernel value the solver reads -- the selection, the step and the gradient -- which reproduces libsvm's decision values to
 * its own convergence instead of to its rounding (1e-8 against 1e-7 .. 3e-6 of a decision).  The decision pass is float64 either way,
 * as libsvm's prediction is.  results[p] on the HOST: rho = -(libsvm's rho: the mean of
 * y G over the free alphas, without any the midpoint of the bounds), so that dec = sum_i coef_i K_i + rho as dsp_svm_create takes it;
 * n_iter; n_sv = alphas > 0; n_bounded = alphas at C; objective = 1/2 a'Qa - e'a; gap = the violation at the end; status.
 * d_coef[P][n] (device, float64) = a_i y_i on the problem's rows and 0 elsewhere; d_dec[P][n] (device, float64, may be NULL) = the
 * decision of EVERY row of the dataset under problem p: its own rows' are the training decisions, the others' the held-out ones, which
 * is the cross-validation prediction.  Degenerate problems are reported, never a fault: rows of one label only is
 * DSP_SVM_TRAIN_ONE_CLASS -- nothing is solved, coef is 0 and every decision +1 (label 0) or -1 (label 1), as libsvm's
 * svm_binary_svc_probability sets them; n_rows == 0 is DSP_SVM_TRAIN_EMPTY, every decision 0; running out of steps is
 * DSP_SVM_TRAIN_MAX_ITER, with the alphas, rho and gap of the last step.  A problem's coef, dec and result are the same bits whatever
 * other problems share the launch and in whatever order.  The call enqueues everything, waits for the stream ONCE and returns with
 * results filled.  cfg NULL: eps 1e-3 (libsvm's), max_iter 1 000 000; max_iter 0 in a cfg means that default too.
 *
 * Platt.  dsp_svm_platt_fit_device is libsvm's sigmoid_train on the pairs (d_dec_cv[r], labels[r]) for r in rows[n_rows] (HOST, NULL:
 * all rows of the dataset): prior-smoothed targets, A = 0, B = log((prior0 + 1) / (prior1 + 1)) to start, Newton with backtracking,
 * 100 iterations, min_step 1e-10, sigma 1e-12, eps 1e-5; prior1 counts label 0, the positive side.  One block, float64 sums in a fixed
 * order: the same bits on every run.  P(label 0 | dec) = 1 / (1 + exp(A dec + B)): prob_a, prob_b of dsp_svm_create.  A, B and
 * n_iter are HOST values: the call waits for the stream.
 *
 * Host helpers (no device).  dsp_svm_folds: fold_ids[n] in 0 .. k - 1 by libsvm's rule -- perm = 0 .. n - 1, for i ascending swap
 * perm[i] with perm[i + draw_i % (n - i)], fold f takes perm[f n / k .. (f + 1) n / k) -- on the library's own draws, draw_i =
 * mix(seed + (i + 1) 0x9E3779B97F4A7C15) with splitmix64's finaliser as for dsp_kmeans_*.  dsp_svm_balanced_weights: sklearn's
 * class_weight = "balanced", C_k = C n_rows / (2 n_k) over rows[n_rows] (NULL: labels[0 .. n_rows)); DSP_EINVAL when a label has no
 * row.  dsp_svm_model_from_training: the support vectors -- rows with coef != 0 -- of z[n][n_features], label 0's first and each
 * label's in row order (libsvm's order), as sv[][n_features] and (float)coef; returns their number (sv and coef_out may be NULL to
 * count), n_sv_label0 (may be NULL) how many carry label 0; more than `capacity`: DSP_EINVAL.
 *
 * dsp_svm_fit_device is the reference's clf.fit: the Scaler on all rows, k_prob problems without fold f = 0 .. k_prob - 1 and the
 * final one on all rows in ONE problems launch, the Platt fit on dec_cv[i] = dec[fold_ids[i]][i], the compacted model.  fold_ids
 * (HOST [n], NULL: dsp_svm_folds(n, k_prob, seed)); the model's arrays are the caller's: offset, scale [n_features], sv [n][n_features]
 * and coef [n] at most.  rho, prob_a, prob_b and gamma are rounded to float as dsp_svm_create takes them.  The call waits for the
 * stream more than once (after the Scaler, after the problems, after the Platt fit): the model is the HOST's when it returns.
 *
 * One stream at a time per trainer; the workspace (z, D2, the launch's problem table) is grow-only.  dsp_svm_trainer_create touches
 * no device.  DSP_EINVAL, before a device is touched and naming the argument: a NULL that may not be; n_features < 1; n < 2 or above
 * the cap; a scaler row or problem row outside 0 .. n - 1, problem rows not strictly ascending; a label other than 0 / 1; C_label0,
 * C_label1 not finite or not > 0; gamma not finite or < 0; eps not finite or not > 0; max_iter outside 0 .. 100 000 000; q_float32 other than 0 / 1; only one of
 * offset / scale; a problems or Platt call before a dataset; k_prob outside 2 .. 64 or above n; a fold id outside 0 .. k_prob - 1.
 * Not covered: shrinking and a kernel cache (every step reads two rows of D2), kernels other than RBF, more than two classes.        */
#define DSP_SVM_TRAIN_MAX_ROWS 8192
#define DSP_SVM_TRAIN_CONVERGED 0
#define DSP_SVM_TRAIN_MAX_ITER 1
#define DSP_SVM_TRAIN_ONE_CLASS 2
#define DSP_SVM_TRAIN_EMPTY 3
typedef struct dsp_svm_train_problem {
    const int *rows;     /* [n_rows] on the HOST, strictly ascending */
    long   n_rows;
    double c_label0, c_label1, gamma;
} dsp_svm_train_problem;
typedef struct dsp_svm_train_config {
    double eps;          /* > 0: the violation below which a problem has converged; 1e-3 = libsvm's */
    int    max_iter;     /* 0: 1 000 000 */
    int    q_float32;    /* 0: Q in float64; 1: the solver's kernel values rounded to float32, as libsvm caches Q */
} dsp_svm_train_config;
typedef struct dsp_svm_train_result {                                               /* 40 bytes */
    double rho, objective, gap;
    int n_iter, n_sv, n_bounded, status;
} dsp_svm_train_result;
typedef struct dsp_svm_fit_model {
    float *offset, *scale;                 /* [n_features]           the caller's */
    float *sv, *coef;                      /* [n][n_features], [n]   the caller's; the first n_sv are written */
    long   n_sv, n_sv_label0;
    float  rho, prob_a, prob_b, gamma;
    int    platt_iter, reserved;
    dsp_svm_train_result final;            /* the problem on all rows */
} dsp_svm_fit_model;
typedef struct dsp_svm_trainer dsp_svm_trainer;
int dsp_svm_trainer_create(int device, int n_features, dsp_svm_trainer **out);
void dsp_svm_trainer_destroy(dsp_svm_trainer *t);
int dsp_svm_train_set_device(dsp_svm_trainer *t, const float *d_feat, long n, const int *scaler_rows, long n_scaler_rows,
                             const float *offset, const float *scale,   /* HOST [n_features], both or neither: the caller's Scaler */
                             float *offset_out, float *scale_out,       /* HOST [n_features], may be NULL */
                             void *stream);
int dsp_svm_train_problems_device(dsp_svm_trainer *t, const dsp_svm_train_problem *problems, long n_problems, const dsp_svm_train_config *cfg,
                                  const int *labels,                    /* HOST [n] */
                                  dsp_svm_train_result *results,        /* HOST [n_problems] */
                                  double *d_coef,                       /* [n_problems][n] */
                                  double *d_dec,                        /* [n_problems][n], may be NULL */
                                  void *stream);
int dsp_svm_platt_fit_device(dsp_svm_trainer *t, const double *d_dec_cv, const int *labels, const int *rows, long n_rows, double *a, double *b,
                             int *n_iter, void *stream);
int dsp_svm_folds(long n, int k, unsigned long long seed, int *fold_ids);
int dsp_svm_balanced_weights(const int *labels, const int *rows, long n_rows, double c, double *c_label0, double *c_label1);
long dsp_svm_model_from_training(const float *z, const int *labels, const double *coef, long n, int n_features, float *sv, float *coef_out,
                                 long capacity, long *n_sv_label0);
int dsp_svm_fit_device(dsp_svm_trainer *t, const float *d_feat, long n, const int *labels, const int *fold_ids, int k_prob,
                       unsigned long long seed, double c_label0, double c_label1, double gamma, const dsp_svm_train_config *cfg,
                       dsp_svm_fit_model *model, void *stream);
/* the trainer's standardised rows z[n][n_features] of the current dataset, copied to the HOST (waits for the stream) */
int dsp_svm_train_rows_host(dsp_svm_trainer *t, float *z, void *stream);

/* STOP-NET TRAINING: the net behind classify_signal from labelled MFCC matrices -- 2fa/audio/word/python/keyword_classifier.py:155-232
 * (StandardScaler, Dense 4-2-2-1 with dropout, Adam, binary cross-entropy, EarlyStopping(patience=10, restore_best_weights=True)) as
 * MANY Keras-style fits per launch over one standardised feature matrix: seeds, folds, dropout
 * and learning rates side by side, the best kept by validation loss.  The helpers below are the definition of every draw.
 *
 * Dataset.  dsp_stop_train_set_device takes a ragged matrix d_mfcc[..][n_coef] (float32, the trainer's device) with HOST
 * frame_offsets[n + 1] as dsp_stop_scan_device does; clip i is rows [frame_offsets[i], frame_offsets[i + 1]), T_i of them.  Feature
 * j = c max_frames + t of clip i is mfcc[off_i + t][c] for t < min(T_i, max_frames) and 0 otherwise (stop_detector.c:36-50).  The
 * Scaler is, per feature over scaler_rows[n_scaler_rows] (HOST, NULL: all n rows), mean and scale = population std (std 0: 1, as
 * sklearn's StandardScaler.scale_): float64 sums with a centred second pass, a lane's rows ascending (lane l of 256 takes rows l, l +
 * 256, ...), the 256 partials by a 6-level xor butterfly per wavefront and the four wavefronts as (0 + 1) + (2 + 3); written as float32
 * in the layout dsp_stop_model_params reads.  The caller may give mean and scale (HOST [n_coef max_frames], both or neither) instead.
 * The trainer keeps Z[n][F_used] = fl32(fl32(x - mean) / (scale == 0 ? 1 : scale)), the inference kernels' expression, with
 * T_used = min(max_frames, max_i T_i), F_used = n_coef T_used and used feature c T_used + t = feature c max_frames + t.  Features past
 * it are 0 for every clip: their gradients are exactly 0, under Adam their weights stay at the initial draw, the kernels skip them and
 * the returned layer-1 kernel carries their initial values.  mean_out / scale_out (HOST [n_coef max_frames], may be NULL) receive the
 * Scaler; with either given the call waits for the stream.  dsp_stop_train_used_features returns F_used (0: no dataset),
 * dsp_stop_train_rows_host copies Z to the HOST.
 *
 * Runs.  dsp_stop_train_runs_device trains n_runs of them together, one workgroup each, one launch per epoch.  A run follows Keras's
 * fit.  Init: kernels Glorot-uniform, w = (2 u - 1) sqrt(6 / (fan_in + fan_out)), fan_in of layer 1 the full n_coef max_frames; biases
 * 0.  Each epoch: the training rows in the order train_rows[order[k]] of the epoch's keyed permutation, ceil(n_train / batch) steps, the
 * last batch the short remainder averaged over its own size.  Forward: ReLU hidden layers with inverted dropout (kept when u >= rate,
 * kept values times 1 / (1 - rate); rate 0: no draw), a sigmoid output.  Loss: binary cross-entropy from the logit a, max(a, 0) - a y +
 * log1p(exp(-|a|)); its gradient (p - y) / B; the ReLU derivative is 1 only where the pre-activation is > 0.  Adam in Keras's form, t =
 * 1, 2, ..., beta1 0.9, beta2 0.999, eps 1e-7: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), m = beta1 m + (1 - beta1) g, v = beta2 v +
 * (1 - beta2) g^2, w -= lr_t m / (sqrt(v) + eps).  After each epoch val_loss is the mean loss over val_rows without dropout; val_loss <
 * best (strict; NaN never improves) snapshots the weights, sets best_epoch and wait = 0, otherwise ++wait and wait >= patience stops
 * the run.  Returned are the best snapshot when restore_best is set and there is one (Keras 3's on_train_end), else the last weights;
 * without validation rows there is no early stop and the last weights are returned.  Weights, moments, activations, losses and every
 * sum are float64, Z is widened as it is read; no float atomics, nothing passes between runs, and every sum over features, a batch or
 * the validation rows has an order fixed by the shapes alone: a run's outputs are the same bits alone, among hundreds of others,
 * reordered, and after the workspace has grown.
 *
 * results[p] on the HOST: n_epochs run; best_epoch (0-based, -1: none) and best_val_loss (NaN: none); last_loss, the last epoch's
 * training loss; status; val_correct, the validation rows on the right side of P > 0.5 at the returned weights; n_dead_units, the
 * hidden units whose activation is 0 on every training row at the returned weights (the all-ReLUs-dead plateau, as a number).
 * d_history[P][max_p epochs_p][2] (device, float64): the training loss as Keras reports it (the sample-weighted mean of the batch
 * losses, dropout on) and val_loss; epochs not run hold NaN.  d_prob[P][n] (device, float64, may be NULL): P(stop) of EVERY row of the
 * dataset under run p's returned weights, dropout off; rows outside train_rows are held-out predictions.  d_params[P][n_params]
 * (device, float64): the returned weights flat, kernel1, bias1, ..., kernel4, bias4, kernels (in, out) row-major.  n_train == 0 is
 * DSP_STOP_TRAIN_EMPTY: nothing is trained, the initial weights are returned with n_epochs 0; n_val == 0 is DSP_STOP_TRAIN_NO_VALIDATION.
 * The call enqueues the epochs without a host round trip, looks at the runs' stop flags every 8 epochs and returns with results filled:
 * it waits for the stream.
 *
 * Random numbers, the library's own (Keras's cannot be reproduced): mix = splitmix64's finaliser as for dsp_kmeans_*, G =
 * 0x9E3779B97F4A7C15, draw(seed, stream, counter) = mix(mix(seed + (stream + 1) G) + (counter + 1) G), u = (draw >> 11) 2^-53.  Stream
 * 0: initial weights, counter = flat parameter index.  Stream 1: the epoch order, a 4-round Feistel network on the smallest even number
 * of bits (at least 2) covering n_train, (L, R) <- (R, L ^ (mix(key_epoch + (r + 1) G + R) & mask)) for r = 0 .. 3, cycle-walked until
 * the value is < n_train, key_epoch = draw(seed, 1, epoch).  Stream 2: dropout, counter = ((global_step 3 + layer) 256 + slot) 16 +
 * unit with global_step counting the run's optimiser steps from 0, layer 0 .. 2 and slot the sample's place in its batch.
 *
 * Host helpers (no device).  dsp_stop_train_param_count; dsp_stop_train_uniform; dsp_stop_train_order (order[n] of an epoch);
 * dsp_stop_train_init (params[n_params], the initial weights); dsp_stop_model_from_training: float64 parameters plus the Scaler as the
 * float32 arrays of dsp_stop_model_params in the caller's `arrays` (2 n_coef max_frames + n_params floats), `model` pointing into them.
 *
 * One stream at a time per trainer; the workspace (Z, the runs' slabs and tables) is grow-only.  dsp_stop_trainer_create touches no
 * device.  DSP_EINVAL, before a device is touched and naming the argument: a NULL that may not be; n_coef, max_frames < 1, a unit
 * count outside 1 .. 16 or units[3] != 1; n outside 1 .. 65536; frame_offsets negative or decreasing; a scaler, training or validation
 * row outside 0 .. n - 1, run rows not strictly ascending; a label other than 0 / 1; only one of mean / scale, or a value not finite;
 * a runs call before a dataset; n_runs above 4096; batch_size outside 1 .. 256, epochs outside 1 .. 10000, patience < 0, a dropout
 * rate outside [0, 1), a learning rate not finite or not > 0, restore_best other than 0 / 1.
 * Not covered: an LDS-resident variant for short clips, float32 training arithmetic, other optimisers, class weights.                */
#define DSP_STOP_TRAIN_CAP_ROWS 65536
#define DSP_STOP_TRAIN_CAP_UNITS 16
#define DSP_STOP_TRAIN_CAP_BATCH 256
#define DSP_STOP_TRAIN_CAP_EPOCHS 10000
#define DSP_STOP_TRAIN_CAP_RUNS 4096
#define DSP_STOP_TRAIN_CONVERGED_EARLY 0
#define DSP_STOP_TRAIN_MAX_EPOCHS 1
#define DSP_STOP_TRAIN_NO_VALIDATION 2
#define DSP_STOP_TRAIN_EMPTY 3
typedef struct dsp_stop_train_run {                                                 /* 88 bytes */
    const int *train_rows, *val_rows;    /* HOST, strictly ascending; val_rows may be NULL with n_val 0 */
    long   n_train, n_val;
    unsigned long long seed;
    double learning_rate;                /* 1e-3 */
    double dropout[3];                   /* 0.3, 0.3, 0.2 */
    int    batch_size;                   /* 32 */
    int    epochs;                       /* 50 */
    int    patience;                     /* 10 */
    int    restore_best;                 /* 1 */
} dsp_stop_train_run;
typedef struct dsp_stop_train_result {                                              /* 40 bytes */
    double best_val_loss, last_loss;
    int n_epochs, best_epoch, status, val_correct, n_dead_units, reserved;
} dsp_stop_train_result;
typedef struct dsp_stop_trainer dsp_stop_trainer;
int dsp_stop_trainer_create(int device, int n_coef, int max_frames, const int *units /* [4] */, dsp_stop_trainer **out);
void dsp_stop_trainer_destroy(dsp_stop_trainer *t);
int dsp_stop_train_set_device(dsp_stop_trainer *t, const float *d_mfcc, long n, const long *frame_offsets /* HOST [n + 1] */,
                              const int *scaler_rows, long n_scaler_rows,
                              const float *mean, const float *scale,         /* HOST [n_coef max_frames], both or neither */
                              float *mean_out, float *scale_out,             /* HOST [n_coef max_frames], may be NULL */
                              void *stream);
long dsp_stop_train_used_features(const dsp_stop_trainer *t);
int dsp_stop_train_rows_host(dsp_stop_trainer *t, float *z /* HOST [n][F_used] */, void *stream);
int dsp_stop_train_runs_device(dsp_stop_trainer *t, const dsp_stop_train_run *runs, long n_runs,
                               const int *labels,                            /* HOST [n], 0 / 1 */
                               dsp_stop_train_result *results,               /* HOST [n_runs] */
                               double *d_history,                            /* [n_runs][max epochs][2] */
                               double *d_prob,                               /* [n_runs][n], may be NULL */
                               double *d_params,                             /* [n_runs][n_params] */
                               void *stream);
long dsp_stop_train_param_count(int n_coef, int max_frames, const int *units);
double dsp_stop_train_uniform(unsigned long long seed, unsigned long long stream, unsigned long long counter);
int dsp_stop_train_order(long n, unsigned long long seed, long epoch, int *order);
int dsp_stop_train_init(int n_coef, int max_frames, const int *units, unsigned long long seed, double *params);
int dsp_stop_model_from_training(int n_coef, int max_frames, const int *units, const double *params, const float *mean, const float *scale,
                                 float *arrays, dsp_stop_model_params *model);

/* --- augmenting raw training clips: time stretch, pitch shift, additive noise; complex STFT and inverse STFT ---
 * cepstrum/train.py:25-36, 52-56 enlarges the minority class with augment(): librosa.effects.time_stretch, librosa.effects.pitch_shift
 * or y + 0.005 * randn, on raw audio, before the features are taken.  These entries do that to a ragged batch of float32 clips in HBM.
 * librosa is an unpinned dependency of the reference: the algorithm is restated here from its published form (stft / phase_vocoder /
 * istft of librosa < 0.10, whose stft pads with "reflect"), and PARITY WITH LIBROSA'S OWN NUMBERS IS UNPINNED.  Two stated differences:
 * pitch_shift resamples with this library's polyphase Kaiser-windowed sinc (dsp_resample_*, scipy.signal.resample_poly's filter) where
 * librosa uses resampy's "kaiser_best" (a longer windowed sinc interpolated at the irrational ratio itself), and at a rational
 * approximation of 2^(-n_steps / 12) (below); and the noise comes from the library's counter-based draws, not numpy's stream.
 *
 * CONSTANTS.  n_fft 2048, hop 512, window 0.5 - 0.5 cos(2 pi i / 2048) (periodic Hann), 1025 bins; float32 samples.
 * STFT (center = True).  A clip of n samples has T = 1 + n / 512 frames; frame t covers samples [512 t, 512 t + 2048) of the clip padded
 * by 1024 on both sides; D[t][k], k = 0 .. 1024, is the forward DFT of window x frame as interleaved float32 (re, im), frame-major.
 * DSP_PAD_REFLECT pads as np.pad(mode = "reflect") and needs n >= 1025; DSP_PAD_ZERO pads with zeros and takes any n >= 1.
 * PHASE VOCODER.  T_out = ceil(T / rate) in double; output frame t reads columns i = floor(t * rate) and i + 1 (a = t * rate - i; columns
 * T and T + 1 read as zero); with phi_k = pi * 512 * k / 1024:
 *     acc_0[k] = angle(D[0][k]);   S[t][k] = ((1 - a) |D[i][k]| + a |D[i+1][k]|) exp(j acc_t[k]);
 *     d = angle(D[i+1][k]) - angle(D[i][k]) - phi_k;  d -= 2 pi rint(d / 2 pi);   acc_{t+1} = acc_t + phi_k + d
 * acc is float64, summed in frame order; sin / cos take acc - 2 pi rint(acc / 2 pi) rounded to float32; angle(0) = 0 (silence in,
 * exact zeros out).
 * INVERSE STFT.  Frame t -> irfft (1 / 2048 included, Im of bins 0 and 1024 ignored) x window, overlap-added at 512 t with the frames
 * summed in ascending t, divided by the sum (same order) of the squared window where that exceeds FLT_MIN; the first 1024 samples
 * dropped; cropped or zero filled to `length`.
 * time_stretch(y, rate) = STFT -> vocoder -> inverse STFT with length = max(1, rint(n / rate)) (double division, ties to even).
 * pitch_shift(y, n_steps): (up, down) = dsp_pitch_ratio(n_steps, 12, max_term): the fraction with max(up, down) <= max_term (the
 * augmenter's, default 256, at most 1024) nearest to 2^(-n_steps / 12) by |up / down - 2^(-n_steps / 12)| in double, ties to the
 * smaller denominator (+-1 step: 185/196, 196/185; +-2: 49/55, 55/49 -- 0.006 and 0.02 cents off).  Stretch by rate = (double)up / down,
 * resample with dsp_resampler_create(device, rate_in = down, rate_out = up) (a copy when up == down), crop or zero fill to n.
 * add_noise: y[i] + sigma z_i with d = the 64-bit draw of dsp_stop_train_uniform's generator at (seed, stream = key, counter = j),
 * u1 = ((d >> 40) + 1) 2^-24, u2 = ((d >> 16) & 0xFFFFFF) 2^-24, r = sqrt(-2 ln u1): z_{2j} = r cos(2 pi u2), z_{2j+1} = r sin(2 pi u2),
 * evaluated in float32 on the GPU; dsp_augment_normal returns z_i in float64.  A stretch or pitch op with sigma > 0 gets the same noise
 * added to its result.
 *
 * HOST ONLY, no GPU: dsp_stft_frames (T), dsp_stretch_frames (T_out), dsp_stretch_length, dsp_pitch_ratio, dsp_augment_normal;
 * dsp_augment_out_offsets: out_offsets[m + 1] = prefix sums of the ops' output lengths (stretch: dsp_stretch_length of its clip; pitch
 * and noise: the clip's length), returns the total; dsp_augment_draw: train.py's policy with the library's draws -- row r with
 * labels[r] == 1 gets an op when u(S + 0, r) < prob; its kind is floor(3 u(S + 1, r)); a stretch has rate = 0.8 + 0.4 u(S + 2, r), a
 * pitch shift n_steps = floor(5 u(S + 3, r)) - 2, noise sigma = 0.005; clip = key = r; u(stream, counter) = dsp_stop_train_uniform(seed,
 * stream, counter) and S = 0xA000000000000000 keeps the policy's streams away from the noise keys.  Returns the op count (ops may be
 * NULL to count; more ops than `cap`: DSP_EINVAL).  All return < 0 on error.
 *
 * A dsp_augmenter holds the tables, grow-only workspaces and one resampler per pitch ratio on one GPU; one call at a time per handle.
 * Offsets are host arrays read before the call returns; the work is enqueued on `stream` and not waited for.
 * dsp_stft_ragged_device: clip c = samples [offsets[c], offsets[c + 1]) of d_in -> d_spec [sum T][1025] (re, im), clip c's rows from
 * frame_offsets_out[c] (n + 1 entries, may be NULL).  dsp_istft_ragged_device: rows [frame_offsets[c], frame_offsets[c + 1]) of d_spec
 * -> lengths[c] samples at d_out + out_offsets[c].  dsp_time_stretch_ragged_device: rates[n] doubles on the host; exactly the STFT
 * entry, the vocoder and the inverse STFT entry on the handle's workspaces; clip c's output at the prefix sums of dsp_stretch_length.
 * dsp_augment_ragged_device: op j reads clip ops[j].clip and writes at out_offsets[j] of dsp_augment_out_offsets (a clip may appear in
 * several ops).  A clip's output is the same bits whatever else is in the batch and in whatever order.
 * DSP_EINVAL with a reason: rate not finite or outside [1/8, 8]; |n_steps| > 12; sigma < 0 (or NaN); an unknown kind; a clip index out of
 * range; a clip to transform with n < 1, or n < 1025 under DSP_PAD_REFLECT; a clip of 2^24 samples or more.  n == 0 (m == 0): DSP_OK,
 * nothing is touched.                                                                                                              */
enum { DSP_PAD_REFLECT = 0, DSP_PAD_ZERO = 1 };
enum { DSP_AUGMENT_STRETCH = 0, DSP_AUGMENT_PITCH = 1, DSP_AUGMENT_NOISE = 2 };
typedef struct dsp_augment_op {
    long clip;                    /* the clip the op reads */
    int kind;                     /* DSP_AUGMENT_* */
    double rate;                  /* STRETCH */
    int n_steps;                  /* PITCH, semitones */
    float sigma;                  /* NOISE (any kind: added to the result when > 0) */
    unsigned long long key;       /* the stream of the noise draws */
} dsp_augment_op;
typedef struct dsp_augmenter dsp_augmenter;
long dsp_stft_frames(long n);
long dsp_stretch_frames(long n_frames, double rate);
long dsp_stretch_length(long n, double rate);
int dsp_pitch_ratio(int n_steps, int bins_per_octave, int max_term, int *up, int *down);
double dsp_augment_normal(unsigned long long seed, unsigned long long key, unsigned long long i);
long dsp_augment_out_offsets(const long *offsets, long n, const dsp_augment_op *ops, long m, long *out_offsets);
long dsp_augment_draw(unsigned long long seed, const int *labels, long n, double prob, dsp_augment_op *ops, long cap);
int dsp_augmenter_create(int device, int pad_mode, int max_term, dsp_augmenter **out);
void dsp_augmenter_destroy(dsp_augmenter *aug);
int dsp_stft_ragged_device(dsp_augmenter *aug, const float *d_in, long n, const long *offsets, float *d_spec, long *frame_offsets_out, void *stream);
int dsp_istft_ragged_device(dsp_augmenter *aug, const float *d_spec, long n, const long *frame_offsets, const long *lengths, float *d_out,
                            const long *out_offsets, void *stream);
int dsp_time_stretch_ragged_device(dsp_augmenter *aug, const float *d_in, long n, const long *offsets, const double *rates, float *d_out, void *stream);
int dsp_augment_ragged_device(dsp_augmenter *aug, const float *d_in, long n, const long *offsets, const dsp_augment_op *ops, long m,
                              unsigned long long seed, float *d_out, void *stream);

/* Reference-layout constant tables for a configuration (what mfcc_params.h holds
 * for the reference config): window[frame_length], mel[n_mels][n_fft/2+1],
 * dct[n_mfcc][n_mels].  Host-only, no GPU needed; any pointer may be NULL.      */
int dsp_mfcc_tables(const dsp_mfcc_config *cfg, float *window, float *mel, float *dct);

/* Per-lane kernel layout of the same tables (struct dsp::LaneTables512 of
 * dsp_amd/csrc/tables.hpp, `size` must equal its sizeof; returns that size when
 * out is NULL).  Host-only introspection used by the CPU tests of the planner. */
int dsp_mfcc_lane_tables(const dsp_mfcc_config *cfg, void *out, int size);
/* the same for a 400-point configuration: dsp::Tables400 (csrc/tables.hpp), the tables mfcc400_kernel.hip reads; tools/emulate_400_fft.py */
int dsp_mfcc400_tables(const dsp_mfcc_config *cfg, void *out, int size);
/* and for 1024- and 2048-point configurations: dsp::GenTables1024 (both 1024-point kernels read it) and dsp::GenTables2048 */
int dsp_mfcc1024_tables(const dsp_mfcc_config *cfg, void *out, int size);
int dsp_mfcc2048_tables(const dsp_mfcc_config *cfg, void *out, int size);

/* classify()'s spectrogram divides every PSD cell by U = fs * sum(window^2) (classifier.cpp:350-365).  The recompute kernel takes a
 * three-instruction form of that division for cells in [2^-60, 2^60] -- but only after the classifier context has compared it with
 * the real division on EVERY float of that range, on the device, for its U.  This call repeats the comparison: *mismatches = the
 * floats on which the two differ (0 expected); returns 1 when the fast form is in use, 0 when not (a mismatch, or
 * DSP_AMD_SPEC_EXACT_DIV set), < 0 on error.                                                                              */
int dsp_classify_division_check(long long *mismatches);

/* The host planner's self-check of BASELINE config 3's fused prefilter (dsp_mfcc_config.prefilter, tables.hpp PrefilterScan): the
 * literal band-pass as a cascade of four second-order sections run as lane scans.  Returns bit 0 = the cascade reproduces the
 * direct-form recurrence (donut-classifier/classifier.c:420-446) on 1024 samples, bit 1 = so does the row form of its scan (the
 * one the kernel runs); steps4 (may be NULL) receives the Kogge-Stone steps each section needs.  < 0: DSP_EINVAL.  Host only. */
int dsp_prefilter_scan_check(int prefilter, int *steps4);

/* --- misc -------------------------------------------------------------------- */
const char *dsp_last_error(void);   /* thread-local, "" when none */
int dsp_device_count(void);
const char *dsp_version(void);
/* ABI check for bindings that mirror the structs (ctypes, cgo, JNI ...): sizeof of the library's own dsp_mfcc_config,
 * dsp_classify_trace and dsp_classify_trace_f64 for which = 0, 1, 2 (-1 otherwise).  dsp_mfcc_config carries no size field of its own:
 * compare once after loading -- a binding built against an older header (fewer fields) must not pass its struct to this library.      */
int dsp_abi_sizeof(int which);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* DSP_AMD_H */
