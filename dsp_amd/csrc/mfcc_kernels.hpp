// mfcc_kernels.hpp -- launch interface of mfcc_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include "clip_span.hpp"
#include "consumer_kernels.hpp"
#include "svm_kernels.hpp"
#include "tables.hpp"

namespace dsp {

// BASELINE config 5 in ONE kernel (clip mode, one wavefront per clip): the MFCC matrix is never written; the
// tile epilogue pools mean | std per coefficient (cepstrum/scrubjay_infer.c:36-66, float64 sums in frame order)
// and the clip ends with Scaler -> RBF-SVM -> Platt (scrubjay_svm.onnx, scrubjay_infer.c:105-141).
constexpr int kSvmFused512MaxSv = 2048;    // the 512-point fused kernel's LDS copy of the SVM's coefficients (launch_mfcc512_pool)

struct PoolSvmArgs {
    SvmModelDev svm;       // n_features = 2 * n_mfcc
    int *labels;           // [n_clips]
    float *decision;       // [n_clips] or nullptr
    float *prob1;          // [n_clips] or nullptr
    float *feat;           // [n_clips][2 * n_mfcc] or nullptr
};

// classify_signal in ONE kernel (2fa/audio/word/c/stop_detector.c:12-55): the tile epilogue standardises its
// 16 x 13 coefficients and adds their layer-1 products (audio_classifier_inference.c:18-36, 44-47) to float64 partial sums,
// the clip ends with layers 2-4 and the sigmoid -- the MFCC matrix never reaches HBM.
struct StopNetArgs {
    StopModelDev m;        // units[0] <= kStopFusedUnits, n_coef = n_mfcc <= 16
    float *prob;           // [n_clips]
};

struct Mfcc512Args {
    const void *in;                // HBM: frames or clips; float32, or int16 PCM (in_kind)
    int in_kind;                   // 0 float32 | 1 int16 mono | 2 int16 stereo ch 0 | 3 int16 stereo average
    float *out;                    // HBM: [n_frames][n_mfcc]
    const LaneTables512 *tables;   // HBM: per-lane constants
    long n_frames;                 // total frames over all clips
    long clip_stride;              // floats between clip starts (clip mode)
    int frames_per_clip;           // 0: independent frames back to back
    int hop;                       // clip mode: floats between frame starts
    int frame_len;                 // <= 512
    int chunk;                     // consecutive frames one wave takes at a time
    int n_mels, n_mfcc;
    float amin, top_db;
    // log_mode 1 (librosa power_to_db, ref = 1, top_db over the whole clip):
    //   frame_max != nullptr : pass 1, only write 10 log10(max mel energy) per frame, no MFCC
    //   clip_floor != nullptr: pass 2, clip log-mel at clip_floor[clip]
    //   both nullptr         : every frame is its own clip (independent frames), one pass
    // log_mode 2 (DSP_LOG_LOG10_FLOOR, n_fft 2048): plain log10 with aubio's 2e-42 floor
    int log_mode;
    // n_fft 2048 only (the aubio-semantics front end of cepstrum/scrubjay_infer.c): spectrum 1 = magnitude into the filterbank;
    // stream_framing: frame t of a clip covers samples [(t + 1) hop - frame_len, (t + 1) hop), zeros outside [0, samples_per_clip)
    int spectrum = 0;
    int stream_framing = 0;
    // n_fft 400 and 2048 (DSP_FRAMING_CENTER, clips): frame t covers samples [t hop - frame_len / 2, t hop + frame_len / 2), zeros outside
    // [0, samples_per_clip)
    int center_framing = 0;
    int samples_per_clip = 0;
    float *frame_max;
    const float *clip_floor;
    // the fused clip kernels (POOL; one wavefront walks one clip): the clip count, and for a ragged batch the clips' spans
    // (spans == nullptr: clip c starts at c * clip_stride and has frames_per_clip frames of samples_per_clip samples).
    // Ragged MFCC matrices (launch_mfcc512 / launch_mfcc2048 with spans set): n_clips spans of >= 1 frame in the caller's order, their
    // ClipSpan::frame0 the first output frame, and behind them the int chunk table of launch_ragged_chunk_map
    long n_clips = 0;
    const ClipSpan *spans = nullptr;
    PoolSvmArgs pool;              // only read by the POOL instantiations (launch_mfcc512_pool)
    StopNetArgs stop{};            // only read by the stop-net instantiations (launch_mfcc512_stop)
};

// The forms of mfcc512_wave_kernel (mfcc_kernels.hip), one row per shape: THE list.  The launchers instantiate a form exactly when it
// is listed here and the host asks mfcc512_has_form before it promises a caller anything.  Every shape has float input at FLEN 512 and
// at FLEN 0 (a run-time predicate for frame lengths below 512), independent frames, clips and ragged batches, tile and per-frame
// epilogue, and the fused clip -> label kernel; the columns say what a shape has beyond that.
//   SPLIT, LEN, GATHER  the shape build_lane_tables_512 selects (LaneTables512::dct_split, dct_len, mel_gather)
//   FLEN400    a compile-time FLEN 400 (the reference's framing, -5 % in clip mode): the shapes of BASELINE configs 4 and 5
//   ROWS16     plain MFCC rows take int16 PCM: clips and ragged batches on the tile epilogue, every FLEN the shape has
//   LABEL16    the frame length at which the fused clip -> label kernel takes int16 (0: float only): what scrubjay_infer.c's and
//              stop_detector.c's callers decode from their WAV files
//   STOP       the fused clip -> stop-word kernel exists (float: FLEN 400 where the shape has it, FLEN 0 otherwise)
//   STOP16     the frame length at which it takes int16 (0: float only): main_test.c's reader in front of classify_signal
//                       SPLIT LEN GATHER FLEN400 ROWS16 LABEL16 STOP  STOP16
#define DSP_MFCC512_FORMS(X)                              \
    X(4, 10, 3, true, true, 400, true, 400)               \
    X(4, 10, 6, false, false, 0, true, 0)                 \
    X(4, 16, 3, false, false, 0, false, 0)                \
    X(4, 16, 6, false, false, 0, false, 0)                \
    X(2, 20, 3, true, false, 400, false, 0)               \
    X(2, 20, 6, false, false, 0, false, 0)

struct Mfcc512Form { int split, len, gather; bool flen400, rows_pcm16; int label_pcm16_flen; bool stop; int stop_pcm16_flen; };
#define DSP_FORM_ROW(...) {__VA_ARGS__},
constexpr Mfcc512Form kMfcc512Forms[] = {DSP_MFCC512_FORMS(DSP_FORM_ROW)};
#undef DSP_FORM_ROW

constexpr const Mfcc512Form *mfcc512_form(int split, int len, int gather)
{
    for (const Mfcc512Form &f : kMfcc512Forms)
        if (f.split == split && f.len == len && f.gather == gather) return &f;
    return nullptr;
}

// what a launch is for: independent frames or clips (ragged batches included) into MFCC rows, clip -> label, clip -> P(stop)
enum class Mfcc512Use { Frames, Clips, Label, Stop };

// "this form exists": in_kind as Mfcc512Args::in_kind; tile: the 16-frame tile epilogue (the fused kernels have no other).  The launchers
// below return hipErrorInvalidConfiguration for a form exactly when this says no
constexpr bool mfcc512_has_form(Mfcc512Use use, int split, int len, int gather, int frame_len, int in_kind, bool tile)
{
    const Mfcc512Form *f = mfcc512_form(split, len, gather);
    if (!f || in_kind < 0 || in_kind > 3) return false;
    if (use == Mfcc512Use::Frames) return in_kind == 0;
    if (use == Mfcc512Use::Clips) return in_kind == 0 || (f->rows_pcm16 && tile);
    const int flen16 = use == Mfcc512Use::Label ? f->label_pcm16_flen : f->stop_pcm16_flen;
    return tile && (in_kind == 0 ? use == Mfcc512Use::Label || f->stop : flen16 != 0 && frame_len == flen16);
}
// the ROWS16 shapes in a caller's terms, for the refusal that names them (kept beside the list: it restates that column)
constexpr const char *kMfcc512RowsPcm16Shapes = "n_mfcc <= 16 with n_mels <= 40 and no mel filter wider than 36 FFT bins (kernel shape 4 x 10, gather 3: "
                                                "dsp_mfcc_default_config's)";

// clip_floor[c] = max_t frame_max[c][t] - top_db
hipError_t launch_clip_floor(const float *frame_max, long n_clips, int frames_per_clip, float top_db, float *clip_floor,
                             hipStream_t stream);

// ragged (args.spans): clip_floor[s] = max over span s's frames of frame_max - top_db
hipError_t launch_clip_floor_ragged(const float *frame_max, const ClipSpan *spans, long n_spans, float top_db, float *clip_floor, hipStream_t stream);
// ragged: chunk_span[k] = the span holding frame k * chunk, k < ceil(total frames / chunk) -- the table RaggedCursor starts its chunks from
hipError_t launch_ragged_chunk_map(const ClipSpan *spans, long n_spans, int chunk, int *chunk_span, hipStream_t stream);

// tile: 16-frame log + MFMA-DCT epilogue (per-frame log mode, chunk % 8 == 0); false: per-frame epilogue
hipError_t launch_mfcc512(const Mfcc512Args &args, int dct_split, int dct_len, int gather, int blocks,
                          hipStream_t stream, bool tile);
// fused clip -> label path: args.chunk must equal args.frames_per_clip, args.out is not written
hipError_t launch_mfcc512_pool(const Mfcc512Args &args, int dct_split, int dct_len, int gather, int blocks, hipStream_t stream);
// fused clip -> stop-word probability (the STOP shapes of the list): args.chunk == args.frames_per_clip, args.stop set
int mfcc512_stop_grid(int blocks, const StopModelDev &m, int in_kind, int dct_split, int dct_len, int gather, int frame_len);      // the grid launch_mfcc512_stop starts for a caller's count
hipError_t launch_mfcc512_stop(const Mfcc512Args &args, int dct_split, int dct_len, int gather, int blocks, hipStream_t stream);
hipError_t launch_mfcc1024(const Mfcc512Args &args, const GenTables1024 *tables, int blocks, hipStream_t stream);
int mfcc1024_blocks_per_cu(bool full);
// register-resident wave-per-frame form (mfcc1024_wave_kernel.hip): tables->n_chunk_slots <= 3, chunk % 8 == 0
struct PrefilterScan;   // tables.hpp
// scan != nullptr: independent 1024-sample frames are band-pass filtered (PrefilterScan, tables.hpp) inside the kernel
// scan_steps (host copy of PrefilterScan::c_steps, with scan): picks the instantiation whose compile-time step counts cover them
hipError_t launch_mfcc1024_wave(const Mfcc512Args &args, const GenTables1024 *tables, int blocks, hipStream_t stream,
                                const PrefilterScan *scan = nullptr, const int *scan_steps = nullptr);
int mfcc1024_wave_blocks_per_cu(bool full, bool prefilter = false);
int mfcc512_lds_bytes_per_block(bool tile);
// n_fft = 2048 (mfcc2048_kernel.hip); pool: the fused clip -> label form (args.chunk == args.frames_per_clip, args.pool set)
struct GenTables2048;
hipError_t launch_mfcc2048(const Mfcc512Args &args, const GenTables2048 *tables, int blocks, hipStream_t stream, bool pool);
int mfcc2048_blocks_per_cu(int n_mels, bool pool, bool aub = false);      // aub: the aubio-semantics kernels (spectrum / log10 / stream framing) and their LDS
int mfcc512_blocks_per_cu(int dct_split, int dct_len, int gather, bool full, bool tile);
// n_fft = 400 (mfcc400_kernel.hip): float frames, clips (complete or centred framing) and ragged batches, both log modes
struct Tables400;
hipError_t launch_mfcc400(const Mfcc512Args &args, const Tables400 *tables, int blocks, hipStream_t stream);
int mfcc400_blocks_per_cu(int n_mels);

}  // namespace dsp
