// mfcc_plan.hpp -- the MFCC plan, the SVM and the plan-level launchers, for the host translation units of the C ABI that read a plan:
// capi.cpp (owner of the plan: lifecycle, the MFCC entry points), capi_scrubjay.cpp (SVM, fused clip kernels, SVM scans),
// capi_consumers.cpp (stop net, speaker GMM, their scanner) and capi_stream.cpp (stream sessions).  Host only, internal.
#pragma once

#include <cstdint>

#include "capi_util.hpp"
#include "mfcc_kernels.hpp"
#include "svm_kernels.hpp"
#include "tables.hpp"

// the jobs below are filled field by name, MfccJob{.in = ..., .n_frames = ...}: designated initialisers, which this compiler takes in C++17
#pragma clang diagnostic ignored "-Wc++20-designator"

namespace dsp {

// The kernel a plan runs and its grid, resolved once: by dsp_mfcc_plan_create and again by dsp_mfcc_plan_set_kernel (capi.cpp).
struct PlanKernel {
    // FFT512_TILE: the wave-per-frame kernel's 16-frame tile epilogue (DSP_KERNEL_WAVE, per-frame log mode); FFT512_FRAME: its per-frame
    // epilogue (DSP_KERNEL_WAVE_FRAME, or DSP_LOG_GLOBAL_REF1); FFT1024_WAVE: the register-resident kernel (<= 3 mel chunk slots per lane
    // and no DSP_KERNEL_ROW); FFT1024_ROW: the general Stockham kernel; FFT2048_AUBIO: magnitude spectrum, log10 floor or stream framing
    enum Family { FFT400, FFT512_TILE, FFT512_FRAME, FFT1024_WAVE, FFT1024_ROW, FFT2048, FFT2048_AUBIO } family = FFT512_TILE;
    int granule = 1;      // a chunk holds a whole number of these frames (tile: half-tiles of 8)
    // resident 256-thread blocks per CU (occupancy queries): the plain entry; FFT1024_WAVE's one-pass prefilter (0: the plan has none);
    // the fused clip kernels, label and stop (0: the family has none)
    int per_cu = 4, per_cu_prefilter = 0, per_cu_fused = 0;
};

}  // namespace dsp

struct dsp_mfcc_plan : dsp::Handle {
    dsp_mfcc_config cfg;
    int n_cu = 0;
    int kernel = DSP_KERNEL_WAVE;   // what dsp_mfcc_plan_set_kernel asked for
    dsp::PlanKernel run;            // what that means on this plan
    int blocks_per_cu = 0;   // 0 = default (= run.per_cu*)
    int chunk = 0;           // 0 = default
    dsp::LaneTables512 host;
    dsp::DeviceBuf<dsp::LaneTables512> d_tables;
    dsp::DeviceBuf<dsp::GenTables1024> d_gen_tables;   // n_fft = 1024
    bool wave1024_fits = false;                        // its filterbank fits the wave kernel (<= 3 mel chunk slots per lane)
    dsp::DeviceBuf<dsp::GenTables2048> d_tables2048;   // n_fft = 2048
    dsp::DeviceBuf<dsp::Tables400> d_tables400;        // n_fft = 400
    dsp::DeviceBuf<dsp::PrefilterScan> d_scan;    // prefilter fused into the 1024-point wave kernel (full frames): its tables
    int scan_steps[4] = {6, 6, 6, 6};             // host copy of PrefilterScan::c_steps (picks the kernel instantiation)
    dsp::DeviceBuf<float> d_filtered;             // per-frame prefilter output (sub-batch)
    dsp::DeviceBuf<float> d_frame_max, d_clip_floor;   // DSP_LOG_GLOBAL_REF1 two-pass workspace
    // Guards the plan's workspaces (d_filtered, d_frame_max / d_clip_floor) while a call reserves them and
    // enqueues the kernels that use them.  The kernels themselves run after the lock is released: a plan whose path uses
    // a workspace (prefilter, DSP_LOG_GLOBAL_REF1 over clips) serves ONE stream at a time;
    // the workspace-free paths (frames / clips / pcm16 / fused, per-frame log mode) may be driven from several streams.
    // The *_host entry points hold it for the whole call (their staging is the device's host pipeline, host_pipe.hpp, whose lock is
    // taken after this one).
    std::recursive_mutex mu;
    dsp::SpanRing spans;      // ragged batches of the fused clip kernels: the clips' spans on their way to the GPU (capi_util.hpp)
};

struct dsp_svm : dsp::Handle {
    dsp::SvmModelDev m{};
    dsp::DeviceBuf<float> d_blob;
    dsp::SpanRing scan;      // dsp_svm_scan_device: the per-recording arrays on their way to the GPU (capi_util.hpp)
};

namespace dsp {

bool valid_cfg(const dsp_mfcc_config &c, std::string &why);      // capi.cpp: what dsp_mfcc_plan_create accepts

// in_kind everywhere below: 0 float samples, 1 / 2 / 3 int16 mono / stereo channel 0 / stereo average (pcm16_kind); < 0 is pcm16_kind's
// error, handed back as it is

// A ragged batch: clip c = samples [offsets[c], offsets[c + 1]) per channel -- or [offsets[c], offsets[c] + lengths[c]) when
// lengths is given (spans anywhere in the buffer, overlapping ones included) -- frame_offsets[c] its first output row (prefix sums of the
// clips' frame counts), n_spans the clips with at least one frame.
struct RaggedBatch {
    const long *offsets, *frame_offsets;
    long n_clips, n_spans;
    const long *lengths = nullptr;
};

// One enqueue of the plan's MFCC kernel (capi.cpp mfcc_run).  frames_per_clip = 0: independent frames back to back; > 0: clips of
// samples_per_clip samples, clip_stride apart.  ragged: a ragged batch instead (frames_per_clip = 0, clip_stride unused): the
// clip-mode kernels with the RaggedCursor.
struct MfccJob {
    const void *in = nullptr;
    int in_kind = 0;
    float *out = nullptr;
    long n_frames = 0;
    int frames_per_clip = 0, samples_per_clip = 0;
    long clip_stride = 0;
    bool fused_prefilter = false;      // the per-frame Butterworth inside the 1024-point wave kernel
    const RaggedBatch *ragged = nullptr;
    void *stream = nullptr;
};
int mfcc_run(dsp_mfcc_plan *p, const MfccJob &job);

// capi.cpp: dsp_mfcc_clips_device / _pcm16_device by in_kind; the frames per clip
int mfcc_clips(dsp_mfcc_plan *p, const void *d_in, int in_kind, long n_clips, int samples_per_clip, long clip_stride, float *d_out, int max_frames,
               void *stream);
// capi.cpp: dsp_mfcc_clips_ragged_device / _pcm16_device by in_kind; the frames of the longest clip.  lengths: spans (RaggedBatch)
int mfcc_clips_ragged(dsp_mfcc_plan *p, const void *d_in, int in_kind, long n_clips, const long *offsets, int max_frames, float *d_out, void *stream,
                      const long *lengths = nullptr);
// What a plan is asked to do, and the one place that says whether it can (capi.cpp): the plan's family and configuration against the
// use, a 512-point plan's shape against the kernel's list of forms (mfcc512_has_form).  Checks on a model stay with the model's owner.
// Frames / Clips / Ragged: MFCC rows of independent frames, equal clips, a ragged batch; FusedLabel / FusedStop: the clip -> label and
// clip -> P(stop) kernels; Scan: a stop / speaker scanner or a stream session; ScrubjayScan: an SVM scanner.
enum class PlanUse { Frames, Clips, Ragged, FusedLabel, FusedStop, Scan, ScrubjayScan };
// DSP_OK, or DSP_EINVAL with the reason.  FusedStop has a two-kernel path behind it: 1 (the fused form exists), 0 (none: take the other
// path) or DSP_EINVAL (neither path takes this plan)
int plan_accepts(const dsp_mfcc_plan *p, PlanUse use, int in_kind);

// the kernels' 8-byte frame loads (4-byte for mono int16); strided: clip starts clip_stride apart are read
inline bool input_aligned(const void *d_in, int in_kind, bool strided, long clip_stride)
{
    return !(reinterpret_cast<uintptr_t>(d_in) & (in_kind == 1 ? 3 : 7)) && !(strided && (clip_stride & 1));
}
inline int check_aligned(const void *d_in, int in_kind, bool strided, long clip_stride)
{
    return input_aligned(d_in, in_kind, strided, clip_stride) ? DSP_OK
           : capi_fail(DSP_EINVAL, "input must be 8-byte aligned (4 for mono int16) with an even clip stride");
}

// the launch fields every path takes from the plan (clip_mode: stream framing applies to clips; independent frames are whole frames)
inline Mfcc512Args plan_args(const dsp_mfcc_plan *p, const void *d_in, int in_kind, bool clip_mode)
{
    const dsp_mfcc_config &c = p->cfg;
    return {.in = d_in, .in_kind = in_kind, .tables = p->d_tables, .hop = c.hop_length, .frame_len = c.frame_length, .n_mels = c.n_mels,
            .n_mfcc = c.n_mfcc, .amin = c.amin, .top_db = c.top_db, .log_mode = c.log_mode, .spectrum = c.spectrum,
            .stream_framing = clip_mode && c.framing == DSP_FRAMING_STREAM,
            .center_framing = clip_mode && c.framing == DSP_FRAMING_CENTER};
}

// persistent-style grid: exactly the 4-wave blocks the chip holds at once (per_cu per CU unless dsp_mfcc_plan_set_launch says otherwise;
// one extra block per CU would run as a second, mostly idle round: measured +14 %), never more blocks than `items` of work fill
inline int grid(const dsp_mfcc_plan *p, int per_cu, long items)
{
    return (int)std::max(1L, std::min((long)p->n_cu * (p->blocks_per_cu > 0 ? p->blocks_per_cu : per_cu), (items + 3) / 4));
}

// A batch of clips for a fused clip kernel (one wavefront walks one clip, the MFCC matrix is never written).  offsets == nullptr: n_clips
// clips of t frames, clip_stride apart; offsets given: a ragged batch (clip c = samples [offsets[c], offsets[c + 1]) per channel, every
// clip with its own frames up to max_frames; t, samples_per_clip and clip_stride unused).
struct FusedClips {
    const void *in = nullptr;
    int in_kind = 0;
    long n_clips = 0;
    int t = 0, samples_per_clip = 0;
    long clip_stride = 0;
    const long *offsets = nullptr;
    int max_frames = 0;
    void *stream = nullptr;
};
// capi_scrubjay.cpp: the one launch of the fused clip kernels, on a plan and a batch its caller has accepted (input_aligned included): the
// SVM's (pool) or the stop net's (stop), one of them non-NULL.  The frames of the longest clip, or < 0.
int launch_fused_clips(dsp_mfcc_plan *p, const FusedClips &c, const PoolSvmArgs *pool, const StopNetArgs *stop);

// capi_consumers.cpp (owner of the models): what dsp_scanner_create and dsp_stream_session_create ask of a plan and of the models they
// borrow -- plan_accepts(Scan) for samples of in_kind, n_coef / d = the plan's n_mfcc on the plan's device, a stop window that fits the
// scan kernel's LDS.  stop / speaker may be NULL (cfg is read only when one is given).  DSP_OK or DSP_EINVAL.
int scan_front_check(const dsp_mfcc_plan *plan, int in_kind, const dsp_stop_model *stop, const dsp_speaker_model *speaker, const dsp_scan_config *cfg);

// What the scanners share (dsp_scanner of capi_consumers.cpp, where mfcc() lives; dsp_scrubjay_scanner of capi_scrubjay.cpp): PCM -> the recordings' ragged MFCC matrix in the scanner's own workspace.
struct ScannerCore {
    dsp_mfcc_plan *plan = nullptr;      // (its device is the scanner's: Handle::device)
    dsp_scan_config cfg{};
    DeviceBuf<float> d_mfcc;
    std::vector<long> fo;      // recording r = rows [fo[r], fo[r + 1]) of d_mfcc
    std::mutex mu;             // held by the caller across mfcc() and the scans that read d_mfcc
    // every row of every recording (no cap) into d_mfcc; the rows in total, or < 0.  rowless_tail: a recording without rows is refused
    // as "recording r<tail>" (nullptr: such recordings pass)
    long mfcc(const void *d_signal, int in_kind, long n, const long *offsets, const char *rowless_tail, void *stream);
};

}  // namespace dsp
