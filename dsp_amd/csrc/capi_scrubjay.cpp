// capi_scrubjay.cpp -- C ABI of the scrub-jay path (include/dsp_amd.h; cepstrum/scrubjay_infer.c): the pooled statistics and the RBF-SVM,
// the fused clip kernels (clip -> label here; their one launcher also serves the stop net of capi_consumers.cpp), and the SVM's window
// scans of long recordings with their scanner.  Same rules as capi.cpp: no CPU fallback, errors through dsp_last_error().
#include <hip/hip_runtime.h>

#include <memory>

#include "mfcc_plan.hpp"

using dsp::capi_fail;

// ---- pooling + SVM ---------------------------------------------------------------------

extern "C" {

int dsp_mfcc_stats_device(const float *d_mfcc, long n_clips, int n_frames, int n_coef, float *d_feat, void *stream)
{
    if (n_clips < 0 || n_frames <= 0 || n_coef <= 0 || n_coef > 64 || (n_clips > 0 && (!d_mfcc || !d_feat)))
        return capi_fail(DSP_EINVAL, "bad argument");
    if (n_clips == 0) return DSP_OK;
    // no handle here: launch on the GPU the caller's buffer lives on
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_mfcc) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return capi_fail(DSP_EINVAL, "d_mfcc is not a device pointer");
    }
    DSP_ON_DEVICE(attr.device);
    DSP_CAPI_HIP(dsp::launch_mfcc_stats(d_mfcc, n_clips, n_frames, n_coef, d_feat, (hipStream_t)stream));
    return DSP_OK;
}

int dsp_svm_create(int device, int n_features, int n_sv, const float *offset, const float *scale,
                   const float *support_vectors, const float *coefficients, float gamma, float rho, float prob_a,
                   float prob_b, dsp_svm **out)
{
    if (!out || !offset || !scale || !support_vectors || !coefficients || n_features <= 0 || n_features > 256 || n_sv <= 0)
        return capi_fail(DSP_EINVAL, "bad argument");
    *out = nullptr;
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_svm &s) -> int {
        const size_t nf = n_features, ns = n_sv, total = 2 * nf + ns * nf + ns;
        if (s.d_blob.alloc(total * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc");
        float *p = s.d_blob;
        hipError_t e = hipMemcpy(p, offset, nf * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p + nf, scale, nf * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p + 2 * nf, support_vectors, ns * nf * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p + 2 * nf + ns * nf, coefficients, ns * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return capi_fail(DSP_EHIP, hipGetErrorString(e));
        s.m = {n_features, n_sv, gamma, rho, prob_a, prob_b, p, p + nf, p + 2 * nf, p + 2 * nf + ns * nf};
        return DSP_OK;
    });
}

void dsp_svm_destroy(dsp_svm *s) { dsp::destroy(s); }

int dsp_svm_predict_device(dsp_svm *s, const float *d_feat, long n_clips, int *d_labels, float *d_decision,
                           float *d_prob1, void *stream)
{
    if (!s || n_clips < 0 || (n_clips > 0 && (!d_feat || !d_labels))) return capi_fail(DSP_EINVAL, "bad argument");
    DSP_ON_DEVICE(s->device);
    DSP_CAPI_HIP(dsp::launch_svm_predict(s->m, d_feat, n_clips, d_labels, d_decision, d_prob1, (hipStream_t)stream));
    return DSP_OK;
}

}  // extern "C"

// ---- the fused clip kernels: clip -> label (SVM) or clip -> P(stop) in one launch, the MFCC matrix never written ----

// Ragged batch -> spans in a ring slot (uploaded on `stream`).  offsets[n_clips + 1]: clip c is samples [offsets[c], offsets[c + 1]) per
// channel of the buffer; every clip must hold at least one frame.  *t_max: frames of the longest clip.
// The kernels deal the spans to their n_waves wavefronts in fixed order (wave w walks spans w, w + n_waves, ...), so the ORDER of the
// spans is the load balance: by frame count, longest first, and snaking -- left to right over the waves in even rounds, right to left in
// odd ones -- every wave's total is within a clip of the mean (in the caller's order: +14 % on clips of 0.5 - 1.5 s).
// (host only: no HIP call) fills h[n_clips]; returns DSP_OK or DSP_EINVAL with the reason
static int build_fused_spans(const dsp_mfcc_config &cfg, const long *offsets, long n_clips, int max_frames, long n_waves, dsp::ClipSpan *h, int *t_max)
{
    std::vector<int> frames((size_t)n_clips), order((size_t)n_clips);
    int tm = 0;
    for (long c = 0; c < n_clips; ++c) {
        const long n = dsp::ragged_clip_length(offsets, c);
        if (n < 0) return (int)n;
        const int t = dsp_mfcc_frames_for(&cfg, (int)n, max_frames);
        if (t == 0) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + " of the ragged batch is shorter than one frame");
        frames[c] = t;
        tm = std::max(tm, t);
    }
    dsp::order_by_key_desc(frames.data(), n_clips, tm, order.data());
    n_waves = std::max(1L, n_waves);
    for (long i = 0; i < n_clips; ++i) {
        const long round = i / n_waves, j = i - round * n_waves;
        const long width = std::min(n_waves, n_clips - round * n_waves);          // the last round may be short
        const long pos = round * n_waves + ((round & 1) ? width - 1 - j : j);
        const long c = order[i];
        h[pos] = dsp::ClipSpan{offsets[c], (int)(offsets[c + 1] - offsets[c]), frames[c], c, 0};
    }
    *t_max = tm;
    return DSP_OK;
}

// the fused kernels' spans in the leased ring slot, uploaded on st
static int ragged_spans(dsp_mfcc_plan *p, const long *offsets, long n_clips, int max_frames, long n_waves, dsp::SpanRing::Lease &slot, int *t_max, hipStream_t st)
{
    if (n_clips >= (1L << 31)) return capi_fail(DSP_EINVAL, "too many clips");
    DSP_CAPI_HIP(p->spans.acquire((size_t)n_clips * sizeof(dsp::ClipSpan), slot));
    const int rc = build_fused_spans(p->cfg, offsets, n_clips, max_frames, n_waves, static_cast<dsp::ClipSpan *>(slot.h()), t_max);
    if (rc < 0) return rc;
    DSP_CAPI_HIP(slot.upload((size_t)n_clips * sizeof(dsp::ClipSpan), st));
    return DSP_OK;
}

/* Test hook (host only): the order a ragged batch of the fused clip kernels runs in -- spans[pos] = {start, samples, frames, caller's
 * index} as 4 longs per clip; wave w of n_waves walks pos = w, w + n_waves, ...  tests/test_capi_cpu.py checks it (also under ASan). */
extern "C" int dsp_debug_fused_spans(const dsp_mfcc_config *cfg, const long *offsets, long n_clips, int max_frames, long n_waves, long *out4)
{
    if (!cfg || !offsets || n_clips < 0 || (n_clips > 0 && !out4)) return capi_fail(DSP_EINVAL, "bad argument");
    std::vector<dsp::ClipSpan> h((size_t)n_clips);
    int tm = 0;
    const int rc = build_fused_spans(*cfg, offsets, n_clips, max_frames, n_waves, h.data(), &tm);
    if (rc < 0) return rc;
    for (long i = 0; i < n_clips; ++i) { out4[4 * i] = h[i].off; out4[4 * i + 1] = h[i].n; out4[4 * i + 2] = h[i].frames; out4[4 * i + 3] = h[i].orig; }
    return tm;
}

// mfcc_plan.hpp: grid, the ragged batch's spans for the grid's 4 * blocks waves, the launch fields, the launch
int dsp::launch_fused_clips(dsp_mfcc_plan *p, const FusedClips &c, const PoolSvmArgs *pool, const StopNetArgs *stop)
{
    const bool ragged = c.offsets != nullptr;
    int t = c.t;
    DSP_ON_DEVICE(p->device);
    hipStream_t st = (hipStream_t)c.stream;
    int blocks = grid(p, p->run.per_cu_fused, c.n_clips);
    if (stop) blocks = mfcc512_stop_grid(blocks, stop->m, c.in_kind, p->host.dct_split, p->host.dct_len, p->host.mel_gather, p->cfg.frame_length);      // what the launcher will start
    SpanRing::Lease slot;
    if (ragged) {
        const int rc = ragged_spans(p, c.offsets, c.n_clips, c.max_frames, 4L * blocks, slot, &t, st);
        if (rc < 0) return rc;
    }
    Mfcc512Args a = plan_args(p, c.in, c.in_kind, true);
    a.n_frames = c.n_clips * (long)t;
    a.n_clips = c.n_clips;
    a.spans = ragged ? static_cast<const ClipSpan *>(slot.d()) : nullptr;
    a.clip_stride = ragged ? 0 : c.clip_stride;
    a.frames_per_clip = t;
    a.chunk = t;                                  // one wavefront walks one clip
    a.samples_per_clip = ragged ? 0 : c.samples_per_clip;
    if (stop) a.stop = *stop; else a.pool = *pool;
    if (stop)
        DSP_CAPI_HIP(dsp::launch_mfcc512_stop(a, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st));
    else if (p->cfg.n_fft == 2048)      // scrubjay_infer.c's own framing (WIN_SIZE 2048, HOP_SIZE 1024): mfcc2048_kernel<POOL>
        DSP_CAPI_HIP(dsp::launch_mfcc2048(a, p->d_tables2048, blocks, st, true));
    else
        DSP_CAPI_HIP(dsp::launch_mfcc512_pool(a, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st));
    return t;
}

// clip -> label in one kernel; in_kind 0 = float samples, 1 / 2 / 3 = int16 mono / stereo channel 0 / stereo average.
// offsets != nullptr: a ragged batch (clips of different lengths back to back or anywhere in the buffer; samples_per_clip / clip_stride unused)
static int scrubjay_fused(dsp_mfcc_plan *p, dsp_svm *s, const void *d_signal, int in_kind, long n_clips, int samples_per_clip,
                          long clip_stride, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream,
                          const long *offsets = nullptr)
{
    if (in_kind < 0) return in_kind;
    if (!p || !s || n_clips < 0) return capi_fail(DSP_EINVAL, "bad argument");
    if (const int rc = dsp::plan_accepts(p, dsp::PlanUse::FusedLabel, in_kind)) return rc;
    if (s->m.n_features != 2 * p->cfg.n_mfcc || s->m.n_features > 64) return capi_fail(DSP_EINVAL, "SVM n_features must equal 2 * n_mfcc (<= 64)");
    if (p->cfg.n_fft == 512 && s->m.n_sv > dsp::kSvmFused512MaxSv)
        return capi_fail(DSP_EINVAL, "the 512-point fused clip -> label kernel holds at most " + std::to_string(dsp::kSvmFused512MaxSv) +
                                " support vectors in LDS (this SVM has " + std::to_string(s->m.n_sv) + "): use the three calls");
    const bool ragged = offsets != nullptr;
    const int t = ragged ? 1 : dsp_mfcc_frames_for(&p->cfg, samples_per_clip, max_frames);
    if (n_clips == 0) return 0;
    if (t == 0) return capi_fail(DSP_EINVAL, "clips shorter than one frame have no features to pool");
    if (!d_signal || !d_labels) return capi_fail(DSP_EINVAL, "NULL buffer");
    if (!ragged && n_clips > 1 && clip_stride < samples_per_clip) return capi_fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    if (const int rc = dsp::check_aligned(d_signal, in_kind, !ragged && n_clips > 1, clip_stride)) return rc;
    if (s->device != p->device) return capi_fail(DSP_EINVAL, "plan and SVM live on different devices");
    const dsp::FusedClips c{.in = d_signal, .in_kind = in_kind, .n_clips = n_clips, .t = t, .samples_per_clip = samples_per_clip,
                            .clip_stride = clip_stride, .offsets = offsets, .max_frames = max_frames, .stream = stream};
    const dsp::PoolSvmArgs pool{s->m, d_labels, d_decision, d_prob1, d_feat};
    return dsp::launch_fused_clips(p, c, &pool, nullptr);
}

extern "C" {

int dsp_scrubjay_fused_device(dsp_mfcc_plan *p, dsp_svm *s, const float *d_signal, long n_clips, int samples_per_clip,
                              long clip_stride, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                              void *stream)
{
    return scrubjay_fused(p, s, d_signal, 0, n_clips, samples_per_clip, clip_stride, max_frames, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_fused_pcm16_device(dsp_mfcc_plan *p, dsp_svm *s, const int16_t *d_pcm, long n_clips, int samples_per_clip, long clip_stride,
                                    int channels, int stereo_mode, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                                    void *stream)
{
    return scrubjay_fused(p, s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, samples_per_clip, clip_stride, max_frames, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_fused_ragged_device(dsp_mfcc_plan *p, dsp_svm *s, const float *d_signal, long n_clips, const long *offsets, int max_frames,
                                     int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    if (!offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    return scrubjay_fused(p, s, d_signal, 0, n_clips, 0, 0, max_frames, d_labels, d_decision, d_prob1, d_feat, stream, offsets);
}

int dsp_scrubjay_fused_ragged_pcm16_device(dsp_mfcc_plan *p, dsp_svm *s, const int16_t *d_pcm, long n_clips, const long *offsets, int channels,
                                           int stereo_mode, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                                           void *stream)
{
    if (!offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    return scrubjay_fused(p, s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, 0, 0, max_frames, d_labels, d_decision, d_prob1, d_feat, stream, offsets);
}

}  // extern "C"

// ---- window scans of long recordings with the SVM: label, decision, P(label 1) and the pooled features per sliding window ------------
// Windows are runs of MFCC rows (capi_util.hpp scan_plan).  Under complete framing and a per-frame log a row depends on its own samples
// only, so a window's rows are rows of the recording's matrix.  Under DSP_FRAMING_STREAM the first H = ceil((frame_length - hop_length) /
// hop_length) rows of a cut-out window see zeros before the window where the recording's rows see samples: each window gets its own
// head rows, from internal spans [start, start + min(H, rows) hop) of the recording (RaggedBatch with lengths).

// the first rows of a stream-framed clip that reach before it (0 under complete framing)
static int head_rows_of(const dsp_mfcc_config &c)
{
    return c.framing == DSP_FRAMING_STREAM ? (c.frame_length - c.hop_length + c.hop_length - 1) / c.hop_length : 0;
}

// host only: window g's clip in samples (absolute in the buffer), or with head_rows > 0 its head span; starts / lengths may be NULL.
// Returns the window count or < 0.
static long window_spans(const dsp_mfcc_config &c, const dsp_scan_config &sc, const long *offsets, long n, long *starts, long *lengths, int head_rows)
{
    const long wf = sc.window_frames, hf = sc.hop_frames, hop = c.hop_length;
    long g = 0;
    for (long r = 0; r < n; ++r) {
        const long len = dsp::ragged_clip_length(offsets, r);
        if (len < 0) return len;
        const long rows = dsp_mfcc_frames_for(&c, (int)len, INT_MAX);
        const long w_n = rows >= wf ? 1 + (rows - wf) / hf : 1;
        const long span = head_rows > 0 ? std::min<long>(head_rows, std::min(rows, wf)) * hop
                                        : (c.framing == DSP_FRAMING_STREAM ? wf * hop : c.frame_length + (wf - 1) * hop);
        for (long w = 0; w < w_n; ++w, ++g) {
            const long a = w * hf * hop;
            if (starts) starts[g] = offsets[r] + a;
            if (lengths) lengths[g] = std::min(span, len - a);
        }
    }
    return g;
}

// dsp_svm_scan_device and the scanner: head_rows > 0 adds window g's head rows, rows [ho[r] + w hc, + hc) of d_head (ho: n + 1 HOST longs)
static int svm_scan(dsp_svm *s, const float *d_mfcc, long n, const long *frame_offsets, const dsp_scan_config *cfg, const float *d_head, int head_rows,
                    const long *ho, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    if (!s) return capi_fail(DSP_EINVAL, "SVM is NULL");
    long rc = dsp::scan_args(cfg, n);
    if (rc < 0 || n == 0) return (int)rc;
    if (!frame_offsets || !d_mfcc || !d_labels) return capi_fail(DSP_EINVAL, "frame_offsets, d_mfcc and d_labels must not be NULL");
    if ((s->m.n_features & 1) || s->m.n_features > 128) return capi_fail(DSP_EINVAL, "the scan pools n_features / 2 <= 64 coefficients per row: n_features must be even, <= 128");
    const int tw = dsp::svm_scan_tile(s->m.n_features, cfg->window_frames, cfg->hop_frames, head_rows);
    std::vector<long> wo((size_t)n + 1), to((size_t)n + 1);
    if ((rc = dsp::scan_plan(cfg, frame_offsets, n, wo.data(), to.data(), std::max(tw, 1))) < 0) return (int)rc;
    if ((rc = dsp::refuse_rowless(frame_offsets, n, " has no MFCC rows (mfcc_stats pools a window's rows: scrubjay_infer.c:55-59)")) < 0) return (int)rc;
    DSP_ON_DEVICE(s->device);
    dsp::SpanRing::Lease slot;
    DSP_CAPI_HIP(dsp::scan_upload(s->scan, frame_offsets, n, wo.data(), to.data(), slot, stream, head_rows > 0 ? ho : nullptr));
    const long *d = static_cast<const long *>(slot.d());
    DSP_CAPI_HIP(dsp::launch_svm_scan(s->m, d_mfcc + frame_offsets[0] * (s->m.n_features / 2), d_head, n, d, d + (n + 1), d + 2 * (n + 1),
                                 head_rows > 0 ? d + 3 * (n + 1) : nullptr, to[(size_t)n], cfg->window_frames, cfg->hop_frames, head_rows, tw, d_labels,
                                 d_decision, d_prob1, d_feat, (hipStream_t)stream));
    return DSP_OK;
}

// a plan that can be scanned for samples of in_kind (plan_accepts), and an SVM that fits it
static int scan_front_end(const dsp_mfcc_plan *p, int in_kind, const dsp_svm *s)
{
    if (const int rc = dsp::plan_accepts(p, dsp::PlanUse::ScrubjayScan, in_kind)) return rc;
    if (s->m.n_features != 2 * p->cfg.n_mfcc || s->m.n_features > 64) return capi_fail(DSP_EINVAL, "SVM n_features must equal 2 * n_mfcc (<= 64)");
    if (s->device != p->device) return capi_fail(DSP_EINVAL, "plan and SVM live on different devices");
    return DSP_OK;
}

// A scrub-jay scanner: PCM -> the recordings' ragged MFCC matrix (+ the windows' head rows) in its own workspace -> svm_scan_kernel.
struct dsp_scrubjay_scanner : dsp::Handle {      // device: the plan's
    dsp::ScannerCore core;
    dsp_svm *svm = nullptr;
    int head_rows = 0;
    dsp::DeviceBuf<float> d_head;
    std::vector<long> wo, ho, starts, lengths;
};

static int scrubjay_scanner_run(dsp_scrubjay_scanner *s, const void *d_signal, int in_kind, long n, const long *offsets, int *d_labels, float *d_decision,
                                float *d_prob1, float *d_feat, void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!s || n < 0) return capi_fail(DSP_EINVAL, "bad argument (scanner, n_recordings >= 0)");
    if (n == 0) return DSP_OK;
    if (!offsets || !d_labels) return capi_fail(DSP_EINVAL, "offsets and d_labels must not be NULL");
    if (n >= (1L << 31)) return capi_fail(DSP_EINVAL, "too many recordings");
    dsp_mfcc_plan *p = s->core.plan;
    if (const int rc = scan_front_end(p, in_kind, s->svm)) return rc;
    std::lock_guard<std::mutex> lock(s->core.mu);
    const long rows = s->core.mfcc(d_signal, in_kind, n, offsets, " is shorter than one frame: mfcc_stats has no rows to pool (scrubjay_infer.c:55-59)", stream);
    if (rows < 0) return (int)rows;
    const long *fo = s->core.fo.data();
    const dsp_scan_config &cfg = s->core.cfg;
    if (s->head_rows > 0) {
        // window g of recording r: its min(H, rows) head rows at ho[r] + (g - wo[r]) hc_r, computed from its own head span
        s->wo.resize((size_t)n + 1);
        const long n_win = dsp::scan_plan(&cfg, fo, n, s->wo.data(), nullptr, 1);
        if (n_win < 0) return (int)n_win;
        s->starts.resize((size_t)n_win);
        s->lengths.resize((size_t)n_win);
        if (window_spans(p->cfg, cfg, offsets, n, s->starts.data(), s->lengths.data(), s->head_rows) != n_win) return capi_fail(DSP_EINVAL, "internal: head spans");
        s->ho.resize((size_t)n + 1);
        s->ho[0] = 0;
        for (long r = 0; r < n; ++r) {
            const long hc = std::min<long>(s->head_rows, std::min<long>(fo[r + 1] - fo[r], cfg.window_frames));
            s->ho[(size_t)r + 1] = s->ho[(size_t)r] + (s->wo[(size_t)r + 1] - s->wo[(size_t)r]) * hc;
        }
        DSP_ON_DEVICE(p->device);
        if (s->d_head.reserve((size_t)s->ho[(size_t)n] * p->cfg.n_mfcc * sizeof(float)) != hipSuccess)
            return capi_fail(DSP_ENOMEM, "hipMalloc (scanner head-row workspace)");
        const int rc = dsp::mfcc_clips_ragged(p, d_signal, in_kind, n_win, s->starts.data(), INT_MAX, s->d_head, stream, s->lengths.data());
        if (rc < 0) return rc;
    }
    return svm_scan(s->svm, s->core.d_mfcc, n, fo, &cfg, s->d_head, s->head_rows, s->ho.data(), d_labels, d_decision, d_prob1, d_feat, stream);
}

extern "C" {

long dsp_scan_window_spans(const dsp_mfcc_config *mfcc, const dsp_scan_config *cfg, const long *offsets, long n_recordings, long *starts, long *lengths)
{
    if (!mfcc) return capi_fail(DSP_EINVAL, "mfcc config is NULL");
    std::string why;
    if (!dsp::valid_cfg(*mfcc, why)) return capi_fail(DSP_EINVAL, why);
    if (mfcc->framing == DSP_FRAMING_CENTER) return capi_fail(DSP_EINVAL, "framing: windows are not cut under DSP_FRAMING_CENTER (n_fft 400 plans are not scanned)");
    if (const int rc = dsp::scan_args(cfg, n_recordings)) return rc;
    if (n_recordings == 0) return 0;
    if (!offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    return window_spans(*mfcc, *cfg, offsets, n_recordings, starts, lengths, 0);
}

int dsp_svm_scan_device(dsp_svm *svm, const float *d_mfcc, long n_recordings, const long *frame_offsets, const dsp_scan_config *cfg, int *d_labels,
                        float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    return svm_scan(svm, d_mfcc, n_recordings, frame_offsets, cfg, nullptr, 0, nullptr, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_scanner_create(dsp_mfcc_plan *plan, dsp_svm *svm, const dsp_scan_config *cfg, dsp_scrubjay_scanner **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (!plan || !svm) return capi_fail(DSP_EINVAL, "plan and SVM must not be NULL");
    if (const int rc = dsp::scan_args(cfg, 0)) return rc;
    if (const int rc = scan_front_end(plan, 0, svm)) return rc;
    return dsp::create_on_host(plan->device, out, [&](dsp_scrubjay_scanner &s) {
        s.core.plan = plan;
        s.core.cfg = *cfg;
        s.svm = svm;
        s.head_rows = head_rows_of(plan->cfg);
        return DSP_OK;
    });
}

void dsp_scrubjay_scanner_destroy(dsp_scrubjay_scanner *s) { dsp::destroy(s); }

int dsp_scrubjay_scanner_run_device(dsp_scrubjay_scanner *s, const float *d_signal, long n_recordings, const long *offsets, int *d_labels,
                                    float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    return scrubjay_scanner_run(s, d_signal, 0, n_recordings, offsets, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_scanner_run_pcm16_device(dsp_scrubjay_scanner *s, const int16_t *d_pcm, long n_recordings, const long *offsets, int channels,
                                          int stereo_mode, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    return scrubjay_scanner_run(s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_recordings, offsets, d_labels, d_decision, d_prob1, d_feat, stream);
}

}  // extern "C"
