// capi_classify_f32.cpp -- C ABI of the float32 donut classifier (include/dsp_amd.h: dsp_classify*, the single-clip helpers of
// sync/lib/classifier.h), the per-clip chain of sync/lib/classifier.cpp on the GPU in float, bit-exact against the compiled reference:
//     iir2_ckpt_kernel (both band-passes, delay lines at every segment start, the energy gate) -> spec_from_ckpt<flags> (1000-3000 Hz
//     map, loud bins) -> classify_midpoints -> spec_from_ckpt<maps> (3000-7500 Hz, clips with midpoints only) -> classify_bands
// The batch entries (uniform and ragged, host and device memory, float and int16 PCM) are classify_front.hpp's.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdio>
#include <new>
#include <thread>
#include <utility>

#include "classify_front.hpp"

static_assert(sizeof(dsp::ClassifyTrace) == sizeof(dsp_classify_trace), "trace layouts must match");

namespace {

namespace front = dsp::front;

dsp::IirCoef coef_f32(double lo, double hi)
{
    double b[9], a[9];
    dsp_butter_bandpass(lo, hi, b, a);
    dsp::IirCoef c;
    for (int i = 0; i < 9; ++i) { c.b[i] = (float)b[i]; c.a[i] = (float)a[i]; }   // classifier.cpp:140-183: float literals
    return c;
}

// counts the floats of its range on which the recompute kernel's three-instruction PSD division differs from the real division, for
// this table's U, on the current device (~1e9 values: a fraction of a millisecond)
hipError_t spec_div_mismatches(const dsp::SpecTables *d_tab, unsigned long long &bad)
{
    dsp::DeviceBuf<unsigned long long> d_bad;
    hipError_t e = d_bad.alloc(sizeof(bad));
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(bad), nullptr);
    if (e == hipSuccess) e = dsp::launch_spec_div_verify(d_tab, d_bad, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    return e;
}

// the workspace for one sub-batch: allocated together, let go together (ClassifyCtx::reserve)
struct ClassifyBufs {
    dsp::DeviceBuf<float> d_sbp;                           // 3000-7500 Hz PSD maps [clip][T][129]
    dsp::DeviceBuf<float> d_ck_bp, d_ck_mp;                // [clip][T][kCkPerSegBp / Mp][8]: delay line of each filter at every segment start (3000-7500 Hz: and middle)
    dsp::DeviceBuf<float> d_mean_mp;                       // [clip][T]: segment means of the 1000-3000 Hz output
    dsp::DeviceBuf<int> labels, d_hits;                    // d_hits: work list of clips with midpoints
    dsp::DeviceBuf<int> d_loud;                            // [clip][T]: time bins of the 1000-3000 Hz map above 70 dB; after the midpoints kernel: rows of the 3000-7500 Hz map the band sums read
    dsp::DeviceBuf<unsigned> d_minmax;                     // [clip][2]: float bits of the smallest / largest positive cell of the 3000-7500 Hz map
    dsp::DeviceBuf<int> d_simd;                            // iir2_ckpt_kernel's per-CU SIMD load table (launch_iir2_ckpt)
    dsp::DeviceBuf<int> d_gate;                            // work list of the segments whose energy does not rule a loud cell out (IIR kernel)
    dsp::DeviceBuf<dsp::ClassifyTrace> trace;
    long cap_clips = 0;                                    // per-clip arrays (labels, hits, trace, minmax)
    long cap_segs = 0;                                     // per-segment arrays: clips x segments per clip of the largest pass so far
};

struct ClassifyCtx : front::Work, ClassifyBufs {
    using Config = dsp_classify_config;
    using Trace = dsp_classify_trace;
    static constexpr int kFloatBytes = 4;

    dsp::DeviceBuf<dsp::SpecTables> d_tab;                 // held = the workspace is initialised (init())
    float keep_min_db = 70.0f;                             // the midpoint threshold d_tab->mp_keep_min was computed for

    static Config default_config()
    {
        // sync/lib/classifier.cpp:67-68 (0.65 / 0.80), :436 (70 dB), :109 (100 / 200 / 80)
        return Config{0.65f, 0.80f, 70.0f, 100.0f, 200.0f, 80.0f};
    }
    static bool valid(const Config &c)
    {
        auto fin = [](float v) { return v == v && v - v == 0.0f; };
        return fin(c.keep_lo) && fin(c.keep_hi) && fin(c.midpoint_db) && fin(c.middle_max) && fin(c.above_min) && fin(c.below_min) &&
               c.keep_lo < c.keep_hi;
    }
    static int pipeline(int, bool) { return 0; }
    // clips per pass through the workspace (42 KB per 1 s clip): 1024 blocks of 64 clips = the four IIR blocks a CU holds
    static long sub_batch(int) { return 65536; }

    int init()
    {
        if (d_tab) return DSP_OK;
        // built in a local and handed to d_tab after the last step that can fail: a failed init() leaves the workspace unopened
        dsp::SpecTables t;
        dsp::build_spec_tables(16000, t);
        dsp::DeviceBuf<dsp::SpecTables> tab;
        DSP_CAPI_HIP(dsp::upload(tab, t));
        DSP_CAPI_HIP(dsp::launch_spec_threshold(tab, 70.0f, nullptr));
        // the recompute kernel's three-instruction PSD division is switched on only after it has been checked against the real one
        unsigned long long bad = 1;
        const hipError_t e = spec_div_mismatches(tab, bad);
        if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
        const int on = bad == 0 && !std::getenv("DSP_AMD_SPEC_EXACT_DIV") ? 1 : 0;
        DSP_CAPI_HIP(hipMemcpy(reinterpret_cast<char *>(tab.get()) + offsetof(dsp::SpecTables, div_fast), &on, sizeof(on), hipMemcpyHostToDevice));
        DSP_CAPI_HIP(hipStreamSynchronize(nullptr));
        d_tab = std::move(tab);
        keep_min_db = 70.0f;
        return DSP_OK;
    }

    void free_workspace() { static_cast<ClassifyBufs &>(*this) = ClassifyBufs{}; }
    void free_all()
    {
        free_workspace();
        d_tab.reset();
    }

    // The per-segment arrays are [clip][T(n)] with the pass's own T, so what a pass needs of them is its PRODUCT clips x T: a ragged
    // batch's pass of few long clips and its pass of many short ones share one allocation (sized by each dimension's maximum it would
    // be their outer product -- 32 GB of maps for 65 536 clips of which one is 13 s long).
    int reserve(int, long clips, int n)
    {
        const long T = std::max(1, front::columns(n));
        if (clips <= cap_clips && clips * T <= cap_segs) return DSP_OK;
        wait_idle();
        const long rows = std::max(clips, cap_clips), segs = std::max(clips * T, cap_segs);
        free_workspace();      // (cap_clips and cap_segs stay 0 if an allocation below fails: the next call starts over)
        DSP_CAPI_HIP(d_sbp.alloc((size_t)segs * dsp::kSpecBins * sizeof(float)));
        DSP_CAPI_HIP(d_ck_bp.alloc((size_t)segs * dsp::kCkPerSegBp * 8 * sizeof(float)));
        DSP_CAPI_HIP(d_ck_mp.alloc((size_t)segs * dsp::kCkPerSegMp * 8 * sizeof(float)));
        DSP_CAPI_HIP(d_loud.alloc((size_t)segs * sizeof(int)));
        DSP_CAPI_HIP(d_minmax.alloc((size_t)rows * 2 * sizeof(unsigned)));
        DSP_CAPI_HIP(d_simd.alloc(sizeof(int) * dsp::kSimdLoadCus * dsp::kSimdLoadStride));
        DSP_CAPI_HIP(d_gate.alloc(((size_t)segs + 1) * sizeof(int)));      // work list of gated-in frames: count + frame numbers
        DSP_CAPI_HIP(d_mean_mp.alloc((size_t)segs * sizeof(float)));
        DSP_CAPI_HIP(labels.alloc((size_t)rows * sizeof(int)));
        DSP_CAPI_HIP(d_hits.alloc((size_t)(rows + 1) * sizeof(int)));
        DSP_CAPI_HIP(trace.alloc((size_t)rows * sizeof(dsp::ClassifyTrace)));
        cap_clips = rows; cap_segs = segs;
        return DSP_OK;
    }

    // one sub-batch already resident at d_x (row stride in samples per channel): labels (+ trace) into the workspace
    // spans != nullptr: a ragged sub-batch (clip c at spans[c].off samples from d_x with spans[c].frames whole segments; n = the longest
    // clip of the pass, total = samples in the buffer)
    int run(int, const Config &cfg, const void *d_x, int in, long clips, int n, long stride, bool want_trace, hipStream_t st,
            const dsp::ClipSpan *spans, long total)
    {
        const dsp::IirCoef bp = coef_f32(3000, 7500), mp = coef_f32(1000, 3000);   // classifier.cpp:14-19, 438-442
        if (cfg.midpoint_db != keep_min_db) {      // the table's threshold PSD value follows the configured dB threshold
            // (earlier calls on this context are ordered before this one by its event)
            DSP_CAPI_HIP(dsp::launch_spec_threshold(d_tab, cfg.midpoint_db, st));
            keep_min_db = cfg.midpoint_db;
        }
        const dsp::ClassifyRule rule{cfg.keep_lo, cfg.keep_hi, cfg.middle_max, cfg.above_min, cfg.below_min};
        // ONE pass over the clips: both recurrences, the delay lines at every segment start, the 1000-3000 Hz segment means and
        // the energy gate.  No filtered signal is written; the spectrogram kernels recompute the segments they transform.
        DSP_CAPI_HIP(dsp::launch_iir2_ckpt(d_x, clips, n, stride, bp, mp, d_ck_bp, d_ck_mp, d_mean_mp, d_gate, d_tab, st, d_simd, in, spans, total));
        // midpoints first (1000-3000 Hz map, as flags, gated frames only); the 3000-7500 Hz spectrogram and its band sums only for
        // clips that have midpoints
        DSP_CAPI_HIP(dsp::launch_spec_from_ckpt(d_x, clips, n, stride, mp, d_ck_mp, d_mean_mp, d_gate, nullptr, d_tab,
                                                reinterpret_cast<float *>(d_loud.get()), true, st, nullptr, nullptr, in, spans));
        // DSP_AMD_CLASSIFY_FULL_MAPS=1: every row of the listed clips' maps is stored and read (no need / minmax hand-over)
        static const bool full_maps = [] { const char *e = std::getenv("DSP_AMD_CLASSIFY_FULL_MAPS"); return e && std::atoi(e) != 0; }();
        unsigned *mm = full_maps ? nullptr : d_minmax.get();
        const int *need = full_maps ? nullptr : d_loud.get();
        DSP_CAPI_HIP(dsp::launch_classify_midpoints(d_loud, clips, n, 16000, labels, trace, d_hits, st, want_trace, mm, spans));
        DSP_CAPI_HIP(dsp::launch_spec_from_ckpt(d_x, clips, n, stride, bp, d_ck_bp, nullptr, nullptr, d_hits, d_tab, d_sbp, false, st, need, mm, in, spans));
        DSP_CAPI_HIP(dsp::launch_classify_bands(d_sbp, clips, n, 16000, labels, trace, d_hits, st, rule, need, mm, spans));
        return DSP_OK;
    }
};
ClassifyCtx *const g_cls_ctx = front::workspaces<ClassifyCtx>();

}  // namespace

extern "C" {

int dsp_classify_division_check(long long *mismatches)
{
    int device = 0;
    int rc = front::host_device(device);
    if (rc < 0) return rc;
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    DSP_ON_DEVICE(device);
    if ((rc = front::open(g_cls, device)) < 0) return rc;
    unsigned long long bad = 0;
    int on = 0;
    hipError_t e = spec_div_mismatches(g_cls.d_tab, bad);
    if (e == hipSuccess) e = hipMemcpy(&on, reinterpret_cast<const char *>(g_cls.d_tab.get()) + offsetof(dsp::SpecTables, div_fast), sizeof(on), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
    if (mismatches) *mismatches = (long long)bad;
    return on ? 1 : 0;
}

int dsp_butter_bandpass_filter_f32(const float *data, long n_clips, int n, long stride, const float *b,
                                   const float *a, float *output)
{
    if (!data || !output || !b || !a || n_clips < 0 || n < 0 || (n_clips > 1 && stride < n)) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    if (n_clips == 0 || n == 0) return DSP_OK;
    int device = 0;
    int rc = front::host_device(device);
    if (rc < 0) return rc;
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    DSP_ON_DEVICE(device);
    if ((rc = front::open(g_cls, device)) < 0) return rc;
    dsp::DeviceBuf<float> dx, dy;
    const size_t bytes = (size_t)n_clips * n * sizeof(float);
    DSP_CAPI_HIP(dx.alloc(bytes));
    if (dy.alloc(bytes) != hipSuccess) return dsp::capi_fail(DSP_ENOMEM, "hipMalloc");
    dsp::IirCoef c;
    for (int i = 0; i < 9; ++i) { c.b[i] = b[i]; c.a[i] = a[i]; }
    hipError_t e = hipMemcpy2D(dx, (size_t)n * sizeof(float), data, (size_t)stride * sizeof(float), (size_t)n * sizeof(float), n_clips, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_iir_f32(dx, n_clips, n, n, c, dy, nullptr);
    if (e == hipSuccess) e = hipMemcpy2D(output, (size_t)stride * sizeof(float), dy, (size_t)n * sizeof(float), (size_t)n * sizeof(float), n_clips, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
    return DSP_OK;
}

int dsp_butter_bandpass_filter_f64(const double *data, long n_clips, int n, long stride, const double *b,
                                   const double *a, double *output)
{
    if (!data || !output || !b || !a || n_clips < 0 || n < 0 || (n_clips > 1 && stride < n)) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    if (n_clips == 0 || n == 0) return DSP_OK;
    int device = 0;
    int rc = front::host_device(device);
    if (rc < 0) return rc;
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    DSP_ON_DEVICE(device);
    if ((rc = front::open(g_cls, device)) < 0) return rc;
    dsp::DeviceBuf<double> dx, dy;
    const size_t bytes = (size_t)n_clips * n * sizeof(double);
    DSP_CAPI_HIP(dx.alloc(bytes));
    if (dy.alloc(bytes) != hipSuccess) return dsp::capi_fail(DSP_ENOMEM, "hipMalloc");
    dsp::IirCoefD c;
    for (int i = 0; i < 9; ++i) { c.b[i] = b[i]; c.a[i] = a[i]; }
    hipError_t e = hipMemcpy2D(dx, (size_t)n * sizeof(double), data, (size_t)stride * sizeof(double), (size_t)n * sizeof(double), n_clips, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_iir_f64(dx, n_clips, n, n, c, dy, nullptr);
    if (e == hipSuccess) e = hipMemcpy2D(output, (size_t)stride * sizeof(double), dy, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n_clips, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
    return DSP_OK;
}

int dsp_compute_spectrogram_f32(const float *signal, int n, int fs, float *frequencies, float *times, float *sxx)
{
    if (!signal || !sxx || n < 0 || fs <= 0) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    const int T = front::columns(n);
    if (frequencies)
        for (int k = 0; k < dsp::kSpecBins; ++k) frequencies[k] = (float)k * (float)fs / (float)dsp::kSpecSeg;   // classifier.cpp:248-251
    if (times)
        for (int t = 0; t < T; ++t) times[t] = ((float)(t * dsp::kSpecHop + dsp::kSpecSeg / 2)) / (float)fs;     // :254-258
    if (T == 0) return 0;
    int device = 0;
    int rc = front::host_device(device);
    if (rc < 0) return rc;
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    DSP_ON_DEVICE(device);
    if ((rc = front::open(g_cls, device)) < 0) return rc;
    dsp::DeviceBuf<float> dx, ds;
    dsp::DeviceBuf<dsp::SpecTables> dt;          // fs enters only through the PSD scale U = fs * sum w^2 (classifier.cpp:296-301)
    DSP_CAPI_HIP(dx.alloc((size_t)n * sizeof(float)));
    const size_t sb = (size_t)dsp::kSpecBins * T * sizeof(float);
    if (ds.alloc(sb) != hipSuccess) return dsp::capi_fail(DSP_ENOMEM, "hipMalloc");
    hipError_t e = hipSuccess;
    if (fs != 16000) {
        dsp::SpecTables t;
        dsp::build_spec_tables(fs, t);
        e = dsp::upload(dt, t);
    }
    if (e == hipSuccess) e = hipMemcpy(dx, signal, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_spectrogram_f32(dx, 1, n, n, dt ? dt.get() : g_cls.d_tab.get(), ds, nullptr);
    if (e == hipSuccess) e = hipMemcpy(sxx, ds, sb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
    return T;
}

int dsp_compute_spectrogram_f64(const double *signal, int n, int fs, double *frequencies, double *times, double *sxx)
{
    if (!signal || !sxx || n < 0 || fs <= 0) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    const int T = front::columns(n);
    if (frequencies)
        for (int k = 0; k < dsp::kSpecBins; ++k) frequencies[k] = (double)k * fs / dsp::kSpecSeg;                      // classifier.c:468-471
    if (times)
        for (int t = 0; t < T; ++t) times[t] = (double)(t * dsp::kSpecHop + dsp::kSpecSeg / 2) / fs;                    // :474-478
    if (T == 0) return 0;
    int device = 0;
    int rc = front::host_device(device);
    if (rc < 0) return rc;
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    DSP_ON_DEVICE(device);
    if ((rc = front::open(g_cls, device)) < 0) return rc;
    dsp::DeviceBuf<double> dx, ds;
    DSP_CAPI_HIP(dx.alloc((size_t)n * sizeof(double)));
    const size_t sb = (size_t)dsp::kSpecBins * T * sizeof(double);
    if (ds.alloc(sb) != hipSuccess) return dsp::capi_fail(DSP_ENOMEM, "hipMalloc");
    hipError_t e = hipMemcpy(dx, signal, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_spectrogram_f64(dx, 1, n, n, fs, ds, nullptr);
    if (e == hipSuccess) e = hipMemcpy(sxx, ds, sb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
    return T;
}

int dsp_sum_intense_f32(float lower, float upper, float half_range, const float *frequencies, int freq_bins,
                        const float *times, int time_bins, const float *db, float midpoint, float *out)
{
    if (!frequencies || !times || !db || !out || freq_bins <= 0 || time_bins <= 0) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    int device = 0;
    int rc = front::host_device(device);
    if (rc < 0) return rc;
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    DSP_ON_DEVICE(device);
    if ((rc = front::open(g_cls, device)) < 0) return rc;
    const size_t nf = freq_bins, nt = time_bins, total = nf + nt + nf * nt + 1;
    dsp::DeviceBuf<float> d;
    DSP_CAPI_HIP(d.alloc(total * sizeof(float)));
    hipError_t e = hipMemcpy(d, frequencies, nf * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + nf, times, nt * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + nf + nt, db, nf * nt * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_sum_intense(lower, upper, half_range, d, freq_bins, d + nf, time_bins, d + nf + nt, midpoint, d + nf + nt + nf * nt, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + nf + nt + nf * nt, sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dsp::capi_fail(DSP_EHIP, hipGetErrorString(e));
    return DSP_OK;
}

void dsp_classify_default_config(dsp_classify_config *cfg)
{
    if (cfg) *cfg = ClassifyCtx::default_config();
}

int dsp_classify_batch_host(const float *signal, long n_clips, int n, long stride, int *labels, dsp_classify_trace *trace)
{
    return front::host_entry<ClassifyCtx>(nullptr, signal, 0, n_clips, n, stride, labels, trace);
}

int dsp_classify_batch_host_cfg(const dsp_classify_config *cfgp, const float *signal, long n_clips, int n, long stride, int *labels,
                                dsp_classify_trace *trace)
{
    return front::host_entry<ClassifyCtx>(cfgp, signal, 0, n_clips, n, stride, labels, trace);
}

int dsp_classify_batch_pcm16_host(const dsp_classify_config *cfgp, const int16_t *pcm, long n_clips, int n, long stride, int channels, int stereo_mode,
                                  int *labels, dsp_classify_trace *trace)
{
    return front::host_entry<ClassifyCtx>(cfgp, pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, n, stride, labels, trace);
}

int dsp_classify_batch_device(const float *d_signal, long n_clips, int n, long stride, int *d_labels, void *stream)
{
    return front::device_entry<ClassifyCtx>(nullptr, d_signal, 0, n_clips, n, stride, d_labels, nullptr, stream);
}

int dsp_classify_batch_device_cfg(const dsp_classify_config *cfgp, const float *d_signal, long n_clips, int n, long stride,
                                  int *d_labels, void *stream)
{
    return front::device_entry<ClassifyCtx>(cfgp, d_signal, 0, n_clips, n, stride, d_labels, nullptr, stream);
}

int dsp_classify_batch_pcm16_device(const dsp_classify_config *cfgp, const int16_t *d_pcm, long n_clips, int n, long stride, int channels,
                                    int stereo_mode, int *d_labels, void *stream)
{
    return front::device_entry<ClassifyCtx>(cfgp, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, n, stride, d_labels, nullptr, stream);
}

int dsp_classify_batch_ragged_device(const dsp_classify_config *cfgp, const float *d_signal, long n_clips, const long *offsets, int *d_labels, void *stream)
{
    return front::ragged_device_entry<ClassifyCtx>(cfgp, d_signal, 0, n_clips, offsets, d_labels, nullptr, stream);
}

int dsp_classify_batch_ragged_pcm16_device(const dsp_classify_config *cfgp, const int16_t *d_pcm, long n_clips, const long *offsets, int channels,
                                           int stereo_mode, int *d_labels, void *stream)
{
    return front::ragged_device_entry<ClassifyCtx>(cfgp, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, d_labels, nullptr, stream);
}

int dsp_classify_batch_ragged_host(const dsp_classify_config *cfgp, const float *signal, long n_clips, const long *offsets, int *labels,
                                   dsp_classify_trace *trace)
{
    return front::ragged_host_entry<ClassifyCtx>(cfgp, signal, 0, n_clips, offsets, labels, trace);
}

int dsp_classify_batch_ragged_pcm16_host(const dsp_classify_config *cfgp, const int16_t *pcm, long n_clips, const long *offsets, int channels,
                                         int stereo_mode, int *labels, dsp_classify_trace *trace)
{
    return front::ragged_host_entry<ClassifyCtx>(cfgp, pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, labels, trace);
}

/* A context of the caller's own: the default entry points share one workspace per device, so two calls on one device run one behind
 * the other; calls through different contexts (on different streams) may overlap. */
struct dsp_classify_ctx { ClassifyCtx c; int device; };

void dsp_classify_ctx_destroy(dsp_classify_ctx *ctx)
{
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lock(ctx->c.mu);
        dsp::DeviceScope on(ctx->device);
        front::release(ctx->c);
    }
    delete ctx;
}

int dsp_classify_ctx_create(int device, dsp_classify_ctx **out)
{
    if (!out) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return dsp::capi_fail(DSP_ENODEV, "no HIP device: libdsp_amd has no CPU fallback");
    if (device < 0 || device >= n || device >= dsp::kMaxDevices) return dsp::capi_fail(DSP_EINVAL, "device index out of range");
    auto *ctx = new (std::nothrow) dsp_classify_ctx;
    if (!ctx) return dsp::capi_fail(DSP_ENOMEM, "out of memory");
    ctx->device = device;
    int rc;
    {
        std::lock_guard<std::mutex> lock(ctx->c.mu);
        dsp::DeviceScope on(device);
        if (on.err != hipSuccess) rc = dsp::capi_fail(DSP_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(on.err));
        else rc = front::open(ctx->c, device);
    }
    if (rc < 0) {
        dsp_classify_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return DSP_OK;
}

int dsp_classify_batch_device_ctx(dsp_classify_ctx *ctx, const dsp_classify_config *cfgp, const float *d_signal, long n_clips, int n, long stride,
                                  int *d_labels, void *stream)
{
    return ctx ? front::device_entry<ClassifyCtx>(cfgp, d_signal, 0, n_clips, n, stride, d_labels, nullptr, stream, &ctx->c)
               : dsp::capi_fail(DSP_EINVAL, "bad argument");
}

/* Test hook (no HIP call): holds the default classifier context of `device` for hold_ms milliseconds.  tests/test_capi_cpu.py runs it
 * from two threads: on two devices the holds overlap, on one device they queue. */
int dsp_debug_hold_classify_ctx(int device, int hold_ms)
{
    if (device < 0 || device >= dsp::kMaxDevices || hold_ms < 0 || hold_ms > 10000) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lock(g_cls_ctx[device].mu);
    std::this_thread::sleep_for(std::chrono::milliseconds(hold_ms));
    return DSP_OK;
}

int dsp_classify_stats(int device, long *gated_segments, long *listed_clips)
{
    if (device < 0 || device >= dsp::kMaxDevices) return dsp::capi_fail(DSP_EINVAL, "device index out of range");
    ClassifyCtx &g_cls = g_cls_ctx[device];
    std::lock_guard<std::mutex> lock(g_cls.mu);
    if (g_cls.device < 0 || !g_cls.d_gate) return dsp::capi_fail(DSP_EINVAL, "no classifier pass has run on this device");
    DSP_ON_DEVICE(device);
    g_cls.wait_idle();
    int ng = 0, nh = 0;
    DSP_CAPI_HIP(hipMemcpy(&ng, g_cls.d_gate, sizeof(int), hipMemcpyDeviceToHost));
    DSP_CAPI_HIP(hipMemcpy(&nh, g_cls.d_hits, sizeof(int), hipMemcpyDeviceToHost));
    if (gated_segments) *gated_segments = ng;
    if (listed_clips) *listed_clips = nh;
    return DSP_OK;
}

int dsp_classify_release(int device)
{
    return front::release_devices<ClassifyCtx>(device);
}

// sync/lib/classifier.h:18 (find_midpoints): the midpoints are a by-product of the classify pipeline (its trace record)
int dsp_find_midpoints(const float *data, int num_frames, int fs, float *midpoints, int max_midpoints)
{
    if (!data || num_frames <= 0 || max_midpoints < 0 || (max_midpoints > 0 && !midpoints)) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    if (fs != 16000) return dsp::capi_fail(DSP_EINVAL, "find_midpoints: only 16000 Hz has filter coefficients (classifier.cpp:138-191)");
    int label = 0;
    dsp_classify_trace tr;
    const int rc = dsp_classify_batch_host(data, 1, num_frames, num_frames, &label, &tr);
    if (rc < 0) return rc;
    for (int i = 0; i < tr.n_midpoints && i < max_midpoints; ++i) midpoints[i] = tr.midpoints[i];
    return tr.n_midpoints;
}

// sync/lib/classifier.h:19.  Same contract: 0/1, 0 also on failure (reason in dsp_last_error()).
int dsp_classify(float *data, int data_size)
{
    int label = 0;
    if (!data || data_size <= 0) { dsp::capi_fail(DSP_EINVAL, "bad argument"); return 0; }
    const int rc = dsp_classify_batch_host(data, 1, data_size, data_size, &label, nullptr);
    if (rc < 0) {
        std::fprintf(stderr, "libdsp_amd: classify: %s\n", dsp_last_error());
        return 0;
    }
    return label;
}

}  // extern "C"
