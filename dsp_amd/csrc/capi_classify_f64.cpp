// capi_classify_f64.cpp -- C ABI of the float64 classifier (include/dsp_amd.h: dsp_classify_batch_*_f64), the whole
// per-clip chain of donut-classifier/classifier.c:83-192 on the GPU in double:
//     butter_bandpass_filter (3000-7500 Hz and, inside find_midpoints, 1000-3000 Hz; :420-446)    iir2_screen_f64_kernel: both recurrences in one
//     compute_spectrogram of the 1000-3000 Hz output (:448-592) -> loud time bins (:679-745)       pass, restart states instead of filtered signals,
//                                                                                                  the loud bins by a bounded screening transform;
//                                                                                                  spec_f64_from_ckpt_kernel<flags> for the undecided
//     clusters -> midpoints (:747-800), work list of the clips that have any                       classify_f64_midpoints_kernel
//     compute_spectrogram of the 3000-7500 Hz output, listed clips only                            spec_f64_from_ckpt_kernel<maps>
//     dB map, normalisation, keep band, band sums, rule (:105-190, :594-653)                       classify_f64_bands_kernel
// Input: float64 samples or int16 PCM (mono / interleaved stereo, converted in the kernels' loads exactly like classifier.c:55-59, :286-297).
// The batch entries (uniform and ragged, host and device memory, float and int16 PCM) are classify_front.hpp's.
// Two yardstick pipelines for the tests (uniform float64 batches only; they materialise both filtered signals like round 3):
//     DSP_AMD_F64_PIPELINE=materialize   iir_kernel<double> x 2 -> spectrogram_f64_fft_kernel<flags / maps> (the same fft_frame)
//     DSP_AMD_F64_DFT=1                  ... -> the direct 256-point DFT ([129][T] maps) and the one-kernel tail
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <utility>

#include "classify_front.hpp"

static_assert(sizeof(dsp::ClassifyTraceD) == sizeof(dsp_classify_trace_f64), "trace layouts must match");

namespace {

namespace front = dsp::front;

long row_of(int n) { return ((long)n + 1) & ~1L; }      // yardstick row: n doubles rounded up to 16 bytes

enum Pipeline { kCkpt = 0, kMaterialize = 1, kDft = 2 };

void coefficients(dsp::IirCoefD &c_bp, dsp::IirCoefD &c_mp)
{
    double b[9], a[9];
    dsp_butter_bandpass(3000.0, 7500.0, b, a);                       // classifier.c:86-91
    for (int i = 0; i < 9; ++i) { c_bp.b[i] = b[i]; c_bp.a[i] = a[i]; }
    dsp_butter_bandpass(1000.0, 3000.0, b, a);                       // :659-664
    for (int i = 0; i < 9; ++i) { c_mp.b[i] = b[i]; c_mp.a[i] = a[i]; }
}

// per pass: `cap_clips` clips, `cap_cells` = clips x columns of the largest pass; allocated together, let go together (Scratch::reserve)
struct PassBufs {
    dsp::DeviceBuf<double> ck_bp, ck_mp, s_bp, mids;
    dsp::DeviceBuf<int> labels, loud, want, n_mids, hits;
    dsp::DeviceBuf<dsp::ClassifyTraceD> trace;
    dsp::DeviceBuf<unsigned long long> minmax;  // [clip][2]: smallest / largest positive cell of a listed clip's map (double bits)
    long cap_clips = 0;
    size_t cap_cells = 0;
};

// the yardstick pipelines' filtered signals (doubles per row) and second map; allocated together, let go together
struct YardstickBufs {
    dsp::DeviceBuf<double> y_bp, y_mp, s_mp;
    long cap_y_clips = 0, cap_y_row = 0;
    int cap_y_T = 0;
};

struct Scratch : front::Work, PassBufs, YardstickBufs {
    using Config = dsp_classify_config_f64;
    using Trace = dsp_classify_trace_f64;
    static constexpr int kFloatBytes = 8;

    dsp::DeviceBuf<dsp::SpecTablesD> tab;  // held = the workspace is initialised (init())
    dsp::DeviceBuf<dsp::ScreenTablesD> scr;
    dsp::DeviceBuf<int> cu_table;          // launch_iir2_screen_f64's per-CU arrival counters
    double U = 0.0;
    long last_segments = 0;                // clips x columns of the last pass (dsp_classify_stats_f64)

    static Config default_config()
    {
        // donut-classifier/classifier.c:141-142 (0.70 / 0.85), :660 (45 dB), :184 (75 / 300 / 100)
        return Config{0.70, 0.85, 45.0, 75.0, 300.0, 100.0};
    }
    static bool valid(const Config &c)
    {
        auto fin = [](double v) { return v == v && v - v == 0.0; };
        return fin(c.keep_lo) && fin(c.keep_hi) && fin(c.midpoint_db) && fin(c.middle_max) && fin(c.above_min) && fin(c.below_min) && c.keep_lo < c.keep_hi;
    }
    // the yardstick pipelines take uniform float64 batches only
    static int pipeline(int in, bool ragged)
    {
        if (ragged || in != 0) return kCkpt;
        const char *d = std::getenv("DSP_AMD_F64_DFT");
        if (d && std::atoi(d) != 0) return kDft;
        const char *p = std::getenv("DSP_AMD_F64_PIPELINE");
        return p && std::strcmp(p, "materialize") == 0 ? kMaterialize : kCkpt;
    }
    // DSP_AMD_F64_SUB_BATCH: a smaller pass (tests: a batch that spans passes).  A pass of the default pipeline is bounded by the
    // blocks of the screening kernel that are resident at once (3 per CU: 49 152 clips on 256 CUs).
    static long sub_batch(int pl)
    {
        const long cap = pl == kCkpt ? (long)dsp::f64_screen_blocks_per_pass() * 64 : 65536;
        const char *e = std::getenv("DSP_AMD_F64_SUB_BATCH");
        const long v = e ? std::atol(e) : 0;
        return v >= 64 ? std::min(v, cap) : cap;
    }

    int init()
    {
        if (tab) return DSP_OK;
        auto t = std::make_unique<dsp::SpecTablesD>();
        auto s = std::make_unique<dsp::ScreenTablesD>();
        dsp::build_spec_tables_f64(16000, *t);
        if (!dsp::build_screen_tables_f64(*t, 16000, *s)) return dsp::capi_fail(DSP_EINVAL, "screening tables: the window is not flat between its tapers");
        // built in locals and handed to the members after the last step that can fail: a failed init() leaves the workspace unopened
        dsp::DeviceBuf<dsp::SpecTablesD> new_tab;
        dsp::DeviceBuf<dsp::ScreenTablesD> new_scr;
        dsp::DeviceBuf<int> new_cu_table;
        DSP_CAPI_HIP(dsp::upload(new_tab, *t));
        DSP_CAPI_HIP(new_cu_table.alloc(sizeof(int) * (dsp::kSimdLoadCus + 16 * 4096)));      // (+ the diagnostic build's per-block records)
        DSP_CAPI_HIP(dsp::upload(new_scr, *s));
        tab = std::move(new_tab);
        scr = std::move(new_scr);
        cu_table = std::move(new_cu_table);
        U = t->U;
        return DSP_OK;
    }

    void free_pass() { static_cast<PassBufs &>(*this) = PassBufs{}; }
    void free_yardstick() { static_cast<YardstickBufs &>(*this) = YardstickBufs{}; }
    void free_all()
    {
        free_pass();
        free_yardstick();
        tab.reset();
        scr.reset();
        cu_table.reset();
    }

    // the workspace for passes of `clips` clips of n samples; grows, never shrinks
    int reserve(int pl, long clips, int n)
    {
        const size_t T = (size_t)front::columns(n);
        // (the per-segment arrays are sized by the PRODUCT clips x T of the largest pass: a ragged batch's pass of few long clips and its
        // pass of many short ones share them; by each dimension's maximum a single 13 s clip among 49 152 would ask for 72 GB)
        const size_t cells_needed = (size_t)clips * std::max<size_t>(T, 1);
        if (clips > cap_clips || cells_needed > cap_cells) {
            wait_idle();
            clips = std::max(clips, cap_clips);
            const size_t cells = std::max(cells_needed, cap_cells);
            free_pass();      // (the capacities stay 0 if an allocation below fails: the next call starts over)
            const size_t ck = cells * dsp::kCkPerSegF64 * 8 * sizeof(double);
            DSP_CAPI_HIP(ck_bp.alloc(ck));
            DSP_CAPI_HIP(ck_mp.alloc(ck));
            DSP_CAPI_HIP(s_bp.alloc(cells * dsp::kSpecBins * sizeof(double)));
            DSP_CAPI_HIP(mids.alloc((size_t)clips * dsp::kMaxMidpoints * sizeof(double)));
            DSP_CAPI_HIP(loud.alloc(cells * sizeof(int)));
            DSP_CAPI_HIP(want.alloc((cells + 1) * sizeof(int)));
            DSP_CAPI_HIP(n_mids.alloc((size_t)clips * sizeof(int)));
            DSP_CAPI_HIP(hits.alloc(((size_t)clips + 1) * sizeof(int)));
            DSP_CAPI_HIP(labels.alloc((size_t)clips * sizeof(int)));
            DSP_CAPI_HIP(trace.alloc((size_t)clips * sizeof(dsp::ClassifyTraceD)));
            DSP_CAPI_HIP(minmax.alloc((size_t)clips * 2 * sizeof(unsigned long long)));
            cap_clips = clips; cap_cells = cells;
        }
        if (pl != kCkpt && (clips > cap_y_clips || row_of(n) > cap_y_row || (int)T > cap_y_T)) {
            wait_idle();
            const long yc = std::max(clips, cap_y_clips), yr = std::max(row_of(n), cap_y_row);
            const size_t yT = std::max(T, (size_t)cap_y_T);
            free_yardstick();
            DSP_CAPI_HIP(y_bp.alloc((size_t)yc * yr * sizeof(double)));
            DSP_CAPI_HIP(y_mp.alloc((size_t)yc * yr * sizeof(double)));
            DSP_CAPI_HIP(s_mp.alloc((size_t)yc * dsp::kSpecBins * yT * sizeof(double)));
            cap_y_clips = yc; cap_y_row = yr; cap_y_T = (int)yT;
        }
        return DSP_OK;
    }

    // one sub-batch resident at d_x (row stride `stride` samples): labels (+ trace) into the workspace
    // spans != nullptr: a ragged sub-batch (clip c at spans[c].off samples from d_x; n = the longest clip of the pass, total = samples in the buffer)
    int run(int pl, const Config &cfg, const void *d_x, int in, long cnt, int n, long stride, bool want_trace, hipStream_t st,
            const dsp::ClipSpan *spans, long total)
    {
        dsp::IirCoefD c_bp, c_mp;
        coefficients(c_bp, c_mp);
        const dsp::ClassifyRuleD rule{cfg.keep_lo, cfg.keep_hi, cfg.midpoint_db, cfg.middle_max, cfg.above_min, cfg.below_min};
        dsp::ClassifyTraceD *tr = want_trace ? trace.get() : nullptr;
        last_segments = cnt * (long)front::columns(n);
        if (pl == kCkpt) {
            const double guard = dsp::f64_threshold_guard();
            DSP_CAPI_HIP(dsp::launch_iir2_screen_f64(d_x, in, cnt, n, stride, c_bp, c_mp, ck_bp, ck_mp, scr, U, cfg.midpoint_db, guard, loud, want, cu_table, st, spans, total));
            DSP_CAPI_HIP(dsp::launch_spec_f64_recheck(d_x, in, cnt, n, stride, c_mp, ck_mp, tab, want, cfg.midpoint_db, guard, loud, st, spans));
            DSP_CAPI_HIP(dsp::launch_classify_f64_midpoints(loud, cnt, n, 16000, mids, n_mids, hits, labels, tr, st, minmax, spans));
            DSP_CAPI_HIP(dsp::launch_spec_f64_listed_from_ckpt(d_x, in, cnt, n, stride, c_bp, ck_bp, tab, hits, s_bp, st, minmax, spans));
            DSP_CAPI_HIP(dsp::launch_classify_f64_bands(s_bp, hits, cnt, n, 16000, U, rule, mids, n_mids, labels, tr, st, minmax, spans));
            return DSP_OK;
        }
        const double *xd = static_cast<const double *>(d_x);
        const long row = cap_y_row;
        DSP_CAPI_HIP(dsp::launch_iir2_f64(xd, cnt, n, stride, row, c_bp, y_bp, c_mp, y_mp, st));
        if (pl == kDft) {                         // direct DFT, [129][T] maps of both outputs, one tail kernel per clip
            DSP_CAPI_HIP(dsp::launch_spectrogram_f64(y_bp, cnt, n, row, 16000, s_bp, st));
            DSP_CAPI_HIP(dsp::launch_spectrogram_f64(y_mp, cnt, n, row, 16000, s_mp, st));
            DSP_CAPI_HIP(dsp::launch_classify_f64_tail(s_bp, s_mp, cnt, n, 16000, rule, labels, tr, st));
            return DSP_OK;
        }
        DSP_CAPI_HIP(dsp::launch_spectrogram_f64_flags(y_mp, cnt, n, row, tab, cfg.midpoint_db, loud, st));
        DSP_CAPI_HIP(dsp::launch_classify_f64_midpoints(loud, cnt, n, 16000, mids, n_mids, hits, labels, tr, st));
        DSP_CAPI_HIP(dsp::launch_spectrogram_f64_listed(y_bp, cnt, n, row, tab, hits, s_bp, st));
        DSP_CAPI_HIP(dsp::launch_classify_f64_bands(s_bp, hits, cnt, n, 16000, U, rule, mids, n_mids, labels, tr, st));
        return DSP_OK;
    }
};
Scratch *const g_w = front::workspaces<Scratch>();

}  // namespace

extern "C" {

void dsp_classify_default_config_f64(dsp_classify_config_f64 *c)
{
    *c = Scratch::default_config();
}

int dsp_classify_batch_device_f64(const dsp_classify_config_f64 *cfgp, const double *d_signal, long n_clips, int n, long stride,
                                  int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream)
{
    return front::device_entry<Scratch>(cfgp, d_signal, 0, n_clips, n, stride, d_labels, d_trace, stream);
}

int dsp_classify_batch_host_f64(const dsp_classify_config_f64 *cfgp, const double *signal, long n_clips, int n, long stride,
                                int *labels, dsp_classify_trace_f64 *trace)
{
    return front::host_entry<Scratch>(cfgp, signal, 0, n_clips, n, stride, labels, trace);
}

int dsp_classify_batch_pcm16_device_f64(const dsp_classify_config_f64 *cfgp, const int16_t *d_pcm, long n_clips, int n, long stride, int channels,
                                        int stereo_mode, int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream)
{
    return front::device_entry<Scratch>(cfgp, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, n, stride, d_labels, d_trace, stream);
}

int dsp_classify_batch_pcm16_host_f64(const dsp_classify_config_f64 *cfgp, const int16_t *pcm, long n_clips, int n, long stride, int channels,
                                      int stereo_mode, int *labels, dsp_classify_trace_f64 *trace)
{
    return front::host_entry<Scratch>(cfgp, pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, n, stride, labels, trace);
}

int dsp_classify_batch_ragged_device_f64(const dsp_classify_config_f64 *cfgp, const double *d_signal, long n_clips, const long *offsets, int *d_labels,
                                         dsp_classify_trace_f64 *d_trace, void *stream)
{
    return front::ragged_device_entry<Scratch>(cfgp, d_signal, 0, n_clips, offsets, d_labels, d_trace, stream);
}

int dsp_classify_batch_ragged_pcm16_device_f64(const dsp_classify_config_f64 *cfgp, const int16_t *d_pcm, long n_clips, const long *offsets, int channels,
                                               int stereo_mode, int *d_labels, dsp_classify_trace_f64 *d_trace, void *stream)
{
    return front::ragged_device_entry<Scratch>(cfgp, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, d_labels, d_trace, stream);
}

int dsp_classify_batch_ragged_host_f64(const dsp_classify_config_f64 *cfgp, const double *signal, long n_clips, const long *offsets, int *labels,
                                       dsp_classify_trace_f64 *trace)
{
    return front::ragged_host_entry<Scratch>(cfgp, signal, 0, n_clips, offsets, labels, trace);
}

int dsp_classify_batch_ragged_pcm16_host_f64(const dsp_classify_config_f64 *cfgp, const int16_t *pcm, long n_clips, const long *offsets, int channels,
                                             int stereo_mode, int *labels, dsp_classify_trace_f64 *trace)
{
    return front::ragged_host_entry<Scratch>(cfgp, pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, labels, trace);
}

int dsp_classify_stats_f64(int device, long *segments, long *undecided, long *listed_clips)
{
    if (device < 0 || device >= dsp::kMaxDevices) return dsp::capi_fail(DSP_EINVAL, "device index out of range");
    Scratch &w = g_w[device];
    std::lock_guard<std::mutex> lock(w.mu);
    if (w.device < 0 || !w.want) return dsp::capi_fail(DSP_EINVAL, "no float64 classifier pass has run on this device");
    DSP_ON_DEVICE(device);
    w.wait_idle();
    int nw = 0, nh = 0;
    DSP_CAPI_HIP(hipMemcpy(&nw, w.want, sizeof(int), hipMemcpyDeviceToHost));
    DSP_CAPI_HIP(hipMemcpy(&nh, w.hits, sizeof(int), hipMemcpyDeviceToHost));
    if (segments) *segments = w.last_segments;
    if (undecided) *undecided = nw;
    if (listed_clips) *listed_clips = nh;
    return DSP_OK;
}

int dsp_classify_debug_f64(int device, int *out, int n_ints)      /* diagnostic builds: the screening kernel's per-block records */
{
    if (device < 0 || device >= dsp::kMaxDevices || !out || n_ints < 0 || n_ints > 16 * 4096) return dsp::capi_fail(DSP_EINVAL, "bad argument");
    Scratch &w = g_w[device];
    std::lock_guard<std::mutex> lock(w.mu);
    if (!w.cu_table) return dsp::capi_fail(DSP_EINVAL, "no pass has run");
    DSP_ON_DEVICE(device);
    w.wait_idle();
    DSP_CAPI_HIP(hipMemcpy(out, w.cu_table + dsp::kSimdLoadCus, sizeof(int) * (size_t)n_ints, hipMemcpyDeviceToHost));
    return DSP_OK;
}

int dsp_classify_release_f64(int device)
{
    return front::release_devices<Scratch>(device);
}

}  // extern "C"
