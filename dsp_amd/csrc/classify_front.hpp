// classify_front.hpp -- the batch front end of both donut classifiers (capi_classify_f32.cpp: sync/lib/classifier.cpp in float,
// capi_classify_f64.cpp: donut-classifier/classifier.c in double): argument checks, the device an entry runs on, the per-device
// workspaces and their lock / event policy, the sub-batch loops of the uniform entries and the whole ragged path.  The two host
// entries make their checks, describe the batch by a layout (host_chunks.hpp) and hand it with their pass to host::Session
// (host_pipe.hpp), which plans, stages and copies; the number of devices (kMaxDevices) is capi_util.hpp's.
// A precision supplies a workspace type W (derived from front::Work) that carries its kernels:
//     Config, Trace                   the public config and trace record types
//     default_config(), valid(cfg)    the reference's thresholds, and whether a config is usable
//     kFloatBytes                     bytes of one float sample
//     pipeline(in, ragged)            which kernel chain a call runs (the float64 yardsticks: uniform float batches only)
//     sub_batch(pl)                   clips per pass through the workspace
//     init()                          tables, once per workspace (the caller holds mu and has made the device current)
//     reserve(pl, clips, n)           the workspace of a pass of `clips` clips of n samples; grows only (host batches are staged by the
//                                     device's host pipeline, host_pipe.hpp, not by the workspace)
//     run(pl, cfg, d_x, in, clips, n, stride, want_trace, st, spans, total)    one pass: labels (+ trace) into `labels` / `trace`
//     free_all()                      lets every device buffer of the workspace go
// Input kinds `in`: 0 float samples, 1 / 2 / 3 int16 mono / interleaved stereo channel 0 / stereo average.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "capi_util.hpp"
#include "classify_kernels.hpp"
#include "host_pipe.hpp"

namespace dsp {
namespace front {

// 957 columns = 13.4 s: a midpoint needs a cluster of >= 12 columns (0.15 s at 14 ms per column) followed by a gap of >= 4
// (0.05 s), so 64 * 15 - 3 columns cannot hold more than the kMaxMidpoints = 64 a trace record has room for
constexpr int kMaxColumns = 957;

inline int columns(int n) { return n < kSpecSeg ? 0 : (n - kSpecSeg) / kSpecHop + 1; }

template <class W> int sample_bytes(int in) { return in == 0 ? W::kFloatBytes : in == 1 ? 2 : 4; }     // all channels

// One workspace PER DEVICE (grow-only until released), its own mutex: threads that drive different GPUs share nothing.  A call
// enqueues on the caller's stream and returns; the next call on that workspace first makes its stream wait for the event this one
// leaves behind.
struct Work {
    std::mutex mu;
    int device = -1;                       // -1: nothing allocated
    hipEvent_t done = nullptr;             // recorded behind the last call's work: the workspace is free once it has fired
    bool pending = false;
    SpanRing spans;                        // ragged batches: the clips' spans on their way to the GPU (capi_util.hpp)
    void wait_idle()
    {
        if (pending && done) (void)hipEventSynchronize(done);
        pending = false;
    }
};
// Immortal: allocated at first use and never deleted, so that no destructor calls into HIP at process exit (or at interpreter
// shutdown, under ctypes beside torch), when the runtime may already be gone.  dsp_classify_release* return the memory.
template <class W> W *workspaces()
{
    static W *const all = new W[kMaxDevices];
    return all;
}

// leaves the "workspace busy until here" event behind the call's work on EVERY exit, so that a failed call cannot hand a workspace
// with kernels still running on it to the next one
struct BusyMark {
    Work &w;
    hipStream_t st;
    ~BusyMark()
    {
        if (w.done && hipEventRecord(w.done, st) == hipSuccess) w.pending = true;
        else { (void)hipGetLastError(); (void)hipStreamSynchronize(st); w.pending = false; }
    }
};

// the caller holds w.mu and has made `device` current
template <class W> int open(W &w, int device)
{
    w.device = device;
    if (!w.done) DSP_CAPI_HIP(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    return w.init();
}

template <class W> void release(W &w)      // on w.device, made current by the caller, under w.mu
{
    w.wait_idle();
    w.free_all();
    if (w.done) (void)hipEventDestroy(w.done);
    w.done = nullptr;
    w.spans.release();
    w.device = -1;
}

template <class W> int release_devices(int device)      // device < 0: all of them
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); count = 0; }
    for (int d = 0; d < kMaxDevices && d < count; ++d) {
        if (device >= 0 && d != device) continue;
        W &w = workspaces<W>()[d];
        std::lock_guard<std::mutex> lock(w.mu);
        if (w.device < 0) continue;
        DSP_ON_DEVICE(d);
        release(w);
    }
    return DSP_OK;
}

// the device of the host entries: DSP_AMD_DEVICE or 0
inline int host_device(int &device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return capi_fail(DSP_ENODEV, "no HIP device: libdsp_amd has no CPU fallback");
    const char *dev = std::getenv("DSP_AMD_DEVICE");
    device = dev ? std::atoi(dev) : 0;
    if (device < 0 || device >= n || device >= kMaxDevices) return capi_fail(DSP_EINVAL, "device index out of range");
    return DSP_OK;
}

// the device of the device-pointer entries: the one that owns the signal
inline int pointer_device(const void *d_signal, int &device)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_signal) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return capi_fail(DSP_EINVAL, "signal is not a device pointer");
    }
    if (attr.device < 0 || attr.device >= kMaxDevices) return capi_fail(DSP_EINVAL, "device index out of range");
    device = attr.device;
    return DSP_OK;
}

template <class W> int config(const typename W::Config *cfgp, typename W::Config &cfg)
{
    cfg = cfgp ? *cfgp : W::default_config();
    if (!W::valid(cfg)) return capi_fail(DSP_EINVAL, "classify config: thresholds must be finite with keep_lo < keep_hi");
    return DSP_OK;
}

template <class W> int check_uniform(const typename W::Config *cfgp, const void *signal, long n_clips, int n, long stride, const int *labels,
                                     typename W::Config &cfg)
{
    if (!signal || !labels || n_clips < 0 || n < 0 || (n_clips > 1 && stride < n)) return capi_fail(DSP_EINVAL, "bad argument");
    const int rc = config<W>(cfgp, cfg);
    if (rc < 0) return rc;
    if (columns(n) > kMaxColumns) return capi_fail(DSP_EINVAL, "clip too long (more than 957 spectrogram columns = 13.4 s at 16 kHz)");
    return DSP_OK;
}

// equal clips on the GPU: d_signal [n_clips][stride] of kind `in`.  own: a context of the caller's (dsp_classify_batch_device_ctx)
// instead of the device's workspace.
template <class W> int device_entry(const typename W::Config *cfgp, const void *d_signal, int in, long n_clips, int n, long stride, int *d_labels,
                                    typename W::Trace *d_trace, void *stream, W *own = nullptr)
{
    if (in < 0) return in;
    typename W::Config cfg;
    int rc = check_uniform<W>(cfgp, d_signal, n_clips, n, stride, d_labels, cfg);
    if (rc < 0 || n_clips == 0) return rc;
    int device = 0;
    if ((rc = pointer_device(d_signal, device)) < 0) return rc;
    if (own && own->device >= 0 && own->device != device) return capi_fail(DSP_EINVAL, "the context belongs to another device than the signal");
    DSP_ON_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (columns(n) == 0) {                   // shorter than one spectrogram segment: no midpoints, label 0
        DSP_CAPI_HIP(hipMemsetAsync(d_labels, 0, (size_t)n_clips * sizeof(int), st));
        if (d_trace) DSP_CAPI_HIP(hipMemsetAsync(d_trace, 0, (size_t)n_clips * sizeof(*d_trace), st));
        return DSP_OK;
    }
    if (n_clips == 1) stride = n;
    W &w = own ? *own : workspaces<W>()[device];
    std::lock_guard<std::mutex> lock(w.mu);
    if ((rc = open(w, device)) < 0) return rc;
    const int pl = W::pipeline(in, false);
    const long sub = W::sub_batch(pl);
    if ((rc = w.reserve(pl, std::min(sub, n_clips), n)) < 0) return rc;
    if (w.pending) DSP_CAPI_HIP(hipStreamWaitEvent(st, w.done, 0));        // the previous call's work on this workspace (any stream)
    BusyMark mark{w, st};
    for (long c0 = 0; c0 < n_clips; c0 += sub) {
        const long cnt = std::min(sub, n_clips - c0);
        const void *src = static_cast<const unsigned char *>(d_signal) + (size_t)c0 * stride * sample_bytes<W>(in);
        if ((rc = w.run(pl, cfg, src, in, cnt, n, stride, d_trace != nullptr, st, nullptr, 0)) < 0) return rc;
        DSP_CAPI_HIP(hipMemcpyAsync(d_labels + c0, w.labels, (size_t)cnt * sizeof(int), hipMemcpyDeviceToDevice, st));
        if (d_trace) DSP_CAPI_HIP(hipMemcpyAsync(d_trace + c0, w.trace, (size_t)cnt * sizeof(*d_trace), hipMemcpyDeviceToDevice, st));
    }
    return DSP_OK;
}

// equal clips in host memory: through the device's host pipeline (host_pipe.hpp) a chunk at a time, a chunk being one pass through the
// workspace.  The pipeline owns the staged input and the results' way home; the workspace is sized for one chunk's clips.
template <class W> int host_entry(const typename W::Config *cfgp, const void *signal, int in, long n_clips, int n, long stride, int *labels,
                                  typename W::Trace *trace)
{
    if (in < 0) return in;
    typename W::Config cfg;
    int rc = check_uniform<W>(cfgp, signal, n_clips, n, stride, labels, cfg);
    if (rc < 0 || n_clips == 0) return rc;
    if (columns(n) == 0) {                   // clips shorter than one segment cannot fire the rule
        std::fill(labels, labels + n_clips, 0);
        if (trace) std::memset(trace, 0, (size_t)n_clips * sizeof(*trace));
        return DSP_OK;
    }
    int device = 0;
    if ((rc = host_device(device)) < 0) return rc;
    DSP_ON_DEVICE(device);
    if (n_clips == 1) stride = n;
    W &w = workspaces<W>()[device];
    std::lock_guard<std::mutex> lock(w.mu);                                     // (the workspace's lock, then the pipeline's)
    if ((rc = open(w, device)) < 0) return rc;
    const int pl = W::pipeline(in, false);
    const size_t bps = (size_t)sample_bytes<W>(in);
    const size_t row = (((size_t)n * bps + 15) & ~(size_t)15) / bps;            // staged rows start on 16 bytes
    host::UniformLayout l{n_clips, (size_t)stride * bps, row * bps, (size_t)n * bps, true};
    // (a chunk is a pass: at least cfg.classify_min_clips clips, at most the workspace's sub-batch)
    host::Session hs;
    if ((rc = hs.open(device, signal, l, {(long)(row * bps), W::sub_batch(pl)})) < 0) return rc;
    if ((rc = w.reserve(pl, l.first[1], n)) < 0) return rc;
    w.wait_idle();
    BusyMark mark{w, nullptr};                                                  // (the kernels of every chunk run on the null stream)
    const bool one = hs.n_chunks(l) == 1;
    host::Outs outs{{labels, trace}, {sizeof(int), sizeof(*trace)}};
    if (one) { outs.resident[0] = w.labels; outs.resident[1] = w.trace; }
    return hs.run(signal, l, outs, [&](long k, const void *d_x, void *const *d_out, hipStream_t st) {
        const long cnt = (long)l.rows(k);
        const int r = w.run(pl, cfg, d_x, in, cnt, n, (long)row, trace != nullptr, st, nullptr, 0);
        if (r < 0 || one) return r;               // (one chunk: the results go home from the workspace, outs.resident)
        DSP_CAPI_HIP(hipMemcpyAsync(d_out[0], w.labels, (size_t)cnt * sizeof(int), hipMemcpyDeviceToDevice, st));
        if (trace) DSP_CAPI_HIP(hipMemcpyAsync(d_out[1], w.trace, (size_t)cnt * sizeof(*trace), hipMemcpyDeviceToDevice, st));
        return (int)DSP_OK;
    });
}

// every clip of a ragged batch, device and host form alike: its length is one (ragged_clip_length) and it has room in a trace record;
// n_max: the longest clip's samples
inline int check_ragged_clips(const long *offsets, long n_clips, int &n_max)
{
    n_max = 0;
    for (long c = 0; c < n_clips; ++c) {
        const long n = ragged_clip_length(offsets, c);
        if (n < 0) return (int)n;
        if (columns((int)n) > kMaxColumns) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + " too long (more than 957 spectrogram columns = 13.4 s at 16 kHz)");
        n_max = std::max(n_max, (int)n);
    }
    return DSP_OK;
}

// Ragged batches (the references read one file of any length per run; their callers loop over files): the clips' spans from the
// host's offsets[n_clips + 1] (samples per channel from the buffer's start), every clip with the segments ITS length holds.
// d_signal: the whole buffer on `device`.  Results to d_labels / d_trace (device) and labels / trace (host), whichever are given.
// locked: the caller holds the workspace's lock (the host entry, which takes the host pipeline's behind it)
template <class W> int ragged(const typename W::Config &cfg, const void *d_signal, int device, int in, long n_clips, const long *offsets,
                              int *d_labels, typename W::Trace *d_trace, int *labels, typename W::Trace *trace, void *stream, bool locked = false)
{
    int rc = DSP_OK, n_max = 0;
    if ((rc = check_ragged_clips(offsets, n_clips, n_max)) < 0) return rc;
    DSP_ON_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (columns(n_max) == 0) {                 // no clip holds a segment: no midpoints, label 0
        if (d_labels) DSP_CAPI_HIP(hipMemsetAsync(d_labels, 0, (size_t)n_clips * sizeof(int), st));
        if (d_trace) DSP_CAPI_HIP(hipMemsetAsync(d_trace, 0, (size_t)n_clips * sizeof(*d_trace), st));
        if (labels) std::fill(labels, labels + n_clips, 0);
        if (trace) std::memset(trace, 0, (size_t)n_clips * sizeof(*trace));
        return DSP_OK;
    }
    if (n_clips >= (1L << 31)) return capi_fail(DSP_EINVAL, "too many clips");
    W &w = workspaces<W>()[device];
    std::unique_lock<std::mutex> lock(w.mu, std::defer_lock);
    if (!locked) lock.lock();
    if ((rc = open(w, device)) < 0) return rc;
    const int pl = W::pipeline(in, true);
    const long sub = W::sub_batch(pl);
    // The clips run in order of length, longest first: the kernels take 64 clips per block and walk to the block's longest, so a block of
    // alike clips wastes nothing (measured on clips of 0.5 - 1.5 s in the caller's order: +54 % over the same samples in equal clips).
    // order[i] = the caller's index of the i-th clip as run; results go home through it (launch_scatter_records / on the host).
    std::vector<int> order((size_t)n_clips), segs((size_t)n_clips);
    for (long c = 0; c < n_clips; ++c) segs[c] = columns((int)(offsets[c + 1] - offsets[c]));
    order_by_key_desc(segs.data(), n_clips, columns(n_max), order.data());
    const size_t span_bytes = (size_t)n_clips * sizeof(ClipSpan), perm_bytes = (size_t)n_clips * sizeof(int);
    SpanRing::Lease slot;
    DSP_CAPI_HIP(w.spans.acquire(span_bytes + perm_bytes, slot));
    ClipSpan *h = static_cast<ClipSpan *>(slot.h());
    for (long i = 0; i < n_clips; ++i) {
        const long c = order[i];
        h[i] = ClipSpan{offsets[c], (int)(offsets[c + 1] - offsets[c]), segs[c], c, 0};
    }
    std::memcpy(static_cast<char *>(slot.h()) + span_bytes, order.data(), perm_bytes);
    if (w.pending) DSP_CAPI_HIP(hipStreamWaitEvent(st, w.done, 0));         // the previous call's work on this workspace (any stream)
    DSP_CAPI_HIP(slot.upload(span_bytes + perm_bytes, st));
    BusyMark mark{w, st};
    const ClipSpan *d_spans = static_cast<const ClipSpan *>(slot.d());
    const int *d_perm = reinterpret_cast<const int *>(static_cast<const char *>(slot.d()) + span_bytes);
    // Passes: as many clips as a pass of equal 1 s clips has SEGMENTS for (the workspaces are [clip][segments of the pass's longest clip]):
    // few clips per pass while they are long, the full sub-batch once they are short
    // (four times that before a pass is cut short: a small remainder pass costs a whole clip's sequential chain for few clips -- 0.5 - 1.5 s
    // clips in two passes measured 3.6 ms against 3.1 ms in one; the bound is there for batches with very long clips, ~11 GB of workspace)
    const long pass_segs = 4 * sub * 71;
    struct Pass { long c0, cnt; int n_row; };
    std::vector<Pass> passes;
    for (long c0 = 0; c0 < n_clips;) {
        const int t_row = std::max(1, h[c0].frames);                            // sorted: the pass's longest clip comes first
        const long cnt = std::min({sub, n_clips - c0, std::max(64L, pass_segs / t_row)});
        passes.push_back(Pass{c0, cnt, (t_row - 1) * kSpecHop + kSpecSeg});
        c0 += cnt;
    }
    for (const Pass &ps : passes)
        if ((rc = w.reserve(pl, ps.cnt, ps.n_row)) < 0) return rc;
    const bool want_trace = d_trace || trace;
    std::vector<int> h_labels;
    std::vector<typename W::Trace> h_trace;
    for (const Pass &ps : passes) {
        const long c0 = ps.c0, cnt = ps.cnt;
        if ((rc = w.run(pl, cfg, d_signal, in, cnt, ps.n_row, 0, want_trace, st, d_spans + c0, offsets[n_clips])) < 0) return rc;
        if (d_labels) DSP_CAPI_HIP(launch_scatter_records(w.labels, d_perm + c0, cnt, sizeof(int), d_labels, st));
        if (d_trace) DSP_CAPI_HIP(launch_scatter_records(w.trace, d_perm + c0, cnt, sizeof(*d_trace), d_trace, st));
        if (!labels && !trace) continue;
        if (labels) {
            h_labels.resize((size_t)cnt);
            DSP_CAPI_HIP(hipMemcpyAsync(h_labels.data(), w.labels, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, st));
        }
        if (trace) {
            h_trace.resize((size_t)cnt);
            DSP_CAPI_HIP(hipMemcpyAsync(h_trace.data(), w.trace, (size_t)cnt * sizeof(*trace), hipMemcpyDeviceToHost, st));
        }
        DSP_CAPI_HIP(hipStreamSynchronize(st));
        for (long i = 0; i < cnt; ++i) {
            if (labels) labels[order[c0 + i]] = h_labels[i];
            if (trace) trace[order[c0 + i]] = h_trace[i];
        }
    }
    return DSP_OK;
}

template <class W> int ragged_device_entry(const typename W::Config *cfgp, const void *d_signal, int in, long n_clips, const long *offsets,
                                           int *d_labels, typename W::Trace *d_trace, void *stream)
{
    if (in < 0) return in;
    if (!d_signal || !d_labels || !offsets || n_clips < 0) return capi_fail(DSP_EINVAL, "bad argument");
    typename W::Config cfg;
    int rc = config<W>(cfgp, cfg);
    if (rc < 0 || n_clips == 0) return rc;
    int device = 0;
    if ((rc = pointer_device(d_signal, device)) < 0) return rc;
    return ragged<W>(cfg, d_signal, device, in, n_clips, offsets, d_labels, d_trace, nullptr, nullptr, stream);
}

template <class W> int ragged_host_entry(const typename W::Config *cfgp, const void *signal, int in, long n_clips, const long *offsets, int *labels,
                                         typename W::Trace *trace)
{
    if (in < 0) return in;
    if (!signal || !labels || !offsets || n_clips < 0) return capi_fail(DSP_EINVAL, "bad argument");
    typename W::Config cfg;
    int rc = config<W>(cfgp, cfg);
    if (rc < 0 || n_clips == 0) return rc;
    if (offsets[n_clips] < offsets[0] || offsets[0] < 0) return capi_fail(DSP_EINVAL, "offsets must be non-negative and non-decreasing, clips shorter than 2^31 samples");
    int device = 0;
    if ((rc = host_device(device)) < 0) return rc;
    // chunks of whole clips (host_chunks.hpp), each one ragged device pass over its own samples with the offsets rebased: every clip gets
    // the label and trace of a one-clip call, so the cuts are invisible.  The results go home in the caller's order (the pass scatters
    // them into the pipeline's staging as it does into a device caller's arrays).
    int n_max = 0;
    if ((rc = check_ragged_clips(offsets, n_clips, n_max)) < 0) return rc;
    DSP_ON_DEVICE(device);
    W &w = workspaces<W>()[device];
    std::lock_guard<std::mutex> lock(w.mu);                                     // (the workspace's lock, then the pipeline's)
    const size_t bps = (size_t)sample_bytes<W>(in);
    host::RaggedLayout l{offsets, n_clips, bps};
    // (at least the bytes of classify_min_clips clips of one second a chunk)
    host::Session hs;
    if ((rc = hs.open(device, signal, l, {16000L * (long)bps, 0})) < 0) return rc;
    std::vector<long> rebased;
    if (hs.n_chunks(l) == 1) {
        // one chunk: the whole buffer travels once and the batch is one ragged pass that brings its results home itself, pass by pass,
        // in the caller's order -- the launches of a device call on the same samples and nothing else
        void *d_flat = nullptr;
        if ((rc = hs.pipe->stage_whole(static_cast<const char *>(signal) + l.base_offset(), l.extent(), d_flat)) < 0) return rc;
        l.rebase(0, rebased);
        rc = ragged<W>(cfg, d_flat, device, in, n_clips, rebased.data(), nullptr, nullptr, labels, trace, nullptr, true);
        (void)hipStreamSynchronize(nullptr);      // the pass's kernels read the staged buffer: they end before the lock is let go
        hs.pipe->last.bytes_d2h = (long)((size_t)n_clips * (sizeof(int) + (trace ? sizeof(*trace) : 0)));
        return rc;
    }
    return hs.run(signal, l, host::Outs{{labels, trace}, {sizeof(int), sizeof(*trace)}}, [&](long k, const void *d_x, void *const *d_out, hipStream_t st) {
        l.rebase(k, rebased);
        return ragged<W>(cfg, d_x, device, in, (long)rebased.size() - 1, rebased.data(), static_cast<int *>(d_out[0]),
                         trace ? static_cast<typename W::Trace *>(d_out[1]) : nullptr, nullptr, nullptr, st, true);
    });
}

}  // namespace front
}  // namespace dsp
