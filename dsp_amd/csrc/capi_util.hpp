// capi_util.hpp -- error reporting, device scopes, the owners of device and pinned host buffers (DeviceBuf, PinnedBuf), the
// ragged-span ring (which frees itself), the scans' host planner, the handles' base with their one create and one destroy path (Handle,
// create_on_device / create_on_host, destroy; the score-matrix stages' StageHandle), the float UBM of a handle and the number of devices that have state of their own
// (kMaxDevices), shared by the translation units of the C ABI (capi.cpp, capi_scrubjay.cpp, capi_consumers.cpp, capi_stream.cpp, capi_gather.cpp, and the
// classifiers' front end classify_front.hpp).  Nothing here knows a plan: what reads one is mfcc_plan.hpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dsp_amd.h"
#include "gmm_model.hpp"

namespace dsp {
int capi_fail(int code, const std::string &msg);   // sets dsp_last_error() for this thread, returns code

// the devices that have a classifier workspace (classify_front.hpp) and a host pipeline (host_pipe.hpp) of their own
constexpr int kMaxDevices = 64;

// The owner of one buffer of the runtime's and of its size: whoever holds it frees it, once, on destruction or reset().  Move-only.
// DeviceBuf<T> is hipMalloc'ed, PinnedBuf page-locked host memory (hipHostMalloc); these two and the public allocator of
// capi_host.cpp are the only callers of the runtime's allocation functions in the host code.
// Its holder makes the buffer's device current before the buffer is let go (a handle's: dsp::destroy and the create helpers, below), and no object of
// static storage holds one: at process exit the HIP runtime may already be gone.
template <class T, bool kPinned> class OwnedBuf {
    T *p = nullptr;
    size_t cap = 0;
public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~OwnedBuf() { reset(); }
    void reset()
    {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    // exactly `bytes`, in place of what was held; empty on an error
    hipError_t alloc(size_t bytes)
    {
        reset();
        void *q = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e == hipSuccess) { p = static_cast<T *>(q); cap = bytes; }
        return e;
    }
    // a grow-only workspace: at least `bytes` afterwards (its contents are not kept), or empty on an error
    hipError_t reserve(size_t bytes) { return cap >= bytes ? hipSuccess : alloc(bytes); }
    T *get() const { return p; }
    operator T *() const { return p; }
    size_t bytes() const { return cap; }
};
template <class T> using DeviceBuf = OwnedBuf<T, false>;
using PinnedBuf = OwnedBuf<char, true>;

// a new buffer holding a copy of the host's object
template <class T> hipError_t upload(DeviceBuf<T> &buf, const T &host)
{
    const hipError_t e = buf.alloc(sizeof(T));
    return e == hipSuccess ? hipMemcpy(buf, &host, sizeof(T), hipMemcpyHostToDevice) : e;
}
}

// Ragged batches: the clips' spans (clip_span.hpp ClipSpan: start, samples, frames, caller's index -- 32 bytes per clip) travel to the GPU through a
// small ring of pinned host / device buffer pairs, so that a call neither waits for the stream it enqueues on nor shares a buffer with
// the call before it (which may still be running, on this stream or another).  A call holds its slot as a Lease: fill h(), upload(),
// enqueue the kernels that read d(), and the lease's end -- on every exit -- records the slot's event behind them on the upload's stream
// and hands the slot back.  A slot is reused only after that event.  An acquirer takes the next slot that is neither leased nor waiting
// for its event; where there is none the ring GROWS by a slot (kSlots to start with, kMaxSlots at most), because waiting for the event
// would be waiting for the caller's stream: a caller that enqueues several calls behind a producer that has not finished -- an
// augmentation takes four leases, a chain of pushes one each -- would find the host blocked in the fifth.  Only a ring of kMaxSlots
// slots, all in flight, makes an acquirer wait: for the lease of the slot whose turn it is to end, then for its event.
// Deadlock-free because no call holds two leases of one ring at once (each user takes one lease, launches, and lets it go before
// it could ask the ring again), and no one waits for a lease while holding a lock a lease holder takes.
// A ring frees itself: its destructor does what release() does (events, then the slots' buffers), so like an OwnedBuf it is destroyed
// with its owner's device current and no object of static storage holds one.  Its holders are the handles below (Handle: on the heap,
// destroyed by dsp::destroy), the default plan of capi.cpp (a pointer that is never deleted) and the classifiers' workspaces
// (classify_front.hpp: the per-device array is allocated immortal; a context's ring is emptied by front::release before the context
// is deleted).
namespace dsp {
struct ClipSpan;
struct SpanRing {
    static constexpr int kSlots = 4, kMaxSlots = 32;
    struct Slot { PinnedBuf h; DeviceBuf<char> d; hipEvent_t done = nullptr; bool used = false, held = false; };      // (h and d of one size)
    class Lease {
        friend struct SpanRing;
        SpanRing *ring = nullptr;
        Slot *s = nullptr;
        hipStream_t st = nullptr;
        bool uploaded = false;
    public:
        Lease() = default;
        Lease(const Lease &) = delete;
        Lease &operator=(const Lease &) = delete;
        ~Lease()
        {
            if (!s) return;
            if (uploaded) { s->used = hipEventRecord(s->done, st) == hipSuccess; if (!s->used) (void)hipStreamSynchronize(st); }
            std::lock_guard<std::mutex> lock(ring->mu);
            s->held = false;
            ring->freed.notify_all();
        }
        void *h() const { return s->h.get(); }
        void *d() const { return s->d.get(); }
        hipError_t upload(size_t bytes, hipStream_t stream)
        {
            st = stream;
            uploaded = true;
            return hipMemcpyAsync(s->d.get(), s->h.get(), bytes, hipMemcpyHostToDevice, stream);
        }
    };
    std::vector<std::unique_ptr<Slot>> slots;      // (their addresses stay put as the ring grows: leases point at them)
    int next = 0;
    std::mutex mu;
    std::condition_variable freed;
    // `out` (empty) leases a slot with room for `bytes` whose previous user has finished
    hipError_t acquire(size_t bytes, Lease &out)
    {
        Slot *sp = nullptr;
        {
            std::unique_lock<std::mutex> lock(mu);
            while ((int)slots.size() < kSlots) slots.emplace_back(new Slot);
            const int n = (int)slots.size();
            for (int i = 0; i < n && !sp; ++i) {      // from the slot whose turn it is: the first that is free and whose upload has been read
                Slot *c = slots[(size_t)((next + i) % n)].get();
                if (!c->held && (!c->used || hipEventQuery(c->done) == hipSuccess)) {
                    sp = c;
                    next = (next + i + 1) % n;
                }
            }
            if (!sp && n < kMaxSlots) {               // every slot is in flight: one more, instead of a wait for the caller's stream
                slots.emplace_back(new Slot);
                sp = slots.back().get();
                next = 0;
            }
            if (!sp) {
                sp = slots[(size_t)next].get();
                next = (next + 1) % n;
                freed.wait(lock, [sp] { return !sp->held; });
            }
            sp->held = true;
        }
        out.ring = this;
        out.s = sp;
        Slot &s = *sp;
        hipError_t e;
        if (!s.done && (e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return e;
        if (s.used && (e = hipEventSynchronize(s.done)) != hipSuccess) return e;
        s.used = false;
        if (s.d.bytes() < bytes) {      // (the pair is let go before either is made anew; d is made last: its size is the pair's)
            s.h.reset();
            s.d.reset();
            const size_t cap = bytes + bytes / 2 + 4096;
            if ((e = s.h.alloc(cap)) != hipSuccess || (e = s.d.alloc(cap)) != hipSuccess) return e;
        }
        return hipSuccess;
    }
    ~SpanRing() { release(); }
    void release()      // on the owner's device, no lease outstanding
    {
        std::lock_guard<std::mutex> lock(mu);
        for (auto &sp : slots) {
            Slot &s = *sp;
            if (s.used) (void)hipEventSynchronize(s.done);
            if (s.done) (void)hipEventDestroy(s.done);
        }
        slots.clear();      // (with the slots' buffers)
        next = 0;
    }
};

// `slot` (empty) leases a slot of `ring` with room for `bytes`: DSP_OK, or DSP_EHIP "the span ring: ..."
inline int lease(SpanRing &ring, size_t bytes, SpanRing::Lease &slot)
{
    const hipError_t e = ring.acquire(bytes, slot);
    return e == hipSuccess ? DSP_OK : capi_fail(DSP_EHIP, std::string("the span ring: ") + hipGetErrorString(e));
}

// a device index the HIP runtime knows, or why not
inline int check_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return capi_fail(DSP_ENODEV, "no HIP device: libdsp_amd has no CPU fallback");
    if (device < 0 || device >= n) return capi_fail(DSP_EINVAL, "device index out of range");
    return DSP_OK;
}

// a caller's float GMM: DSP_EINVAL "<who> and its arrays must not be NULL"; handed in as a model, then "<prefix>k must be 1 .. 64, got <k>", and d
inline int check_gmm_float_arrays(const dsp_gmm_float_params *g, const char *who)
{
    return g && g->log_consts && g->means && g->inv_covs ? DSP_OK : capi_fail(DSP_EINVAL, std::string(who) + " and its arrays must not be NULL");
}
inline int check_gmm_float_params(const dsp_gmm_float_params *g, const char *who, const char *prefix)
{
    if (const int rc = check_gmm_float_arrays(g, who)) return rc;
    if (g->k < 1 || g->k > kGmmMaxK) return capi_fail(DSP_EINVAL, std::string(prefix) + "k must be 1 .. 64, got " + std::to_string(g->k));
    if (g->d < 1 || g->d > kGmmMaxD) return capi_fail(DSP_EINVAL, std::string(prefix) + "d must be 1 .. 16, got " + std::to_string(g->d));
    return DSP_OK;
}

// The float UBM of a handle (enroller, verifier).  A caller's UBM that check_gmm_float_params has passed -> the float32 block of
// gmm_model.hpp on the host, or DSP_EINVAL where a value is not finite in float32
inline int pack_ubm(const dsp_gmm_float_params *ubm, std::vector<float> &host)
{
    host = pack_gmm_model(ubm->k, ubm->d, ubm->log_consts, ubm->means, ubm->inv_covs);
    for (const float v : host)
        if (!std::isfinite(v)) return capi_fail(DSP_EINVAL, "ubm: log_consts, means and inv_covs must be finite in float32");
    return DSP_OK;
}
// that block into `model` on the current device: DSP_OK, DSP_ENOMEM, or DSP_EHIP "<copy_failed>: <the runtime's error>" with `model`
// left empty (the enroller names the call, as it always has)
inline int upload_ubm(const std::vector<float> &host, DeviceBuf<float> &model, const char *copy_failed = "hipMemcpy of the UBM")
{
    if (model.alloc(host.size() * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the UBM");
    const hipError_t e = hipMemcpy(model, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) return DSP_OK;
    model.reset();
    return capi_fail(DSP_EHIP, std::string(copy_failed) + ": " + hipGetErrorString(e));
}

// clip c of a ragged batch is samples [offsets[c], offsets[c + 1]) per channel: its length, or DSP_EINVAL naming the clip
inline long ragged_clip_length(const long *offsets, long c)
{
    const long n = offsets[c + 1] - offsets[c];
    if (offsets[c] < 0 || n < 0 || n > INT32_MAX)
        return capi_fail(DSP_EINVAL, "offsets must be non-negative and non-decreasing, clips shorter than 2^31 samples (clip " + std::to_string(c) + ")");
    return n;
}

// the input kind of int16 PCM (1 / 2 / 3: mono / stereo channel 0 / stereo average), or DSP_EINVAL
inline int pcm16_kind(int channels, int stereo_mode)
{
    if (channels != 1 && channels != 2) return capi_fail(DSP_EINVAL, "channels must be 1 or 2");
    if (channels == 2 && stereo_mode != DSP_STEREO_CHANNEL0 && stereo_mode != DSP_STEREO_AVERAGE) return capi_fail(DSP_EINVAL, "bad stereo_mode");
    return channels == 1 ? 1 : (stereo_mode == DSP_STEREO_CHANNEL0 ? 2 : 3);
}

}

// ---- window scans of long recordings (capi_consumers.cpp: stop / speaker; capi_scrubjay.cpp: SVM) ----------------------------------------------
// Recording r is rows [frame_offsets[r], frame_offsets[r + 1]) of a ragged MFCC matrix, R rows: R >= window_frames gives
// 1 + (R - window_frames) / hop_frames windows, fewer rows one window of all of them.
namespace dsp {
inline int scan_args(const dsp_scan_config *cfg, long n)
{
    if (!cfg || cfg->window_frames < 1 || cfg->hop_frames < 1) return capi_fail(DSP_EINVAL, "dsp_scan_config: window_frames and hop_frames must be >= 1");
    if (n < 0) return capi_fail(DSP_EINVAL, "n_recordings < 0");
    return DSP_OK;
}

// the host planner: wo[r + 1] = wo[r] + windows of recording r, to[r + 1] = to[r] + ceil(windows / tw) (to may be NULL); total windows or < 0
inline long scan_plan(const dsp_scan_config *cfg, const long *frame_offsets, long n, long *wo, long *to, int tw)
{
    if (const int rc = scan_args(cfg, n)) return rc;
    if (n == 0) {
        if (wo) wo[0] = 0;
        if (to) to[0] = 0;
        return 0;
    }
    if (!frame_offsets || !wo) return capi_fail(DSP_EINVAL, "frame_offsets and window_offsets must not be NULL");
    if (frame_offsets[0] < 0) return capi_fail(DSP_EINVAL, "frame_offsets must be non-negative");
    wo[0] = 0;
    if (to) to[0] = 0;
    for (long r = 0; r < n; ++r) {
        const long rows = frame_offsets[r + 1] - frame_offsets[r];
        if (rows < 0) return capi_fail(DSP_EINVAL, "frame_offsets decrease at recording " + std::to_string(r));
        const long w = rows >= cfg->window_frames ? 1 + (rows - cfg->window_frames) / cfg->hop_frames : 1;
        wo[r + 1] = wo[r] + w;
        if (to) to[r + 1] = to[r] + (w + tw - 1) / tw;
    }
    return wo[n];
}

// a scan that pools or averages a window's rows: DSP_EINVAL "recording r<tail>" for the first recording (or `what`) without rows
inline int refuse_rowless(const long *frame_offsets, long n, const char *tail, const char *what = "recording")
{
    for (long r = 0; r < n; ++r)
        if (frame_offsets[r + 1] == frame_offsets[r]) return capi_fail(DSP_EINVAL, what + (" " + std::to_string(r)) + tail);
    return DSP_OK;
}

// frame_offsets[n + 1] of a ragged matrix outside a scan (n >= 1): non-negative and non-decreasing, or DSP_EINVAL naming the first
// recording (or `what`) at which they decrease
inline int check_frame_offsets(const long *frame_offsets, long n, const char *what = "recording")
{
    if (frame_offsets[0] < 0) return capi_fail(DSP_EINVAL, "frame_offsets must be non-negative");
    for (long r = 0; r < n; ++r)
        if (frame_offsets[r + 1] < frame_offsets[r]) return capi_fail(DSP_EINVAL, std::string("frame_offsets decrease at ") + what + " " + std::to_string(r));
    return DSP_OK;
}

// per-recording arrays for the kernels, rows relative to frame_offsets[0]: fo, wo[, to][, extra], n + 1 longs each, into a leased ring
// slot, uploaded
inline hipError_t scan_upload(SpanRing &ring, const long *frame_offsets, long n, const long *wo, const long *to, SpanRing::Lease &slot,
                              void *stream, const long *extra = nullptr)
{
    const size_t one = (size_t)(n + 1) * sizeof(long), bytes = (2 + (to ? 1 : 0) + (extra ? 1 : 0)) * one;
    const hipError_t e = ring.acquire(bytes, slot);
    if (e != hipSuccess) return e;
    long *h = static_cast<long *>(slot.h());
    for (long r = 0; r <= n; ++r) h[r] = frame_offsets[r] - frame_offsets[0];
    std::memcpy(h + (n + 1), wo, one);
    if (to) std::memcpy(h + 2 * (n + 1), to, one);
    if (extra) std::memcpy(h + (to ? 3 : 2) * (n + 1), extra, one);
    return slot.upload(bytes, (hipStream_t)stream);
}
}

// order[i] = index of the i-th largest key, ties in input order (what std::stable_sort gives) -- by counting: a ragged batch of 125 000
// clips is ordered in well under a millisecond, where the comparison sort took longer than the kernel it was ordering for
namespace dsp {
inline void order_by_key_desc(const int *key, long n, int key_max, int *order)
{
    if (key_max < 0 || key_max > (1 << 22)) {               // (absurd key ranges: the comparison sort)
        for (long i = 0; i < n; ++i) order[i] = (int)i;
        std::stable_sort(order, order + n, [&](int a, int b) { return key[a] > key[b]; });
        return;
    }
    std::vector<long> start((size_t)key_max + 2, 0);
    for (long i = 0; i < n; ++i) ++start[(size_t)(key_max - key[i]) + 1];
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    for (long i = 0; i < n; ++i) order[start[(size_t)(key_max - key[i])]++] = (int)i;
}
}

#define DSP_CAPI_HIP(call)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return dsp::capi_fail(DSP_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The entry points work on the GPU their plan / model / buffers live on, which need not be the caller's current device
// (torch keeps its own idea of it): switch for the duration of the call and put the caller's device back on every exit.
namespace dsp {
struct DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device); else prev = -1;      // nothing to restore
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

}
#define DSP_ON_DEVICE(dev)                                                                                        \
    dsp::DeviceScope dsp_device_scope_(dev);                                                                      \
    if (dsp_device_scope_.err != hipSuccess)                                                                      \
        return dsp::capi_fail(DSP_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(dsp_device_scope_.err))

// ---- handles: one create path, one destroy path ----------------------------------------------------------------------------------
// Every handle that lives on one GPU derives from Handle, is made by create_on_device or create_on_host and is let go by destroy: its
// device members (DeviceBuf, SpanRing, handles it owns) are released by its own destructor, and these three are the only places that
// run it -- always inside the DeviceScope of the handle's device.  Not here, each for a reason: dsp_gather (capi_gather.cpp) owns
// communicators on several devices, so there is no one device to make current; the classifier contexts (dsp_classify_ctx and the
// per-device Work of classify_front.hpp) live under their own mutex and are immortal or released by front::release.
namespace dsp {
struct Handle {
    int device = 0;
};

// The handle of a create function whose arguments have passed (its own checks, check_device among them, stay in front of this call,
// in their order): made and initialised with `device` current -- init(H &) returns DSP_OK or what capi_fail returned -- and stored in
// *out on success alone.  The handle is declared after the scope, so whatever init had allocated when it failed is freed before the
// caller's device is put back.
template <class H, class Init> int create_on_device(int device, H **out, Init init)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    DSP_ON_DEVICE(device);
    auto h = std::make_unique<H>();
    h->device = device;
    if (const int rc = init(*h)) return rc;
    *out = h.release();
    return DSP_OK;
}

// The same for a handle whose create touches no device (init may check arguments and fill host members, nothing else): a device that
// does not exist is reported by the first call that launches, only a negative index here.
template <class H, class Init> int create_on_host(int device, H **out, Init init)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (device < 0) return capi_fail(DSP_EINVAL, "device index out of range");
    auto h = std::make_unique<H>();
    h->device = device;
    if (const int rc = init(*h)) return rc;
    *out = h.release();
    return DSP_OK;
}
template <class H> int create_on_host(int device, H **out)
{
    return create_on_host(device, out, [](H &) { return DSP_OK; });
}

// every dsp_*_destroy of a Handle: NULL is a no-op
template <class H> void destroy(H *h)
{
    if (!h) return;
    DeviceScope scope(h->device);
    delete h;
}

// the deleter of a handle another handle owns: std::unique_ptr<dsp_mfcc_plan, DestroyWith<dsp_mfcc_plan_destroy>>
template <auto Destroy> struct DestroyWith {
    template <class H> void operator()(H *h) const { Destroy(h); }
};

// What a stage on a score matrix keeps between calls (dsp_segmenter, dsp_trial_evaluator, dsp_calibrator derive from it): a grow-only
// workspace and the ring its host arrays travel through.
struct StageHandle : Handle {
    DeviceBuf<char> ws;
    SpanRing spans;
};
}
