// host_pipe.hpp -- the host pipeline: how a batch in HOST memory travels through the GPU for the blocking *_host entry points (capi.cpp:
// the MFCC entries; classify_front.hpp: both classifiers; capi_host.cpp: its configuration, statistics and the pinned allocator).
//
// One pipeline per device, made at first use and immortal like front::workspaces() (no destructor calls into HIP at exit);
// dsp_host_pipeline_release returns its memory and its stream.  It has a mutex of its own.  LOCK ORDER: the entry's lock first (plan->mu of an MFCC
// plan, w.mu of a classifier's workspace), then the pipeline's; nothing takes them the other way round, and the pipeline's lock is
// never held while another pipeline's is asked for.
//
// A call cuts its batch into chunks (host_chunks.hpp) and sends them through a ring of `depth` slots.  A slot owns a pinned host buffer
// and a device staging buffer for input, the same pair for output, and two events.  ONE stream of the pipeline's own beside the null
// stream, ordered by those events:
//     s_in          H2D of chunk k into its slot                                          records in_done
//     null stream   waits in_done; the entry's kernels; D2H of the results                records out_done
// so that with depth >= 2 the copy in of chunk k + 1 runs under the kernels and the copy out of chunk k.  (The copy in is all but the
// whole of a host call; kernels and copy out share a stream because a stream of their own each measured no faster, and every stream
// the library holds sits on one of the process's few hardware queues.)  A slot is taken again only after out_done of the chunk that
// had it has fired (the host waits for it, as SpanRing's acquirer does for its slot's event), which is behind every reader and writer
// of the slot's four buffers.
// A batch of ONE chunk takes none of this: copy in, kernels and copy out on the null stream, straight from and to the caller's arrays,
// one synchronise (run_one) -- the one pass and the launches of the whole batch, and what a single clip through compute_mfcc() or
// classify() costs.
// The input path of a batch of several chunks is chosen per call from the caller's pointer (hipPointerGetAttributes; a plain malloc
// pointer is unknown to the runtime: that is "pageable", and the sticky error is cleared):
//     pinned / registered memory    copied asynchronously straight from it (1-D, or 2-D where rows are re-pitched)
//     pageable memory               by pageable_mode.  _WHOLE (the default): the batch is NOT cut -- one chunk, above; cutting a pageable
//                                   batch measured level with that at best.  _REGISTER: the caller's arrays are
//                                   page-locked for the duration of the call and read as pinned; where the runtime refuses, _DIRECT:
//                                   the array is handed to the runtime's own pageable copy, chunk by chunk.  _STAGE: each chunk's
//                                   rows are packed by memcpy into the slot's pinned buffer at the pitch the kernels want
// Results return the same way: into the caller's arrays directly where they are pinned (or, under _REGISTER, can be page-locked), else
// into the slot's pinned buffer and by memcpy after out_done.  The entries stay blocking: when run() returns every output byte is in
// the caller's memory and nothing is in flight; after a failure everything is drained as well, every slot is free, and the next
// call finds the pipeline usable.  Device staging is bounded by depth x the largest chunk, never by the batch (of pinned memory).
//
// WHERE THINGS LIVE.  The arithmetic of a batch -- its plan, its extent, where chunk k lies -- is a layout of host_chunks.hpp (HIP-free).
// An entry makes its checks, takes its own lock, describes its batch by a layout and its result arrays by an Outs, and hands both
// with its `kernels` callable to a Session (the foot of this file): open() checks the device, locks the pipeline, plans the chunks
// and opens the pipeline; run() builds the Job and every chunk's InCopy / OutCopy.  No entry fills one itself.  The slots' buffers are
// DeviceBuf / PinnedBuf (capi_util.hpp) of exactly the bytes asked for; release() lets them go, the pipelines being immortal.
#pragma once

#include <hip/hip_runtime_api.h>

#include <climits>
#include <cstring>
#include <mutex>
#include <vector>

#include "capi_util.hpp"
#include "host_chunks.hpp"

namespace dsp {
namespace host {

constexpr int kMaxDepth = 4;
// From tools/time_host.py's sweep on the target (profiles/host_stream_sweep.jsonl).  Far above any test batch, so that the
// small host calls of the suite -- and compute_mfcc() / classify() -- are one chunk.
constexpr long kDefaultChunkBytes = 64L << 20;
constexpr int kDefaultDepth = 2, kDefaultPageable = DSP_HOST_PAGEABLE_WHOLE;
// the fewest clips of a chunk of a classifier's host batch (dsp_host_pipeline_config::classify_min_clips): a pass walks every clip's
// recurrence in sequence, 64 clips per block, so a pass of few clips costs nearly what a pass of thousands does.  The default is the
// largest sub-batch: a classifier's chunk is a whole pass through its workspace, as before the pipeline -- measured from pinned memory, smaller passes
// under the copy are worth 4.7 % on the float64 classifier and nothing on ragged batches
constexpr int kDefaultClassifyMinClips = 65536;
inline dsp_host_pipeline_config default_config() { return {kDefaultChunkBytes, kDefaultDepth, kDefaultPageable, kDefaultClassifyMinClips}; }

// how one chunk's input lies in the caller's memory and in the staging buffer: `rows` rows of `width` bytes, src_pitch apart at the
// caller's, dst_pitch apart in staging (rows == 1: one run of `width` bytes)
struct InCopy {
    const void *src = nullptr;
    size_t src_pitch = 0, dst_pitch = 0, width = 0, rows = 1;
    // rows of clips (a single chunk is then copied by the runtime's 2-D copy even where the pitches agree: from pageable memory it
    // measured 1.5 % faster than the 1-D copy of the same bytes, and it is the copy these entries have always made)
    bool pitched = false;
    size_t staged_bytes() const { return host::staged_bytes(rows, dst_pitch, width); }
};
// up to two result arrays per chunk (a classifier's labels and trace), back to back in the staging buffer at 256-byte boundaries
struct OutCopy {
    void *dst[2] = {nullptr, nullptr};
    size_t bytes[2] = {0, 0};
    size_t at(int i) const { return i == 0 ? 0 : (bytes[0] + 255) & ~(size_t)255; }
    size_t staged_bytes() const { return bytes[1] ? at(1) + bytes[1] : bytes[0]; }
};

// A batch: its chunk count, the caller's arrays and their extents (for the choice of the paths), and -- for a batch of ONE chunk whose
// kernels leave their results in a workspace of the entry's -- where those lie on the device (else they are written to d_out).
// Pipe::run() takes two callables beside it: chunk(k, InCopy &, OutCopy &), the copies of chunk k (Session::run makes it), and the
// entry's kernels(k, d_in, d_out, stream) -> int: d_in the staged input, d_out[i] where result array i is to be left (OutCopy::at).
struct Job {
    long n_chunks = 0;
    const void *in_base = nullptr;
    size_t in_extent = 0;
    void *out_base[2] = {nullptr, nullptr};
    size_t out_extent[2] = {0, 0};
    const void *resident[2] = {nullptr, nullptr};
};

// whether [p, p + bytes) is host memory the runtime knows (page-locked by its allocator, or registered): what a copy engine reads without a bounce.
// Both ends are asked.  (An array whose ends are registered and whose middle is not is copied correctly all the same -- the runtime
// bounces what it does not know -- only not asynchronously.)
inline bool pinned_range(const void *p, size_t bytes)
{
    if (!p || bytes == 0) return false;
    const void *ends[2] = {p, static_cast<const char *>(p) + bytes - 1};
    for (const void *q : ends) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {      // a plain malloc pointer: pageable
            (void)hipGetLastError();
            return false;
        }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}

struct Pipe {
    std::mutex mu;
    int device = -1;                                   // -1: nothing allocated
    dsp_host_pipeline_config cfg = default_config();
    hipStream_t s_in = nullptr;                        // the copies in of a batch of several chunks; everything else runs on the null stream
    bool events = false;                               // every slot has its two events
    struct Slot {
        PinnedBuf h_in, h_out;                         // grow-only, to exactly the bytes of the largest chunk seen
        DeviceBuf<char> d_in, d_out;
        hipEvent_t in_done = nullptr, out_done = nullptr;
        bool pending = false;                          // a chunk's results are on their way: out_done has to fire before anything else
        OutCopy out;                                   // of that chunk, for the memcpy home
        bool out_staged = false;
    } slots[kMaxDepth];
    dsp_host_stats last{};

    size_t staging_bytes() const { size_t b = 0; for (const Slot &s : slots) b += s.d_in.bytes() + s.d_out.bytes(); return b; }
    size_t pinned_bytes() const { size_t b = 0; for (const Slot &s : slots) b += s.h_in.bytes() + s.h_out.bytes(); return b; }

    // The input bytes a chunk of this call may hold: cfg.chunk_bytes -- but a batch in PAGEABLE memory is not cut under
    // DSP_HOST_PAGEABLE_WHOLE (the default: measured, cutting it does not pay).  A batch that fits a chunk is not asked about.
    long chunk_bytes_for(const void *in_base, size_t in_extent) const
    {
        if (cfg.pageable_mode != DSP_HOST_PAGEABLE_WHOLE || in_extent <= (size_t)cfg.chunk_bytes || pinned_range(in_base, in_extent)) return cfg.chunk_bytes;
        return LONG_MAX / 4;
    }

    // the caller holds mu and has made `dev` current; n_chunks > 1: with the copy stream.  The stream is made by the first call of
    // several chunks and kept until dsp_host_pipeline_release: ONE stream, because a process has few hardware queues (four by default)
    // that the runtime deals its streams out over, and streams of the library's would sit on queues the caller's own then share
    int open(int dev, long n_chunks)
    {
        device = dev;
        if (!events) {
            for (Slot &s : slots) {
                if (!s.in_done) DSP_CAPI_HIP(hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming));
                if (!s.out_done) DSP_CAPI_HIP(hipEventCreateWithFlags(&s.out_done, hipEventDisableTiming));
            }
            events = true;      // (only now: a creation that failed is made up for by the next call)
        }
        if (n_chunks > 1 && !s_in) DSP_CAPI_HIP(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
        return DSP_OK;
    }

    // everything idle, every slot free (after a failure; the error that caused it stays in dsp_last_error())
    void drain()
    {
        if (s_in) (void)hipStreamSynchronize(s_in);
        (void)hipStreamSynchronize(nullptr);
        (void)hipGetLastError();
        for (Slot &s : slots) s.pending = false;
    }

    void release()      // on the pipeline's device, made current by the caller, under mu
    {
        drain();
        for (Slot &s : slots) {
            if (s.in_done) (void)hipEventDestroy(s.in_done);
            if (s.out_done) (void)hipEventDestroy(s.out_done);
            s = Slot{};                                // (lets the four buffers go)
        }
        if (s_in) (void)hipStreamDestroy(s_in);
        s_in = nullptr;
        events = false;
        device = -1;
    }

    template <class Chunk, class Kernels> int run(const Job &job, const Chunk &chunk, const Kernels &kernels);

    // a whole batch into slot 0's device input buffer on the null stream (the one-chunk ragged classifier, whose pass reads the flat
    // buffer and brings its results home itself); counted as the call's only chunk
    int stage_whole(const void *src, size_t bytes, void *&d)
    {
        last = dsp_host_stats{};
        last.n_chunks = last.depth = 1;
        last.input_path = last.output_path = DSP_HOST_PATH_DIRECT;
        Slot &s = slots[0];
        DSP_CAPI_HIP(s.d_in.reserve(bytes + 256));
        if (bytes) DSP_CAPI_HIP(hipMemcpyAsync(s.d_in, src, bytes, hipMemcpyHostToDevice, nullptr));
        last.bytes_h2d = (long)bytes;
        last.peak_staging_bytes = (long)staging_bytes();
        last.pinned_ring_bytes = (long)pinned_bytes();
        d = s.d_in;
        return DSP_OK;
    }

private:
    // the chunk that had the slot: wait for its results, take them home
    static int retire(Slot &s)
    {
        if (!s.pending) return DSP_OK;
        DSP_CAPI_HIP(hipEventSynchronize(s.out_done));
        s.pending = false;
        if (s.out_staged)
            for (int i = 0; i < 2; ++i)
                if (s.out.bytes[i]) std::memcpy(s.out.dst[i], static_cast<const char *>(s.h_out) + s.out.at(i), s.out.bytes[i]);
        return DSP_OK;
    }
    template <class Chunk, class Kernels> int run_one(const Job &job, const Chunk &chunk, const Kernels &kernels);
    template <class Chunk, class Kernels> int run_chunks(const Job &job, const Chunk &chunk, const Kernels &kernels, bool in_staged, bool out_staged);
};

// Immortal, one per device (see the head of this file)
inline Pipe *pipes()
{
    static Pipe *const all = new Pipe[kMaxDevices];
    return all;
}

// A batch of ONE chunk: copy in, the kernels, copy out on the null stream, straight from and to the caller's arrays whatever memory
// they are (the runtime's own copy), then one synchronise -- no events, no pointer queries, no other stream
template <class Chunk, class Kernels> int Pipe::run_one(const Job &job, const Chunk &chunk, const Kernels &kernels)
{
    Slot &s = slots[0];
    InCopy ic;
    OutCopy oc;
    chunk(0, ic, oc);
    int rc;
    DSP_CAPI_HIP(s.d_in.reserve(ic.staged_bytes() + 256));
    DSP_CAPI_HIP(s.d_out.reserve(oc.staged_bytes()));
    void *const d_out[2] = {s.d_out.get(), s.d_out.get() + oc.at(1)};
    if (ic.staged_bytes() == 0) {
    } else if (ic.pitched) {
        DSP_CAPI_HIP(hipMemcpy2DAsync(s.d_in, ic.dst_pitch, ic.src, ic.src_pitch, ic.width, ic.rows, hipMemcpyHostToDevice, nullptr));
    } else DSP_CAPI_HIP(hipMemcpyAsync(s.d_in, ic.src, ic.staged_bytes(), hipMemcpyHostToDevice, nullptr));
    last.bytes_h2d = (long)(ic.width * ic.rows);
    if ((rc = kernels(0, s.d_in.get(), d_out, nullptr)) < 0) return rc;
    for (int i = 0; i < 2; ++i) {
        if (!oc.bytes[i]) continue;
        const void *from = job.resident[i] ? job.resident[i] : d_out[i];
        DSP_CAPI_HIP(hipMemcpyAsync(oc.dst[i], from, oc.bytes[i], hipMemcpyDeviceToHost, nullptr));
        last.bytes_d2h += (long)oc.bytes[i];
    }
    DSP_CAPI_HIP(hipStreamSynchronize(nullptr));
    return DSP_OK;
}

// Several chunks.  in_staged / out_staged: through the slots' pinned buffers; otherwise the caller's arrays are handed to the copies as
// they are.  Chunk k: its copy in on s_in (-> in_done); on the null stream, behind in_done, its kernels and the copy out (-> out_done).
template <class Chunk, class Kernels> int Pipe::run_chunks(const Job &job, const Chunk &chunk, const Kernels &kernels, bool in_staged, bool out_staged)
{
    const int depth = cfg.depth;
    for (long k = 0; k < job.n_chunks; ++k) {
        Slot &s = slots[k % depth];
        int rc = retire(s);
        if (rc < 0) return rc;
        InCopy ic;
        OutCopy oc;
        chunk(k, ic, oc);
        // the kernels' vector loads may reach a few bytes past a row's end: slack behind the staged input, as behind a caller's buffer
        DSP_CAPI_HIP(s.d_in.reserve(ic.staged_bytes() + 256));
        DSP_CAPI_HIP(s.d_out.reserve(oc.staged_bytes()));
        void *const d_out[2] = {s.d_out.get(), s.d_out.get() + oc.at(1)};
        if (ic.staged_bytes() == 0) {      // (a chunk of empty clips: nothing travels in)
        } else if (in_staged) {
            DSP_CAPI_HIP(s.h_in.reserve(ic.staged_bytes()));
            if (ic.rows > 1 && ic.src_pitch != ic.dst_pitch) {
                for (size_t r = 0; r < ic.rows; ++r)
                    std::memcpy(static_cast<char *>(s.h_in) + r * ic.dst_pitch, static_cast<const char *>(ic.src) + r * ic.src_pitch, ic.width);
            } else std::memcpy(s.h_in, ic.src, ic.staged_bytes());
            DSP_CAPI_HIP(hipMemcpyAsync(s.d_in, s.h_in, ic.staged_bytes(), hipMemcpyHostToDevice, s_in));
        } else if (ic.rows > 1 && ic.src_pitch != ic.dst_pitch) {
            DSP_CAPI_HIP(hipMemcpy2DAsync(s.d_in, ic.dst_pitch, ic.src, ic.src_pitch, ic.width, ic.rows, hipMemcpyHostToDevice, s_in));
        } else DSP_CAPI_HIP(hipMemcpyAsync(s.d_in, ic.src, ic.staged_bytes(), hipMemcpyHostToDevice, s_in));
        last.bytes_h2d += (long)(ic.width * ic.rows);
        DSP_CAPI_HIP(hipEventRecord(s.in_done, s_in));
        DSP_CAPI_HIP(hipStreamWaitEvent(nullptr, s.in_done, 0));
        if ((rc = kernels(k, s.d_in.get(), d_out, nullptr)) < 0) return rc;
        if (out_staged) DSP_CAPI_HIP(s.h_out.reserve(oc.staged_bytes()));
        for (int i = 0; i < 2; ++i) {
            if (!oc.bytes[i]) continue;
            void *to = out_staged ? s.h_out.get() + oc.at(i) : oc.dst[i];
            DSP_CAPI_HIP(hipMemcpyAsync(to, d_out[i], oc.bytes[i], hipMemcpyDeviceToHost, nullptr));
            last.bytes_d2h += (long)oc.bytes[i];
        }
        DSP_CAPI_HIP(hipEventRecord(s.out_done, nullptr));
        s.pending = true;
        s.out = oc;
        s.out_staged = out_staged;
        last.peak_staging_bytes = std::max(last.peak_staging_bytes, (long)staging_bytes());
    }
    for (long k = std::max(0L, job.n_chunks - depth); k < job.n_chunks; ++k)      // the chunks still in flight, oldest first
        if (const int rc = retire(slots[k % depth])) return rc;
    return DSP_OK;
}

// page-locks [p, p + bytes) for the duration of a call; false where the runtime refuses (read-only pages, limits, a range that overlaps
// a registered one): the caller takes another path
inline bool register_range(const void *p, size_t bytes)
{
    if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// the caller holds mu (and, before it, its own lock), has made the pipeline's device current and has opened the pipeline
template <class Chunk, class Kernels> int Pipe::run(const Job &job, const Chunk &chunk, const Kernels &kernels)
{
    last = dsp_host_stats{};
    last.n_chunks = job.n_chunks;
    if (job.n_chunks <= 0) return DSP_OK;
    int rc;
    if (job.n_chunks == 1) {
        last.depth = 1;
        last.input_path = last.output_path = DSP_HOST_PATH_DIRECT;
        if ((rc = run_one(job, chunk, kernels)) < 0) { (void)hipStreamSynchronize(nullptr); (void)hipGetLastError(); }
    } else {
        last.depth = cfg.depth;
        const void *registered[3] = {nullptr, nullptr, nullptr};
        const bool may_register = cfg.pageable_mode == DSP_HOST_PAGEABLE_REGISTER;
        // input: memory the runtime knows is copied from as it is; pageable memory by the configured mode (_WHOLE gets here only where
        // the entry has a bound of its own on a pass, a classifier's sub-batch: chunk by chunk through the runtime's copy)
        if (pinned_range(job.in_base, job.in_extent)) last.input_path = DSP_HOST_PATH_PINNED;
        else if (cfg.pageable_mode == DSP_HOST_PAGEABLE_STAGE) last.input_path = DSP_HOST_PATH_STAGED;
        else if (may_register && register_range(job.in_base, job.in_extent)) { last.input_path = DSP_HOST_PATH_REGISTERED; registered[0] = job.in_base; }
        else last.input_path = DSP_HOST_PATH_DIRECT;
        // results: into the caller's arrays where every one of them is pinned (or can be registered), else through the pinned ring
        // (a copy to pageable memory would hold the host until it has ended, and with it the chunks behind)
        const int n_out = job.out_base[1] ? 2 : 1;
        bool all_pinned = true;
        for (int i = 0; i < n_out; ++i) all_pinned = all_pinned && pinned_range(job.out_base[i], job.out_extent[i]);
        last.output_path = all_pinned ? DSP_HOST_PATH_PINNED : DSP_HOST_PATH_STAGED;
        if (!all_pinned && may_register) {
            bool ok = true;
            for (int i = 0; i < n_out && ok; ++i) {
                if (pinned_range(job.out_base[i], job.out_extent[i])) continue;
                ok = register_range(job.out_base[i], job.out_extent[i]);
                if (ok) registered[1 + i] = job.out_base[i];
            }
            if (ok) last.output_path = DSP_HOST_PATH_REGISTERED;
            else for (int i = 1; i < 3; ++i) { if (registered[i]) (void)hipHostUnregister(const_cast<void *>(registered[i])); registered[i] = nullptr; }
        }
        rc = run_chunks(job, chunk, kernels, last.input_path == DSP_HOST_PATH_STAGED, last.output_path == DSP_HOST_PATH_STAGED);
        if (rc < 0) drain();
        else if (registered[0]) (void)hipStreamSynchronize(s_in);
        for (const void *r : registered)
            if (r) (void)hipHostUnregister(const_cast<void *>(r));
    }
    last.pinned_ring_bytes = (long)pinned_bytes();
    last.peak_staging_bytes = std::max(last.peak_staging_bytes, (long)staging_bytes());
    return rc;
}

// An entry's result arrays (one or two; base[1] NULL: one): array i holds unit[i] bytes per unit.  Chunk k owns the units
// [prefix[first[k]], prefix[first[k + 1]]) of each -- prefix NULL: its items themselves, one unit an item (ragged MFCC: a unit is a row,
// prefix the clips' frame offsets, from 0).  resident: Job::resident.
struct Outs {
    void *base[2] = {nullptr, nullptr};
    size_t unit[2] = {0, 0};
    const long *prefix = nullptr;
    const void *resident[2] = {nullptr, nullptr};
};

// A classifier's chunk is one pass through its workspace: at least the pipeline's classify_min_clips items, counted as min_item_bytes
// each (0: no floor; "at least one" asks nothing, every chunk holds an item), at most max_items (0: no cap)
struct ChunkLimits { long min_item_bytes = 0, max_items = 0; };

// The one driver of the *_host entries: the device's pipeline, locked, for the duration of a call.  The entry holds its own lock and
// has made the device current; `in` is the caller's pointer the layout counts from.
struct Session {
    Pipe *pipe = nullptr;
    std::unique_lock<std::mutex> lock;

    // locks the pipeline of `device`, plans the layout's chunks (l.first) and opens the pipeline for that many
    template <class Layout> int open(int device, const void *in, Layout &l, ChunkLimits lim = {})
    {
        if (device < 0 || device >= kMaxDevices) return capi_fail(DSP_EINVAL, "device index out of range");
        pipe = &pipes()[device];
        lock = std::unique_lock<std::mutex>(pipe->mu);
        const long min_items = pipe->cfg.classify_min_clips;
        const long floor = lim.min_item_bytes > 0 && min_items > 1 ? min_items * lim.min_item_bytes : 0;
        l.plan(std::max(pipe->chunk_bytes_for(static_cast<const char *>(in) + l.base_offset(), l.extent()), floor), lim.max_items);
        return pipe->open(device, n_chunks(l));
    }
    template <class Layout> static long n_chunks(const Layout &l) { return (long)l.first.size() - 1; }

    // every chunk of the batch through the pipeline, kernels(k, d_in, d_out, stream) enqueueing those of chunk k
    template <class Layout, class Kernels> int run(const void *in, const Layout &l, const Outs &o, const Kernels &kernels)
    {
        const auto unit = [&](long item) { return (size_t)(o.prefix ? o.prefix[item] : item); };
        Job job;
        job.n_chunks = n_chunks(l);
        job.in_base = static_cast<const char *>(in) + l.base_offset();
        job.in_extent = l.extent();
        for (int i = 0; i < 2; ++i) {
            job.out_base[i] = o.base[i];
            job.out_extent[i] = o.base[i] ? unit(l.first.back()) * o.unit[i] : 0;
            job.resident[i] = o.resident[i];
        }
        const auto chunk = [&](long k, InCopy &ic, OutCopy &oc) {
            ic.src = static_cast<const char *>(in) + l.src_offset(k);
            ic.src_pitch = l.src_pitch; ic.dst_pitch = l.dst_pitch; ic.width = l.chunk_width(k); ic.rows = l.rows(k); ic.pitched = l.pitched;
            const size_t u0 = unit(l.first[(size_t)k]), u1 = unit(l.first[(size_t)k + 1]);
            for (int i = 0; i < 2 && o.base[i]; ++i) {
                oc.dst[i] = static_cast<char *>(o.base[i]) + u0 * o.unit[i];
                oc.bytes[i] = (u1 - u0) * o.unit[i];
            }
        };
        return pipe->run(job, chunk, kernels);
    }
};

}  // namespace host
}  // namespace dsp
