// host_chunks.hpp -- the arithmetic of the host pipeline (host_pipe.hpp): how a batch in host memory is cut into the chunks that travel
// through the pinned ring (the planner), and where a chunk's bytes lie in the caller's memory and in staging (the layouts).  No HIP, no
// library state: it compiles on its own (tests/test_host_stream_cpu.py builds it into a stand-alone program under the sanitizers); the
// planner is what dsp_host_plan_chunks hands out, the layouts are what host::Session (host_pipe.hpp) drives every *_host entry from.
//
// A plan is the list of the chunks' first items, first[0] = 0 < first[1] < ... < first[n_chunks] = n_items: chunk k is items
// [first[k], first[k + 1]).  The chunks tile the batch in order and every chunk holds at least one item; a batch without items has no chunk.
//     uniform items   floor(chunk_bytes / item_bytes) items per chunk, at least 1 (at most max_items where the caller has a bound of its
//                     own: a classifier's sub-batch)
//     ragged batches  clip c = samples [offsets[c], offsets[c + 1]) of bytes_per_sample bytes each.  Cut at clip boundaries only, filled
//                     greedily up to chunk_bytes: a chunk is closed in front of the first clip that would take it past chunk_bytes.  A
//                     clip longer than chunk_bytes is therefore the only clip WITH SAMPLES of its chunk, and an empty clip never opens a
//                     chunk of its own (it rides with the clips before it; the empty clips at the batch's head with the first one behind).
// A layout is a batch (at least one item) with its plan.  Both kinds answer the same questions in bytes -- base_offset() and extent() of
// the whole batch from the caller's pointer, src_offset(k), rows(k) and chunk_width(k) of chunk k -- so that one driver serves both.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace dsp {
namespace host {

constexpr long kMinChunkBytes = 4096;

inline void plan_uniform(long n_items, long item_bytes, long chunk_bytes, std::vector<long> &first, long max_items = 0)
{
    first.clear();
    first.push_back(0);
    long per = std::max(1L, chunk_bytes / std::max(1L, item_bytes));
    if (max_items > 0) per = std::min(per, max_items);
    for (long c = per; c < n_items; c += per) first.push_back(c);
    if (n_items > 0) first.push_back(n_items);
}

// false: the offsets decrease somewhere (first is left empty)
inline bool plan_ragged(const long *offsets, long n_clips, long bytes_per_sample, long chunk_bytes, std::vector<long> &first)
{
    first.clear();
    for (long c = 0; c < n_clips; ++c)
        if (offsets[c + 1] < offsets[c]) return false;
    first.push_back(0);
    long bytes = 0;                       // of the open chunk
    for (long c = 0; c < n_clips; ++c) {
        const long b = (offsets[c + 1] - offsets[c]) * bytes_per_sample;
        if (b > 0 && bytes > 0 && (b > chunk_bytes || bytes > chunk_bytes - b)) {      // (written without the sum: no overflow)
            first.push_back(c);
            bytes = 0;
        }
        bytes += b;
    }
    if (n_clips > 0) first.push_back(n_clips);
    return true;
}

// what `rows` rows of `width` bytes, dst_pitch apart, take in staging
inline size_t staged_bytes(size_t rows, size_t dst_pitch, size_t width) { return rows > 1 ? dst_pitch * (rows - 1) + width : width; }

// Uniform items (frames, or clips of one length): item c is `width` bytes at src_pitch * c from the caller's pointer, staged dst_pitch
// apart -- the kernels' stride, and what the planner counts an item as.  pitched: rows of clips (InCopy::pitched)
struct UniformLayout {
    long n_items = 0;
    size_t src_pitch = 0, dst_pitch = 0, width = 0;
    bool pitched = false;
    std::vector<long> first;
    void plan(long chunk_bytes, long max_items = 0) { plan_uniform(n_items, (long)dst_pitch, chunk_bytes, first, max_items); }
    size_t base_offset() const { return 0; }
    size_t extent() const { return src_pitch * (size_t)(n_items - 1) + width; }
    size_t src_offset(long k) const { return (size_t)first[(size_t)k] * src_pitch; }
    size_t rows(long k) const { return (size_t)(first[(size_t)k + 1] - first[(size_t)k]); }
    size_t chunk_width(long) const { return width; }
    size_t staged_bytes(long k) const { return host::staged_bytes(rows(k), dst_pitch, width); }
};

// A ragged batch: clip c is samples [offsets[c], offsets[c + 1]) of bytes_per_sample bytes.  A chunk's samples start at a multiple of
// four samples at or below its first clip, start(k): every clip keeps its alignment in staging (16 bytes for floats, 8 for mono int16)
// and the copy starts on 8 bytes; consecutive chunks may share up to three samples.  The chunk's kernels see the offsets of rebase(k).
struct RaggedLayout {
    const long *offsets = nullptr;
    long n_clips = 0;
    size_t bytes_per_sample = 0;
    std::vector<long> first;
    static constexpr size_t src_pitch = 0, dst_pitch = 0;      // (one run of bytes a chunk)
    static constexpr bool pitched = false;
    void plan(long chunk_bytes, long = 0) { plan_ragged(offsets, n_clips, (long)bytes_per_sample, chunk_bytes, first); }
    long start(long k) const { return offsets[k == 0 ? 0 : first[(size_t)k]] & ~3L; }      // (k == 0: before there is a plan as well)
    size_t base_offset() const { return (size_t)start(0) * bytes_per_sample; }
    size_t extent() const { return (size_t)(offsets[n_clips] - start(0)) * bytes_per_sample; }
    size_t src_offset(long k) const { return (size_t)start(k) * bytes_per_sample; }
    size_t rows(long) const { return 1; }
    size_t chunk_width(long k) const { return (size_t)(offsets[first[(size_t)k + 1]] - start(k)) * bytes_per_sample; }
    // the offsets of chunk k's clips from the chunk's first staged sample: first[k + 1] - first[k] + 1 of them
    void rebase(long k, std::vector<long> &out) const
    {
        const long c0 = first[(size_t)k], cnt = first[(size_t)k + 1] - c0, s = start(k);
        out.resize((size_t)cnt + 1);
        for (long c = 0; c <= cnt; ++c) out[(size_t)c] = offsets[c0 + c] - s;
    }
};

}  // namespace host
}  // namespace dsp
