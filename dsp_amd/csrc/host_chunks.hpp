// host_chunks.hpp -- the chunk planner of the host pipeline (host_pipe.hpp): how a batch in host memory is cut into the chunks that travel
// through the pinned ring.  No HIP, no library state: it compiles on its own (tests/test_host_stream_cpu.py builds it into a stand-alone
// program under the sanitizers) and is what dsp_host_plan_chunks hands out.
//
// A plan is the list of the chunks' first items, first[0] = 0 < first[1] < ... < first[n_chunks] = n_items: chunk k is items
// [first[k], first[k + 1]).  The chunks tile the batch in order and every chunk holds at least one item; a batch without items has no chunk.
//     uniform items   floor(chunk_bytes / item_bytes) items per chunk, at least 1 (at most max_items where the caller has a bound of its
//                     own: a classifier's sub-batch)
//     ragged batches  clip c = samples [offsets[c], offsets[c + 1]) of bytes_per_sample bytes each.  Cut at clip boundaries only, filled
//                     greedily up to chunk_bytes: a chunk is closed in front of the first clip that would take it past chunk_bytes.  A
//                     clip longer than chunk_bytes is therefore the only clip WITH SAMPLES of its chunk, and an empty clip never opens a
//                     chunk of its own (it rides with the clips before it; the empty clips at the batch's head with the first one behind).
#pragma once

#include <algorithm>
#include <vector>

namespace dsp {
namespace host {

constexpr long kMinChunkBytes = 4096;

inline long uniform_items_per_chunk(long item_bytes, long chunk_bytes, long max_items = 0)
{
    long per = std::max(1L, chunk_bytes / std::max(1L, item_bytes));
    if (max_items > 0) per = std::min(per, max_items);
    return per;
}

inline void plan_uniform(long n_items, long item_bytes, long chunk_bytes, std::vector<long> &first, long max_items = 0)
{
    first.clear();
    first.push_back(0);
    const long per = uniform_items_per_chunk(item_bytes, chunk_bytes, max_items);
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

}  // namespace host
}  // namespace dsp
