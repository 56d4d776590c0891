// span_find.hpp -- "which span owns this block": the one binary search of the ragged launches whose blocks find their recording, speaker,
// clip or stream by it -- owner_of_unit (gmm_estep.hpp), owner_of_tile (resample_kernels.hip), scan_find (scan_device.hpp).  Joined only
// where the kernels' instructions stayed the same: clip_of_tile (vad_kernels.hip), owner_of_chunk (segment_kernels.hip) and span_of
// (augment_kernels.hip) write the search differently and keep their own.
#pragma once

#include <hip/hip_runtime.h>

namespace dsp {

// the last i in [0, n) with first(i) <= key (first non-decreasing, first(0) <= key; n >= 1): entries that own nothing share their
// successor's first and are passed over
template <class First> __device__ __forceinline__ long owner_of(long n, long key, First first)
{
    long lo = 0, hi = n;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (first(mid) <= key) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace dsp
