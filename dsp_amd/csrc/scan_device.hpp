// scan_device.hpp -- device helpers of the window scans of long recordings (consumer_kernels.hip: stop / speaker, svm_kernels.hip: SVM).
#pragma once

#include <hip/hip_runtime.h>

namespace dsp {

// the r with off[r] <= key < off[r + 1] (off non-decreasing over n + 1 entries, off[0] <= key < off[n])
__device__ __forceinline__ long scan_find(const long *__restrict__ off, long n, long key)
{
    long lo = 0, hi = n;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (off[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace dsp
