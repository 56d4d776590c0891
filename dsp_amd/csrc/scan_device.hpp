// scan_device.hpp -- device helpers of the window scans of long recordings (consumer_kernels.hip: stop / speaker, svm_kernels.hip: SVM).
#pragma once

#include <hip/hip_runtime.h>

#include "span_find.hpp"

namespace dsp {

// the r with off[r] <= key < off[r + 1] (off non-decreasing over n + 1 entries, off[0] <= key < off[n]): span_find.hpp's owner_of
__device__ __forceinline__ long scan_find(const long *__restrict__ off, long n, long key)
{
    return owner_of(n, key, [off](long r) { return off[r]; });
}

}  // namespace dsp
