// stream_kernels.hpp -- the device side of stream sessions (capi_stream.cpp, include/dsp_amd.h "LIVE STREAMS"): one gather of short
// runs that stitches [carried samples | new chunk] per stream in front of the ragged MFCC kernel, puts the new tail back into the
// carry, and does the same for MFCC rows around the window scans.  The MFCC and scan kernels themselves are not touched.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <vector>

namespace dsp {

// One run of the gather: `bytes` from src0 + src (from = 0) or src1 + src (from = 1) to dst + dst.  Offsets and sizes in bytes, all
// multiples of the launch's granule (2: mono int16 sample frames; 4: float / stereo int16 sample frames and MFCC rows).  The host cuts
// long runs into slices of at most kStreamCopySlice bytes (a multiple of 16, so a slice keeps its run's alignment): one block per slice.
struct CopyRun {
    long src, dst;
    int bytes, from;
};
static_assert(sizeof(CopyRun) == 24, "three 8-byte scalar loads per run");
constexpr int kStreamCopySlice = 16384;

// a run of the gather, cut into the kernel's slices
inline void add_copy_runs(std::vector<CopyRun> &v, long src, long dst, long bytes, int from)
{
    for (long o = 0; o < bytes; o += kStreamCopySlice) v.push_back(CopyRun{src + o, dst + o, (int)std::min<long>(kStreamCopySlice, bytes - o), from});
}

// No run's source may overlap a run's destination within one launch (the session reads a carry in one launch and writes it in another).
// granule: 2 or 4.  n_runs = 0: no launch.
hipError_t launch_stream_copy(const CopyRun *d_runs, long n_runs, const void *src0, const void *src1, void *dst, int granule, hipStream_t stream);

}  // namespace dsp
