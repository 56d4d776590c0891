// stream_kernels.hip -- the gather of stream sessions (stream_kernels.hpp).  Memory bound: per push every new sample is read and
// written once on its way in front of the MFCC kernel, and every carried sample / row once more.  One block per slice of a run
// (<= 16 KiB): the widest vector access the run's source and destination BOTH allow (16 bytes when they agree modulo 16, which the host
// arranges for the carries and for chunks whose position agrees with the carry in front of them; else 8, 4 or the granule), the
// ragged edges in front of and behind the aligned body element by element.  No LDS, no atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "stream_kernels.hpp"

namespace dsp {

namespace {

// n elements of V; s and d are aligned to V
template <class V> __device__ __forceinline__ void copy_elems(const char *__restrict__ s, char *__restrict__ d, int n)
{
    const V *sv = reinterpret_cast<const V *>(s);
    V *dv = reinterpret_cast<V *>(d);
    for (int i = threadIdx.x; i < n; i += blockDim.x) dv[i] = sv[i];
}

// s and d agree modulo sizeof(V): G-sized elements up to d's first V boundary, whole V's, G-sized elements behind them
template <class G, class V> __device__ __forceinline__ void copy_run(const char *__restrict__ s, char *__restrict__ d, int bytes)
{
    constexpr int w = (int)sizeof(V);
    int head = (int)((w - (reinterpret_cast<uintptr_t>(d) & (w - 1))) & (w - 1));
    head = head < bytes ? head : bytes;
    const int body = (bytes - head) & ~(w - 1);
    copy_elems<G>(s, d, head / (int)sizeof(G));
    copy_elems<V>(s + head, d + head, body / w);
    copy_elems<G>(s + head + body, d + head + body, (bytes - head - body) / (int)sizeof(G));
}

// G: the granule every offset and size is a multiple of (unsigned short: 2 bytes, unsigned: 4 bytes).  Everything below is uniform
// over the block: one run per block, the branch on its alignment taken by all lanes alike.
template <class G> __global__ __launch_bounds__(256) void stream_copy_kernel(const CopyRun *__restrict__ runs, const char *__restrict__ src0,
                                                                             const char *__restrict__ src1, char *__restrict__ dst)
{
    const CopyRun r = runs[blockIdx.x];
    const char *s = (r.from ? src1 : src0) + r.src;
    char *d = dst + r.dst;
    const unsigned apart = (unsigned)((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d)) & 15);
    if (apart == 0) copy_run<G, uint4>(s, d, r.bytes);
    else if ((apart & 7) == 0) copy_run<G, uint2>(s, d, r.bytes);
    else if ((apart & 3) == 0) copy_run<G, unsigned>(s, d, r.bytes);
    else copy_elems<G>(s, d, r.bytes / (int)sizeof(G));
}

}  // namespace

hipError_t launch_stream_copy(const CopyRun *d_runs, long n_runs, const void *src0, const void *src1, void *dst, int granule, hipStream_t stream)
{
    if (n_runs <= 0) return hipSuccess;
    if (n_runs > INT32_MAX || (granule != 2 && granule != 4)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n_runs), block(256);
    const char *a = static_cast<const char *>(src0), *b = static_cast<const char *>(src1);
    char *o = static_cast<char *>(dst);
    if (granule == 2) hipLaunchKernelGGL(stream_copy_kernel<unsigned short>, grid, block, 0, stream, d_runs, a, b, o);
    else hipLaunchKernelGGL(stream_copy_kernel<unsigned>, grid, block, 0, stream, d_runs, a, b, o);
    return hipGetLastError();
}

}  // namespace dsp
