// resample_kernels.hip -- rational-ratio polyphase FIR resampling (scipy.signal.resample_poly's defaults).
//
//   y[k] = sum_i x[i] h[k down + half - i up]
//
// Output k reads polyphase branch p = (k down + half) mod up and the samples that end at i_max = (k down + half) div up: with the
// branch stored reversed and zero filled to `row` floats, y[k] = sum_jj x[i_max - (T - 1) + jj] taps[p][jj], jj ascending = input sample
// ascending: ONE float32 FMA chain per output, whose order depends on nothing but k.  Samples outside the recording are zeros.
//
// A block takes `tile` consecutive outputs of one recording and stages the samples they read in LDS, decoded to float in the load
// (int16 stays int16 in HBM).  A lane takes four outputs k, k + up, k + 2 up, k + 3 up: one branch, so one tap read feeds four FMAs, and
// the four sample streams lie `down` apart.  up == 1 has a single branch, whose taps are wave-uniform scalar loads: there a lane's four
// outputs lie a quarter tile apart and neighbouring lanes take neighbouring outputs.  The tile's outputs go through LDS to 16-byte
// stores wherever the output position allows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resample_kernels.hpp"
#include "span_find.hpp"

namespace dsp {
namespace {

constexpr int kR = kResampleOutputsPerLane;
constexpr int kThreads = 256;

// IN as everywhere (mfcc_kernels.hip): 0 float, 1 int16 mono s / 32768, 2 stereo L / 32768, 3 stereo (L + R) / 65536
template <int IN> __device__ inline float load_sample(const void *in, long i)
{
    if constexpr (IN == 0) return static_cast<const float *>(in)[i];
    else if constexpr (IN == 1) return (float)static_cast<const short *>(in)[i] * (1.0f / 32768.0f);
    else if constexpr (IN == 2) return (float)static_cast<const short *>(in)[2 * i] * (1.0f / 32768.0f);
    else return (float)((int)static_cast<const short *>(in)[2 * i] + (int)static_cast<const short *>(in)[2 * i + 1]) * (1.0f / 65536.0f);
}

template <int IN> __device__ inline float decode_pair(unsigned q)      // one 32-bit word of int16 PCM: a stereo frame (IN 2 / 3)
{
    const int l = (int)(short)(q & 0xffffu), r = (int)q >> 16;
    return IN == 2 ? (float)l * (1.0f / 32768.0f) : (float)(l + r) * (1.0f / 65536.0f);
}

// the recording (ResampleSpan) or stream (StreamResampleSpan) that owns tile t: the last one whose first tile is <= t (those without
// output own no tile) -- span_find.hpp's owner_of
template <class Span> __device__ inline long owner_of_tile(const Span *spans, long n, long t)
{
    return owner_of(n, t, [spans](long i) { return spans[i].tile0; });
}

// ys[0, cnt) -> o[0, cnt): one float per lane up to the first 16-byte boundary of o, 16-byte stores, a tail of single floats
__device__ inline void store_tile(const float *ys, float *o, int cnt)
{
    int head = (int)((0 - (reinterpret_cast<uintptr_t>(o) >> 2)) & 3);
    if (head > cnt) head = cnt;
    if ((int)threadIdx.x < head) o[threadIdx.x] = ys[threadIdx.x];
    const int nv = (cnt - head) >> 2;
    for (int v = threadIdx.x; v < nv; v += kThreads) {
        const float *y = ys + head + 4 * v;
        *reinterpret_cast<float4 *>(o + head + 4 * v) = make_float4(y[0], y[1], y[2], y[3]);
    }
    const int tail = head + 4 * nv + (int)threadIdx.x;
    if (tail < cnt) o[tail] = ys[tail];
}

template <int IN, bool STAGED, bool UP1>
__global__ __launch_bounds__(kThreads) void resample_kernel(const void *__restrict__ in, const ResampleSpan *__restrict__ spans, long n_rec,
                                                            long tile_base, ResampleShape s, const float *__restrict__ taps, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ys = lds;                      // [tile]
    float *xs = lds + s.tile;             // [span + 16] (tile is a multiple of 4: 16-byte aligned)
    const long t = tile_base + blockIdx.x;
    const ResampleSpan sp = spans[owner_of_tile(spans, n_rec, t)];
    const long k0 = (t - sp.tile0) * s.tile;
    const long a0 = k0 * s.down + s.half;
    const long i0 = a0 / s.up;
    const unsigned p0 = (unsigned)(a0 - i0 * s.up);
    const long i_lo = i0 - (s.taps - 1);                         // the first sample output k0 reads (may be < 0: zeros)
    unsigned shift = 0;                                            // xs[shift + d] = sample i_lo + d
    if constexpr (STAGED) {
        constexpr int ESZ = IN == 1 ? 2 : 4, EPC = 16 / ESZ;       // bytes per sample frame in HBM, frames per 16-byte chunk
        const uintptr_t g = reinterpret_cast<uintptr_t>(in) + (uintptr_t)((sp.in_off + i_lo) * ESZ);
        const bool vec = g % ESZ == 0;                             // (interleaved stereo at an odd int16: frame by frame)
        shift = vec ? (unsigned)(g & 15) / ESZ : 0;
        const int chunks = (int)(shift + s.span + EPC - 1) / EPC;
        for (int c = threadIdx.x; c < chunks; c += kThreads) {
            const long first = i_lo - (long)shift + (long)c * EPC;        // the chunk's first sample
            float v[EPC];
            if (vec && first >= 0 && first + EPC <= sp.n) {        // a whole aligned 16 bytes of this recording
                const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const char *>(in) + (sp.in_off + first) * ESZ);
                const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (IN == 0) v[e] = __uint_as_float(w[e]);
                    else if constexpr (IN == 1) {
                        v[2 * e] = (float)(int)(short)(w[e] & 0xffffu) * (1.0f / 32768.0f);
                        v[2 * e + 1] = (float)((int)w[e] >> 16) * (1.0f / 32768.0f);
                    } else v[e] = decode_pair<IN>(w[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const long i = first + e;
                    v[e] = i >= 0 && i < sp.n ? load_sample<IN>(in, sp.in_off + i) : 0.0f;
                }
            }
#pragma unroll
            for (int e = 0; e < EPC; e += 4)
                *reinterpret_cast<float4 *>(xs + c * EPC + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
        }
        __syncthreads();
    }
    const long left = sp.n_out - k0;                               // outputs of the recording from k0 on (>= 1)
    const int cnt = left < s.tile ? (int)left : s.tile;
    for (int it = threadIdx.x; it < s.items; it += kThreads) {
        // the lane's outputs k0 + q + r ostep share branch p; their sample streams lie xstep apart.  up == 1 has one branch: there the
        // lanes take neighbouring outputs (samples `down` apart: no LDS bank conflict for an odd down, two-way for 2 and 6)
        const int b = UP1 ? 0 : it / s.up;
        const int q = UP1 ? it : b * kR * s.up + (it - b * s.up);
        const int ostep = UP1 ? s.items : s.up, xstep = UP1 ? s.items * s.down : s.down;
        if (q >= cnt) continue;
        const unsigned w = (unsigned)q * (unsigned)s.down + p0;
        const unsigned irel = UP1 ? w : w / (unsigned)s.up;        // i_max(k0 + q) - i0
        const unsigned p = UP1 ? 0u : w - irel * (unsigned)s.up;
        const float *row = taps + (size_t)p * s.row;
        float acc[kR] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float *x = xs + shift + irel;
        const long ib = sp.in_off + i_lo + irel;
        for (int jj = 0; jj < s.row; jj += 4) {
            const float4 h4 = *reinterpret_cast<const float4 *>(row + jj);
            const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    float xv;
                    if constexpr (STAGED) xv = x[r * xstep + jj + u];
                    else {
                        const long i = (long)irel + i_lo + (long)r * xstep + jj + u;
                        xv = i >= 0 && i < sp.n ? load_sample<IN>(in, ib + (long)r * xstep + jj + u) : 0.0f;
                    }
                    acc[r] = __builtin_fmaf(xv, h[u], acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) ys[q + r * ostep] = acc[r];
    }
    __syncthreads();
    store_tile(ys, out + sp.out_off + k0, cnt);
}

// up == down == 1: the samples themselves (float: bit for bit; int16: decoded)
template <int IN>
__global__ __launch_bounds__(kThreads) void resample_copy_kernel(const void *__restrict__ in, const ResampleSpan *__restrict__ spans, long n_rec,
                                                                 long tile_base, int tile, float *__restrict__ out)
{
    const long t = tile_base + blockIdx.x;
    const ResampleSpan sp = spans[owner_of_tile(spans, n_rec, t)];
    const long k0 = (t - sp.tile0) * tile;
    const long left = sp.n_out - k0;
    const int cnt = left < tile ? (int)left : tile;
    for (int k = threadIdx.x; k < cnt; k += kThreads) {
        if constexpr (IN == 0) {
            const unsigned bits = static_cast<const unsigned *>(in)[sp.in_off + k0 + k];
            reinterpret_cast<unsigned *>(out)[sp.out_off + k0 + k] = bits;
        } else out[sp.out_off + k0 + k] = load_sample<IN>(in, sp.in_off + k0 + k);
    }
}

template <int IN>
void launch_one(const void *in, const ResampleSpan *spans, long n_rec, long base, unsigned blocks, const ResampleShape &s, const float *taps,
                float *out, hipStream_t stream)
{
    if (s.up == 1 && s.down == 1)
        hipLaunchKernelGGL(resample_copy_kernel<IN>, dim3(blocks), dim3(kThreads), 0, stream, in, spans, n_rec, base, s.tile, out);
    else if (!s.staged)
        hipLaunchKernelGGL((resample_kernel<IN, false, false>), dim3(blocks), dim3(kThreads), (size_t)s.lds_bytes, stream, in, spans, n_rec, base, s, taps, out);
    else if (s.up == 1)
        hipLaunchKernelGGL((resample_kernel<IN, true, true>), dim3(blocks), dim3(kThreads), (size_t)s.lds_bytes, stream, in, spans, n_rec, base, s, taps, out);
    else
        hipLaunchKernelGGL((resample_kernel<IN, true, false>), dim3(blocks), dim3(kThreads), (size_t)s.lds_bytes, stream, in, spans, n_rec, base, s, taps, out);
}

// ---- live streams: the same outputs from a feed that arrives in chunks ----
// A block takes `tile` consecutive NEW outputs of one stream, counted from the first output of the push.  What differs from
// resample_kernel is the stage alone: the samples come from the stream's carry (frame by frame: it is short and lies wherever its slot
// does) and then from the chunk (aligned 16-byte loads for its interior), zeros before the carry's first sample and past the last
// received one.  The filter loop and the store restate resample_kernel<IN, true, UP1>'s: the same taps, the same jj order, the same FMA.
template <int IN, bool UP1>
__global__ __launch_bounds__(kThreads) void resample_stream_kernel(const void *__restrict__ carry, const void *__restrict__ chunks,
                                                                   const StreamResampleSpan *__restrict__ spans, long n_spans, long tile_base,
                                                                   ResampleShape s, const float *__restrict__ taps, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *ys = lds;                      // [tile]
    float *xs = lds + s.tile;             // [span + 16]
    const long t = tile_base + blockIdx.x;
    const StreamResampleSpan sp = spans[owner_of_tile(spans, n_spans, t)];
    const long kr = (t - sp.tile0) * s.tile;                      // the tile's first output, counted from the span's first
    const long a0 = (sp.k0 + kr) * s.down + s.half;
    const long i0 = a0 / s.up;
    const unsigned p0 = (unsigned)(a0 - i0 * s.up);
    const long i_lo = i0 - (s.taps - 1);                         // the first sample the tile's first output reads
    constexpr int ESZ = IN == 1 ? 2 : 4, EPC = 16 / ESZ;
    const long rel = sp.chunk_off - sp.n0;                        // sample i of the stream is sample frame rel + i of the chunk buffer
    const uintptr_t g = reinterpret_cast<uintptr_t>(chunks) + (uintptr_t)((rel + i_lo) * ESZ);
    const bool vec = g % ESZ == 0;                                 // (interleaved stereo at an odd int16: frame by frame)
    const unsigned shift = vec ? (unsigned)(g & 15) / ESZ : 0;     // xs[shift + d] = sample i_lo + d
    const int n16 = (int)(shift + s.span + EPC - 1) / EPC;
    for (int c = threadIdx.x; c < n16; c += kThreads) {
        const long first = i_lo - (long)shift + (long)c * EPC;
        float v[EPC];
        if (vec && first >= sp.n0 && first + EPC <= sp.n1) {       // a whole aligned 16 bytes of the chunk
            const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const char *>(chunks) + (rel + first) * ESZ);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (IN == 0) v[e] = __uint_as_float(w[e]);
                else if constexpr (IN == 1) {
                    v[2 * e] = (float)(int)(short)(w[e] & 0xffffu) * (1.0f / 32768.0f);
                    v[2 * e + 1] = (float)((int)w[e] >> 16) * (1.0f / 32768.0f);
                } else v[e] = decode_pair<IN>(w[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const long i = first + e;
                float x = 0.0f;
                if (i >= sp.n0) { if (i < sp.n1) x = load_sample<IN>(chunks, rel + i); }
                else if (i >= sp.c0) x = load_sample<IN>(carry, sp.carry_off + (i - sp.c0));
                v[e] = x;
            }
        }
#pragma unroll
        for (int e = 0; e < EPC; e += 4)
            *reinterpret_cast<float4 *>(xs + c * EPC + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
    }
    __syncthreads();
    const long left = sp.n_out - kr;                               // outputs of the span from the tile's first on (>= 1)
    const int cnt = left < s.tile ? (int)left : s.tile;
    for (int it = threadIdx.x; it < s.items; it += kThreads) {
        const int b = UP1 ? 0 : it / s.up;
        const int q = UP1 ? it : b * kR * s.up + (it - b * s.up);
        const int ostep = UP1 ? s.items : s.up, xstep = UP1 ? s.items * s.down : s.down;
        if (q >= cnt) continue;
        const unsigned w = (unsigned)q * (unsigned)s.down + p0;
        const unsigned irel = UP1 ? w : w / (unsigned)s.up;
        const unsigned p = UP1 ? 0u : w - irel * (unsigned)s.up;
        const float *row = taps + (size_t)p * s.row;
        float acc[kR] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float *x = xs + shift + irel;
        for (int jj = 0; jj < s.row; jj += 4) {
            const float4 h4 = *reinterpret_cast<const float4 *>(row + jj);
            const float h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int r = 0; r < kR; ++r) acc[r] = __builtin_fmaf(x[r * xstep + jj + u], h[u], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) ys[q + r * ostep] = acc[r];
    }
    __syncthreads();
    store_tile(ys, out + sp.out_off + kr, cnt);
}

template <int IN>
void launch_stream_one(const void *carry, const void *chunks, const StreamResampleSpan *spans, long n_spans, long base, unsigned blocks,
                       const ResampleShape &s, const float *taps, float *out, hipStream_t stream)
{
    if (s.up == 1)
        hipLaunchKernelGGL((resample_stream_kernel<IN, true>), dim3(blocks), dim3(kThreads), (size_t)s.lds_bytes, stream, carry, chunks, spans, n_spans, base, s, taps, out);
    else
        hipLaunchKernelGGL((resample_stream_kernel<IN, false>), dim3(blocks), dim3(kThreads), (size_t)s.lds_bytes, stream, carry, chunks, spans, n_spans, base, s, taps, out);
}

}  // namespace

hipError_t launch_resample_stream(const void *d_carry, const void *d_chunks, int in_kind, const StreamResampleSpan *d_spans, long n_spans,
                                  long total_tiles, const ResampleShape &s, const float *d_taps, float *d_out, hipStream_t stream)
{
    if (!s.staged || (s.up == 1 && s.down == 1)) return hipErrorInvalidValue;
    constexpr long kMaxBlocks = 1L << 30;
    for (long base = 0; base < total_tiles; base += kMaxBlocks) {
        const unsigned blocks = (unsigned)(total_tiles - base < kMaxBlocks ? total_tiles - base : kMaxBlocks);
        switch (in_kind) {
        case 0: launch_stream_one<0>(d_carry, d_chunks, d_spans, n_spans, base, blocks, s, d_taps, d_out, stream); break;
        case 1: launch_stream_one<1>(d_carry, d_chunks, d_spans, n_spans, base, blocks, s, d_taps, d_out, stream); break;
        case 2: launch_stream_one<2>(d_carry, d_chunks, d_spans, n_spans, base, blocks, s, d_taps, d_out, stream); break;
        case 3: launch_stream_one<3>(d_carry, d_chunks, d_spans, n_spans, base, blocks, s, d_taps, d_out, stream); break;
        default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_resample(const void *d_in, int in_kind, const ResampleSpan *d_spans, long n_rec, long total_tiles, const ResampleShape &s,
                           const float *d_taps, float *d_out, hipStream_t stream)
{
    constexpr long kMaxBlocks = 1L << 30;
    for (long base = 0; base < total_tiles; base += kMaxBlocks) {
        const unsigned blocks = (unsigned)(total_tiles - base < kMaxBlocks ? total_tiles - base : kMaxBlocks);
        switch (in_kind) {
        case 0: launch_one<0>(d_in, d_spans, n_rec, base, blocks, s, d_taps, d_out, stream); break;
        case 1: launch_one<1>(d_in, d_spans, n_rec, base, blocks, s, d_taps, d_out, stream); break;
        case 2: launch_one<2>(d_in, d_spans, n_rec, base, blocks, s, d_taps, d_out, stream); break;
        case 3: launch_one<3>(d_in, d_spans, n_rec, base, blocks, s, d_taps, d_out, stream); break;
        default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dsp
