// enroll_kernels.hip -- sliding CMVN of a ragged MFCC matrix and MAP enrolment of speakers against a float UBM.
//
// CMVN (sliding_cmvn of the reference's speaker/gmm_utils.py): row t of a recording of n rows is normalised by the mean and the population
// standard deviation of rows [max(0, t - half), min(n, t + half)), half = window / 2, per coefficient, in the two-pass form:
//   mu = sum x / c,  sigma = sqrt(sum (x - mu)^2 / c),  y = (x[t] - mu) / (sigma + 1e-8)
// A block takes kCmvnTileRows consecutive rows of one recording and stages them and `half` rows each side in LDS; a lane takes one
// (row, coefficient) and runs both passes from LDS in ascending row order, float32.  Nothing a row reads lies outside its recording.
//
// Enrolment (map_adapt_gmm of the reference's adapt_ubm.py scripts, means only): per row the posteriors of the k components under the
// UBM, per speaker N_k = sum_t p_k and F_k = sum_t p_k x, then mean_k = alpha_k F_k / N'_k + (1 - alpha_k) mu_k.
//   statistics  one block per chunk of kEnrollChunkRows rows of one speaker.  The E-step is gmm_estep.hpp's: lane k of a wave owns
//               component k and the accumulators N_k, F_k[d] in registers; the four waves take interleaved rows of the chunk from an LDS
//               image and combine through LDS in wave order.  The chunk's partial goes to the workspace with plain stores: no atomics
//               anywhere.
//   finalise    one block per speaker sums its chunks' partials in ascending chunk order in float64 and does the MAP update, the Q6
//               rounding, the saturation count and the mean of ll.
// The chunks of a speaker depend on its own row count alone and every sum has a fixed order, so a speaker's outputs are the same bits
// whatever the batch around it.
//
// Out of scope: variance or weight adaptation (the UBM itself is trained by ubm_kernels.hip); the n_fft-400 librosa front end (these kernels take whatever MFCC
// matrix the existing entries wrote and leave every front end alone); CMVN inside scanners or stream sessions (a stream needs a 150-row
// look-ahead); the float log-sum-exp scorer (verify_kernels.hip); CMVN fused into the statistics pass.  No existing speaker scoring entry, nor any result of
// one, changes: the enrolled Q6 means go to dsp_speaker_model_create as any other target's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "enroll_kernels.hpp"
#include "gmm_estep.hpp"

namespace dsp {
namespace {

__global__ __launch_bounds__(kThreads) void cmvn_kernel(const float *__restrict__ in, const RowSpan *__restrict__ spans, long n_rec, long tile_base,
                                                        int d, int half, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];      // [shift + staged rows * d]
    const long t = tile_base + blockIdx.x;
    const RowSpan sp = spans[owner_of_unit(spans, n_rec, t)];
    const long t0 = (t - sp.unit0) * kCmvnTileRows;                 // the tile's first row within the recording (< n)
    const long lo = t0 - half > 0 ? t0 - half : 0;
    const long hi = t0 + kCmvnTileRows + half < sp.n ? t0 + kCmvnTileRows + half : sp.n;
    const float *src = in + (sp.row0 + lo) * d;
    const int total = (int)(hi - lo) * d;                           // <= (kCmvnTileRows + 2 half) * d floats
    // 16-byte loads of the aligned chunks that lie wholly inside the staged rows, single floats at both ends: xs[shift + i] = src[i]
    const int shift = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    const int chunks = (shift + total + 3) >> 2;
    for (int c = threadIdx.x; c < chunks; c += kThreads) {
        const int first = 4 * c - shift;
        if (first >= 0 && first + 4 <= total) {
            *reinterpret_cast<float4 *>(xs + 4 * c) = *reinterpret_cast<const float4 *>(src + first);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (first + e >= 0 && first + e < total) xs[4 * c + e] = src[first + e];
        }
    }
    __syncthreads();
    const long left = sp.n - t0;
    const int rows = left < kCmvnTileRows ? (int)left : kCmvnTileRows;
    float *o = out + (sp.row0 + t0) * d;
    for (int it = threadIdx.x; it < rows * d; it += kThreads) {
        const int r = it / d, j = it - r * d;
        const long row = t0 + r;
        const long s = row - half > 0 ? row - half : 0;
        const long e = row + half < sp.n ? row + half : sp.n;
        const int cnt = (int)(e - s);                               // >= 1: half >= 1
        const float *p = xs + shift + (int)(s - lo) * d + j;
        const float fc = (float)cnt;
        float sum = 0.0f;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) sum += p[i * d];
        const float mu = sum / fc;
        float var = 0.0f;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const float dv = p[i * d] - mu;
            var = __builtin_fmaf(dv, dv, var);
        }
        const float sigma = sqrtf(var / fc);
        o[it] = (xs[shift + (int)(row - lo) * d + j] - mu) / (sigma + 1e-8f);
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void enroll_stats_kernel(const float *__restrict__ feats, const RowSpan *__restrict__ spans, long n_spk,
                                                                long chunk_base, GmmModel ubm, float *__restrict__ partials)
{
    constexpr int W = kThreads / 64, P = 64 * (D + 1);
    __shared__ __attribute__((aligned(16))) float xs[kEnrollChunkRows * kRowLd];
    __shared__ float part[W * P];                                    // per wave: [lane][D + 1]
    __shared__ double ll_part[W];                                    // per wave: its rows' sum of ll (wave-uniform, kept in float64)
    const long c = chunk_base + blockIdx.x;
    const RowSpan sp = spans[owner_of_unit(spans, n_spk, c)];
    const long r0 = (c - sp.unit0) * kEnrollChunkRows;
    const long left = sp.n - r0;
    const int cnt = left < kEnrollChunkRows ? (int)left : kEnrollChunkRows;
    stage_rows<D>(xs, feats + (sp.row0 + r0) * D, cnt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = ubm.k;
    const LaneGmm<D> g(ubm, lane);
    float N = 0.0f, F[D];
#pragma unroll
    for (int j = 0; j < D; ++j) F[j] = 0.0f;
    double ll_sum = 0.0;
    __syncthreads();
    for (int r = wave; r < cnt; r += W) {
        float x[4 * ((D + 3) / 4)], ll;
        const float p = row_posterior<D>(xs, r, g, x, ll);
        ll_sum += (double)ll;
        N += p;
#pragma unroll
        for (int j = 0; j < D; ++j) F[j] = __builtin_fmaf(p, x[j], F[j]);
    }
    float *mine = part + wave * P + lane * (D + 1);
    mine[0] = N;
#pragma unroll
    for (int j = 0; j < D; ++j) mine[1 + j] = F[j];
    if (lane == 0) ll_part[wave] = ll_sum;
    __syncthreads();
    float *dst = partials + (size_t)c * ((size_t)k * (D + 1) + 1);
    const int n_stats = k * (D + 1);
    for (int i = threadIdx.x; i < n_stats; i += kThreads) dst[i] = sum_waves(part, P, i);
    if (threadIdx.x == 0) dst[n_stats] = (float)sum_waves(ll_part, 1, 0);
}

__global__ __launch_bounds__(kThreads) void enroll_finalize_kernel(const RowSpan *__restrict__ spans, GmmModel ubm, const float *__restrict__ partials,
                                                                   int map_fixed, float param, float *__restrict__ means, int8_t *__restrict__ means_q6,
                                                                   float *__restrict__ counts, float *__restrict__ ll_mean, int *__restrict__ saturated)
{
    __shared__ double sums[kGmmMaxK * (kGmmMaxD + 1) + 1];
    __shared__ int clamped;
    const long spk = blockIdx.x;
    const RowSpan sp = spans[spk];
    const int k = ubm.k, d = ubm.d, n_stats = k * (d + 1);
    const long n_chunks = (sp.n + kEnrollChunkRows - 1) / kEnrollChunkRows;
    const float *src = partials + (size_t)sp.unit0 * (size_t)(n_stats + 1);
    if (threadIdx.x == 0) clamped = 0;
    sum_partials(src, n_chunks, (size_t)(n_stats + 1), n_stats + 1, sums);      // ascending chunk
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < k * d; i += kThreads) {
        const int kk = i / d, j = i - kk * d;
        const double n1 = sums[kk * (d + 1)] + 1e-8;
        const double alpha = map_fixed ? (double)param : n1 / (n1 + (double)param);
        const double mean = alpha * (sums[kk * (d + 1) + 1 + j] / n1) + (1.0 - alpha) * (double)ubm.means()[i];
        const float mean32 = (float)mean;
        const size_t at = (size_t)spk * (size_t)(k * d) + i;
        if (means) means[at] = mean32;
        const float q = rintf(mean32 * 64.0f);                        // ties to even
        mine += q < -128.0f || q > 127.0f;
        if (means_q6) means_q6[at] = (int8_t)(int)fminf(fmaxf(q, -128.0f), 127.0f);
    }
    if (counts)
        for (int kk = threadIdx.x; kk < k; kk += kThreads) counts[(size_t)spk * k + kk] = (float)sums[kk * (d + 1)];
    if (threadIdx.x == 0 && ll_mean) ll_mean[spk] = (float)(sums[n_stats] / (double)sp.n);
    if (saturated) {
        if (mine) atomicAdd(&clamped, mine);                          // (an integer count in LDS: any order, one value)
        __syncthreads();
        if (threadIdx.x == 0) saturated[spk] = clamped;
    }
}

}  // namespace

hipError_t prepare_cmvn()
{
    // images above 64 KiB (windows from about 960 rows at d = 16) need the kernel's dynamic LDS limit raised: to the widest image, the
    // rows and the 4 floats of the alignment shift.  Idempotent, per device.
    constexpr int kMaxLds = ((kCmvnTileRows + kCmvnMaxWindow) * kGmmMaxD + 4) * 4;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(cmvn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
}

hipError_t launch_cmvn(const float *d_in, const RowSpan *d_spans, long n_rec, long total_tiles, int d, int window, float *d_out, hipStream_t stream)
{
    constexpr long kMaxBlocks = 1L << 30;
    if (d < 1 || d > kGmmMaxD || window < 2 || window > kCmvnMaxWindow) return hipErrorInvalidValue;
    const int half = window / 2;
    const size_t lds = ((size_t)(kCmvnTileRows + 2 * half) * d + 4) * 4;
    for (long base = 0; base < total_tiles; base += kMaxBlocks) {
        const unsigned blocks = (unsigned)(total_tiles - base < kMaxBlocks ? total_tiles - base : kMaxBlocks);
        hipLaunchKernelGGL(cmvn_kernel, dim3(blocks), dim3(kThreads), lds, stream, d_in, d_spans, n_rec, base, d, half, d_out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_enroll(const float *d_feats, const RowSpan *d_spans, long n_speakers, long total_chunks, const GmmModel &ubm, float *d_partials,
                         int map_fixed, float param, float *d_means, int8_t *d_means_q6, float *d_counts, float *d_ll_mean, int *d_saturated,
                         hipStream_t stream)
{
    constexpr long kMaxBlocks = 1L << 30;
    if (ubm.k < 1 || ubm.k > kGmmMaxK || n_speakers > kMaxBlocks) return hipErrorInvalidValue;
    for (long base = 0; base < total_chunks; base += kMaxBlocks) {
        const unsigned blocks = (unsigned)(total_chunks - base < kMaxBlocks ? total_chunks - base : kMaxBlocks);
        const hipError_t e = dispatch_d(ubm.d, [&](auto dc) {
            hipLaunchKernelGGL(enroll_stats_kernel<decltype(dc)::value>, dim3(blocks), dim3(kThreads), 0, stream, d_feats, d_spans, n_speakers, base, ubm, d_partials);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(enroll_finalize_kernel, dim3((unsigned)n_speakers), dim3(kThreads), 0, stream, d_spans, ubm, d_partials, map_fixed, param, d_means,
                       d_means_q6, d_counts, d_ll_mean, d_saturated);
    return hipGetLastError();
}

}  // namespace dsp
