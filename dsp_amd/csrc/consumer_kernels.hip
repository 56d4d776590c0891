// consumer_kernels.hip -- gfx950 kernels for the consumers of the MFCC matrix and the resampler.
// All three are tiny next to the MFCC chain (a 98 x 13 matrix per clip); they exist so that a clip
// goes from PCM to its decision without leaving HBM.
#include <hip/hip_runtime.h>

#include "consumer_kernels.hpp"
#include "scan_device.hpp"

#pragma clang fp contract(off)

namespace dsp {

// ---- stop-word net ---------------------------------------------------------------------------
// The reference standardises all n_coef * max_frames inputs and sums layer 1 sequentially in fp32
// (audio_classifier_inference.c:25-33).  Here a wave sums only the T x n_coef live inputs (float64
// partial sums, so the result does not depend on the lane split); the zero-padded inputs t >= T
// contribute a constant per T that the host precomputed in float64 (StopModelDev::pad).  Layers 2-4
// (<= 16 units) run on lane 0 in the reference's order.
__global__ __launch_bounds__(256) void stop_tail_kernel(const StopModelDev m, const float *__restrict__ mfcc, long n_clips, int T,
                                                        float *__restrict__ prob)
{
    const int lane = threadIdx.x & 63;
    const long clip = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (clip >= n_clips) return;
    const int u1 = m.units[0];
    const int Tc = T < m.max_frames ? T : m.max_frames;          // stop_detector.c:26-30
    const float *x = mfcc + clip * (long)T * m.n_coef;
    double acc[kStopMaxUnits];
#pragma unroll
    for (int j = 0; j < kStopMaxUnits; ++j) acc[j] = 0.0;
    const int live = Tc * m.n_coef;
    for (int p = lane; p < live; p += 64) {
        const int t = p / m.n_coef, c = p - t * m.n_coef;
        const int i = c * m.max_frames + t;                     // stop_detector.c:48: coefficient-major index
        const float xs = (x[p] - m.mean[i]) / m.div[i];     // audio_classifier_inference.c:46
        const float *w = m.kernel[0] + (long)i * u1;
#pragma unroll
        for (int j = 0; j < kStopMaxUnits; ++j)
            if (j < u1) acc[j] += (double)w[j] * (double)xs;
    }
#pragma unroll
    for (int j = 0; j < kStopMaxUnits; ++j)
        for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o);
    if (lane != 0) return;
    float h[2][kStopMaxUnits];
    for (int j = 0; j < u1; ++j) {
        const float s = (float)((double)m.bias[0][j] + m.pad[(long)Tc * u1 + j] + acc[j]);
        h[0][j] = s > 0.0f ? s : 0.0f;
    }
    int n_in = u1;
    for (int l = 1; l < 4; ++l) {                                // dense_forward, :18-35
        const int n_out = m.units[l];
        const float *src = h[(l - 1) & 1];
        float *dst = h[l & 1];
        for (int j = 0; j < n_out; ++j) {
            float s = m.bias[l][j];
            for (int i = 0; i < n_in; ++i) s = s + m.kernel[l][i * n_out + j] * src[i];
            dst[j] = (l < 3 && !(s > 0.0f)) ? 0.0f : s;
        }
        n_in = n_out;
    }
    prob[clip] = 1.0f / (1.0f + expf(-h[1][0]));                 // :13-15
}

hipError_t launch_stop_tail(const StopModelDev &m, const float *mfcc, long n_clips, int T, float *prob, hipStream_t stream)
{
    if (n_clips <= 0) return hipSuccess;
    for (int l = 0; l < 4; ++l)
        if (m.units[l] <= 0 || m.units[l] > kStopMaxUnits) return hipErrorInvalidValue;
    if (T < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stop_tail_kernel, dim3((unsigned)((n_clips + 3) / 4)), dim3(256), 0, stream, m, mfcc, n_clips, T, prob);
    return hipGetLastError();
}

// ---- speaker GMM -------------------------------------------------------------------------------
// Integer path, bit-exact: x Q6 = (int16)(x * 64) (speaker_gmm.c:118-122), per mixture
// sum_d (x - mean)^2 * inv_cov in int64 (Q23), >> 15, / 2, log_const - that, max over mixtures (:29-50).
constexpr int kGmmMaxD = 16, kGmmMaxK = 64;

struct GmmLds {
    int8_t means[kGmmMaxK * kGmmMaxD];
    int32_t inv_covs[kGmmMaxK * kGmmMaxD];
    int16_t log_consts[kGmmMaxK];
};

__device__ __forceinline__ long long gmm_ll(const GmmLds &g, int k_n, int d_n, const int (&x)[kGmmMaxD])
{
    long long best = LLONG_MIN;
    for (int k = 0; k < k_n; ++k) {
        long long sum_sq = 0;
#pragma unroll
        for (int d = 0; d < kGmmMaxD; ++d) {
            if (d < d_n) {
                const int diff = x[d] - (int)g.means[k * d_n + d];            // |diff| < 2^16
                sum_sq += (long long)diff * (long long)diff * (long long)g.inv_covs[k * d_n + d];
            }
        }
        sum_sq >>= 15;
        sum_sq /= 2;
        const long long term = (long long)g.log_consts[k] - sum_sq;
        best = term > best ? term : best;
    }
    return best;
}

__global__ __launch_bounds__(256) void speaker_llr_kernel(const GmmDev target, const GmmDev ubm, const float *__restrict__ mfcc,
                                                          long n_clips, int T, long long threshold, long long *__restrict__ llr_mean,
                                                          int *__restrict__ labels, long long *__restrict__ ll_target,
                                                          long long *__restrict__ ll_ubm)
{
    __shared__ GmmLds gt, gu;
    for (int i = threadIdx.x; i < target.k * target.d; i += 256) {
        gt.means[i] = target.means[i]; gt.inv_covs[i] = target.inv_covs[i];
        gu.means[i] = ubm.means[i]; gu.inv_covs[i] = ubm.inv_covs[i];
    }
    for (int i = threadIdx.x; i < target.k; i += 256) { gt.log_consts[i] = target.log_consts[i]; gu.log_consts[i] = ubm.log_consts[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long clip = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (clip >= n_clips) return;
    const int d_n = target.d;
    long long sum = 0;
    for (int t = lane; t < T; t += 64) {
        const float *f = mfcc + (clip * (long)T + t) * d_n;
        int x[kGmmMaxD];
#pragma unroll
        for (int d = 0; d < kGmmMaxD; ++d) x[d] = d < d_n ? (int)(short)(int)(f[d] * 64.0f) : 0;   // low 16 bits of the int32 truncation
        const long long lt = gmm_ll(gt, target.k, d_n, x), lu = gmm_ll(gu, ubm.k, d_n, x);
        if (ll_target) ll_target[clip * (long)T + t] = lt;
        if (ll_ubm) ll_ubm[clip * (long)T + t] = lu;
        sum += lt - lu;                                                                           // :104-108
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) {
        const long long mean = sum / (long long)T;                                                // :135
        llr_mean[clip] = mean;
        if (labels) labels[clip] = mean > threshold ? 1 : 0;                                      // :138-141
    }
}

hipError_t launch_speaker_llr(const GmmDev &target, const GmmDev &ubm, const float *mfcc, long n_clips, int T,
                              long long threshold, long long *llr_mean, int *labels, long long *ll_target,
                              long long *ll_ubm, hipStream_t stream)
{
    if (n_clips <= 0) return hipSuccess;
    if (T <= 0 || target.d != ubm.d || target.k != ubm.k || target.d > kGmmMaxD || target.k > kGmmMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(speaker_llr_kernel, dim3((unsigned)((n_clips + 3) / 4)), dim3(256), 0, stream, target, ubm, mfcc, n_clips, T,
                       threshold, llr_mean, labels, ll_target, ll_ubm);
    return hipGetLastError();
}

// ragged MFCC matrix (dsp_mfcc_clips_ragged_device): clip c is rows [frame_offsets[c], frame_offsets[c + 1]) of mfcc, every clip >= 1 row
// (the host checked); one wave per clip, the same integer arithmetic and truncating mean as speaker_llr_kernel, per-frame outputs by row
__global__ __launch_bounds__(256) void speaker_llr_ragged_kernel(const GmmDev target, const GmmDev ubm, const float *__restrict__ mfcc,
                                                                 long n_clips, const long *__restrict__ frame_offsets, long long threshold,
                                                                 long long *__restrict__ llr_mean, int *__restrict__ labels,
                                                                 long long *__restrict__ ll_target, long long *__restrict__ ll_ubm)
{
    __shared__ GmmLds gt, gu;
    for (int i = threadIdx.x; i < target.k * target.d; i += 256) {
        gt.means[i] = target.means[i]; gt.inv_covs[i] = target.inv_covs[i];
        gu.means[i] = ubm.means[i]; gu.inv_covs[i] = ubm.inv_covs[i];
    }
    for (int i = threadIdx.x; i < target.k; i += 256) { gt.log_consts[i] = target.log_consts[i]; gu.log_consts[i] = ubm.log_consts[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long clip = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (clip >= n_clips) return;
    const int d_n = target.d;
    const long r0 = frame_offsets[clip], r1 = frame_offsets[clip + 1];
    long long sum = 0;
    for (long r = r0 + lane; r < r1; r += 64) {
        const float *f = mfcc + r * d_n;
        int x[kGmmMaxD];
#pragma unroll
        for (int d = 0; d < kGmmMaxD; ++d) x[d] = d < d_n ? (int)(short)(int)(f[d] * 64.0f) : 0;   // low 16 bits of the int32 truncation
        const long long lt = gmm_ll(gt, target.k, d_n, x), lu = gmm_ll(gu, ubm.k, d_n, x);
        if (ll_target) ll_target[r] = lt;
        if (ll_ubm) ll_ubm[r] = lu;
        sum += lt - lu;                                                                           // :104-108
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) {
        const long long mean = sum / (long long)(r1 - r0);                                        // :135
        llr_mean[clip] = mean;
        if (labels) labels[clip] = mean > threshold ? 1 : 0;                                      // :138-141
    }
}

hipError_t launch_speaker_llr_ragged(const GmmDev &target, const GmmDev &ubm, const float *mfcc, long n_clips, const long *frame_offsets,
                                     long long threshold, long long *llr_mean, int *labels, long long *ll_target, long long *ll_ubm,
                                     hipStream_t stream)
{
    if (n_clips <= 0) return hipSuccess;
    if (target.d != ubm.d || target.k != ubm.k || target.d > kGmmMaxD || target.k > kGmmMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(speaker_llr_ragged_kernel, dim3((unsigned)((n_clips + 3) / 4)), dim3(256), 0, stream, target, ubm, mfcc, n_clips,
                       frame_offsets, threshold, llr_mean, labels, ll_target, ll_ubm);
    return hipGetLastError();
}

// ---- linear resampler ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void upsample_linear_kernel(const float *__restrict__ in, long n_clips, int old_size, long in_stride,
                                                              float *__restrict__ out, int new_size, long out_stride)
{
    const long clip = blockIdx.y;
    const float step = (float)(old_size - 1) / (float)(new_size - 1);       // main.cpp:66
    const float *src = in + clip * in_stride;
    float *dst = out + clip * out_stride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < new_size; i += gridDim.x * 256) {
        const float old_index = (float)i * step;
        const int lo = (int)floorf(old_index);
        const int hi = lo == old_size - 1 ? old_size - 1 : lo + 1;
        const float frac = old_index - (float)lo;
        const float a = src[lo], b = src[hi];
        dst[i] = a + (b - a) * frac;
    }
}

hipError_t launch_upsample_linear(const float *in, long n_clips, int old_size, long in_stride, float *out, int new_size,
                                  long out_stride, hipStream_t stream)
{
    if (n_clips <= 0 || new_size <= 0) return hipSuccess;
    if (old_size < 1 || new_size < 2 || n_clips > 65535) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((new_size + 255) / 256 < 64 ? (new_size + 255) / 256 : 64);
    hipLaunchKernelGGL(upsample_linear_kernel, dim3(gx, (unsigned)n_clips), dim3(256), 0, stream, in, n_clips, old_size, in_stride, out,
                       new_size, out_stride);
    return hipGetLastError();
}

// ---- fft_real_forward (2fa/audio/word/c/mfcc.c:16-95) as its own entry point -------------------------------------------------
// The reference's non-static helper: frame_length real samples, zero-padded to n_fft, forward transform, ALL n_fft complex bins
// interleaved [re, im].  Inside compute_mfcc the transform lives in the MFCC kernels' registers (mfcc_kernels.hip); this batch kernel
// serves callers that link the symbol itself: one 256-thread block per frame, radix-2 Stockham through LDS (9 passes at n_fft = 512),
// twiddles from sincospif (the reference runs a float32 recurrence; the gate is 1e-4 of the frame's L-inf norm, as for the MFCCs).
__global__ __launch_bounds__(256) void fft_real_forward_kernel(const float *__restrict__ in, long n_frames, int frame_length, long in_stride, int n_fft,
                                                               float *__restrict__ out)
{
    extern __shared__ float2 fbuf[];                       // [2][n_fft]
    const long fr = blockIdx.x;
    if (fr >= n_frames) return;
    float2 *a = fbuf, *b = fbuf + n_fft;
    for (int i = threadIdx.x; i < n_fft; i += 256) a[i] = make_float2(i < frame_length ? in[fr * in_stride + i] : 0.0f, 0.0f);
    __syncthreads();
    for (int ns = 1; ns < n_fft; ns <<= 1) {               // butterfly j: k = j % ns, inputs x[j], x[j + n/2] W_{2 ns}^k, outputs y[(j - k) 2 + k], + ns
        for (int j = threadIdx.x; j < n_fft / 2; j += 256) {
            const int k = j % ns;
            float sn, cs;
            sincospif(-(float)k / (float)ns, &sn, &cs);
            const float2 u = a[j], v = a[j + n_fft / 2];
            const float2 t = make_float2(v.x * cs - v.y * sn, v.x * sn + v.y * cs);
            const int o = (j - k) * 2 + k;
            b[o] = make_float2(u.x + t.x, u.y + t.y);
            b[o + ns] = make_float2(u.x - t.x, u.y - t.y);
        }
        __syncthreads();
        float2 *sw = a; a = b; b = sw;
    }
    for (int i = threadIdx.x; i < n_fft; i += 256) reinterpret_cast<float2 *>(out)[fr * n_fft + i] = a[i];
}

hipError_t launch_fft_real_forward(const float *in, long n_frames, int frame_length, long in_stride, int n_fft, float *out, hipStream_t stream)
{
    if (n_frames <= 0) return hipSuccess;
    if (n_fft < 2 || (n_fft & (n_fft - 1)) || n_fft > 4096 || frame_length < 0 || frame_length > n_fft || n_frames >= (1L << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fft_real_forward_kernel, dim3((unsigned)n_frames), dim3(256), (size_t)2 * n_fft * sizeof(float2), stream, in, n_frames, frame_length,
                       in_stride, n_fft, out);
    return hipGetLastError();
}

// ---- scanning long recordings (dsp_stop_scan_device, dsp_speaker_scan_device) ----------------------------------------------------
// Recording r is rows [fo[r], fo[r + 1]) of a ragged MFCC matrix; its windows are wo[r] .. wo[r + 1) of the scan (host planner,
// capi_consumers.cpp).  Window w of a recording with R >= window_frames rows covers rows [w hop, w hop + window_frames); a recording with
// fewer rows has one window over all of them.  Only these per-recording arrays travel to the GPU: a block or a wave finds its recording
// by a uniform binary search (scan_find, scan_device.hpp).

// Stop-word net over windows.  One block of 256 threads per tile of TW consecutive windows of one recording (tiles per recording
// to[r] .. to[r + 1)): the rows the tile's windows cover are staged in LDS once, then thread (slot = tid % TW, stripe = tid / TW) sums
// layer 1 of window slot over the inputs p = stripe, stripe + 256 / TW, ... -- the same per-input arithmetic as stop_tail_kernel
// (fl((x - mean) / div), float64 products and partial sums, pad[Tc]), the partial sums added in stripe order through LDS.  With TW = 64
// a wave's 64 lanes are 64 windows at one input position, so mean / div / W1 are wave-uniform (scalar) loads.  Layers 2-4 and the
// sigmoid on thread `slot` in stop_tail_kernel's order.
template <int TW>
__global__ __launch_bounds__(256) void stop_scan_kernel(const StopModelDev m, const float *__restrict__ mfcc, long n_rec, const long *__restrict__ fo,
                                                        const long *__restrict__ wo, const long *__restrict__ to, int window_frames, int hop,
                                                        float *__restrict__ prob)
{
    extern __shared__ double scan_lds[];
    float *rows = reinterpret_cast<float *>(scan_lds);
    const long r = scan_find(to, n_rec, (long)blockIdx.x);
    const long w0 = ((long)blockIdx.x - to[r]) * TW;
    const long n_win = wo[r + 1] - wo[r];
    const int nw = (int)(n_win - w0 < TW ? n_win - w0 : TW);
    const long n_rows = fo[r + 1] - fo[r];
    const int len = n_rows < window_frames ? (int)n_rows : window_frames;
    const int Tc = len < m.max_frames ? len : m.max_frames;                // stop_detector.c:26-30
    const int nc = m.n_coef, u1 = m.units[0];
    // stage rows [w0 hop, w0 hop + (nw - 1) hop + Tc) of the recording: inside it (the planner's window count)
    const long n_stage = ((long)(nw - 1) * hop + Tc) * nc;
    const float *src = mfcc + (fo[r] + w0 * hop) * nc;
    for (long i = threadIdx.x; i < n_stage; i += 256) rows[i] = src[i];
    __syncthreads();
    const int slot = (int)threadIdx.x % TW;
    const int stripe = TW == 64 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / TW) : (int)threadIdx.x / TW;
    constexpr int S = 256 / TW;
    double acc[kStopMaxUnits];
#pragma unroll
    for (int j = 0; j < kStopMaxUnits; ++j) acc[j] = 0.0;
    if (slot < nw) {
        const float *x = rows + (long)slot * hop * nc;
        const int live = Tc * nc;
        for (int p = stripe; p < live; p += S) {
            const int t = p / nc, c = p - t * nc;
            const int i = c * m.max_frames + t;                          // stop_detector.c:48: coefficient-major index
            const float xs = (x[p] - m.mean[i]) / m.div[i];              // audio_classifier_inference.c:46
            const float *w = m.kernel[0] + (long)i * u1;
#pragma unroll
            for (int j = 0; j < kStopMaxUnits; ++j)
                if (j < u1) acc[j] += (double)w[j] * (double)xs;
        }
    }
    __syncthreads();                                                     // the rows are dead: the same LDS takes the partial sums
    double *part = scan_lds;                                             // [S][TW][u1]
    for (int j = 0; j < u1; ++j) part[((long)stripe * TW + slot) * u1 + j] = acc[j];
    __syncthreads();
    if ((int)threadIdx.x >= nw) return;
    float h[2][kStopMaxUnits];
    for (int j = 0; j < u1; ++j) {
        double a = 0.0;
        for (int s = 0; s < S; ++s) a += part[((long)s * TW + threadIdx.x) * u1 + j];
        const float v = (float)((double)m.bias[0][j] + m.pad[(long)Tc * u1 + j] + a);
        h[0][j] = v > 0.0f ? v : 0.0f;
    }
    int n_in = u1;
    for (int l = 1; l < 4; ++l) {                                        // dense_forward, :18-35
        const int n_out = m.units[l];
        const float *in = h[(l - 1) & 1];
        float *out = h[l & 1];
        for (int j = 0; j < n_out; ++j) {
            float s = m.bias[l][j];
            for (int i = 0; i < n_in; ++i) s = s + m.kernel[l][i * n_out + j] * in[i];
            out[j] = (l < 3 && !(s > 0.0f)) ? 0.0f : s;
        }
        n_in = n_out;
    }
    prob[wo[r] + w0 + threadIdx.x] = 1.0f / (1.0f + expf(-h[1][0]));   // :13-15
}

// LDS bytes of a tile of tw windows: its rows, or the partial sums after them
static long stop_scan_lds(const StopModelDev &m, int window_frames, int hop, int tw)
{
    const long len = window_frames < m.max_frames ? window_frames : m.max_frames;
    const long row_bytes = ((long)(tw - 1) * hop + len) * m.n_coef * (long)sizeof(float);
    const long part_bytes = 256L * m.units[0] * (long)sizeof(double);
    return row_bytes > part_bytes ? row_bytes : part_bytes;
}

int stop_scan_tile(const StopModelDev &m, int window_frames, int hop)
{
    for (int tw : {64, 16, 4, 1})
        if (stop_scan_lds(m, window_frames, hop, tw) <= kScanLdsBytes) return tw;
    return 0;
}

hipError_t launch_stop_scan(const StopModelDev &m, const float *mfcc, long n_rec, const long *fo, const long *wo, const long *to, long n_tiles,
                            int window_frames, int hop, int tw, float *prob, hipStream_t stream)
{
    if (n_tiles <= 0) return hipSuccess;
    for (int l = 0; l < 4; ++l)
        if (m.units[l] <= 0 || m.units[l] > kStopMaxUnits) return hipErrorInvalidValue;
    if (window_frames < 1 || hop < 1 || n_tiles >= (1L << 31) || tw != stop_scan_tile(m, window_frames, hop)) return hipErrorInvalidValue;
    const size_t lds = (size_t)stop_scan_lds(m, window_frames, hop, tw);
    const dim3 grid((unsigned)n_tiles), block(256);
    switch (tw) {
    case 64: hipLaunchKernelGGL(stop_scan_kernel<64>, grid, block, lds, stream, m, mfcc, n_rec, fo, wo, to, window_frames, hop, prob); break;
    case 16: hipLaunchKernelGGL(stop_scan_kernel<16>, grid, block, lds, stream, m, mfcc, n_rec, fo, wo, to, window_frames, hop, prob); break;
    case 4: hipLaunchKernelGGL(stop_scan_kernel<4>, grid, block, lds, stream, m, mfcc, n_rec, fo, wo, to, window_frames, hop, prob); break;
    default: hipLaunchKernelGGL(stop_scan_kernel<1>, grid, block, lds, stream, m, mfcc, n_rec, fo, wo, to, window_frames, hop, prob); break;
    }
    return hipGetLastError();
}

// Speaker LLR over windows: the per-row values v = LL_target - LL_ubm (gmm_ll, as speaker_llr_ragged_kernel) once per row, an inclusive
// scan of them in uint64 (wrapping: a window's difference of prefix sums is the int64 sum the reference accumulates, wrapped the same
// way, with no signed overflow here), then per window the truncating mean of that sum (speaker_gmm.c:135) and the label.
// Pass 1: block b scans rows [b kLlrScanChunk, (b + 1) kLlrScanChunk) -- loc[row] = inclusive sum within the chunk, chunk_sum[b] = its total.
__global__ __launch_bounds__(256) void speaker_rows_scan_kernel(const GmmDev target, const GmmDev ubm, const float *__restrict__ mfcc, long n_rows,
                                                                unsigned long long *__restrict__ loc, unsigned long long *__restrict__ chunk_sum)
{
    __shared__ GmmLds gt, gu;
    __shared__ unsigned long long wave_sum[4];
    for (int i = threadIdx.x; i < target.k * target.d; i += 256) {
        gt.means[i] = target.means[i]; gt.inv_covs[i] = target.inv_covs[i];
        gu.means[i] = ubm.means[i]; gu.inv_covs[i] = ubm.inv_covs[i];
    }
    for (int i = threadIdx.x; i < target.k; i += 256) { gt.log_consts[i] = target.log_consts[i]; gu.log_consts[i] = ubm.log_consts[i]; }
    __syncthreads();
    constexpr int kPer = kLlrScanChunk / 256;
    const int d_n = target.d, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = (long)blockIdx.x * kLlrScanChunk + (long)threadIdx.x * kPer;
    unsigned long long v[kPer], run = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        v[q] = 0;
        if (row0 + q < n_rows) {
            const float *f = mfcc + (row0 + q) * d_n;
            int x[kGmmMaxD];
#pragma unroll
            for (int d = 0; d < kGmmMaxD; ++d) x[d] = d < d_n ? (int)(short)(int)(f[d] * 64.0f) : 0;   // low 16 bits of the int32 truncation
            v[q] = (unsigned long long)gmm_ll(gt, target.k, d_n, x) - (unsigned long long)gmm_ll(gu, ubm.k, d_n, x);   // :104-108, wrapping
        }
        run += v[q];
        v[q] = run;
    }
    unsigned long long incl = run;                                       // inclusive scan of the threads' totals in the wave
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned long long base = incl - run;
    for (int k = 0; k < wave; ++k) base += wave_sum[k];
#pragma unroll
    for (int q = 0; q < kPer; ++q)
        if (row0 + q < n_rows) loc[row0 + q] = base + v[q];
    if (threadIdx.x == 255) chunk_sum[blockIdx.x] = base + run;
}

// Pass 2: one block turns chunk_sum[n_chunks] into its exclusive prefix sums
__global__ __launch_bounds__(256) void scan_chunk_sums_kernel(unsigned long long *__restrict__ chunk_sum, long n_chunks)
{
    __shared__ unsigned long long wave_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (long c0 = 0; c0 < n_chunks; c0 += 256) {
        const long c = c0 + threadIdx.x;
        const unsigned long long x = c < n_chunks ? chunk_sum[c] : 0;
        unsigned long long incl = x;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned long long base = carry + incl - x;
        for (int k = 0; k < wave; ++k) base += wave_sum[k];
        const unsigned long long total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        __syncthreads();
        if (c < n_chunks) chunk_sum[c] = base;
        carry += total;
    }
}

// Pass 3: thread per window.  Q(k) = sum of the first k rows = loc[k - 1] + chunk_sum[(k - 1) / kLlrScanChunk]; window sum = Q(e) - Q(s).
// The wave finds its first window's recording by binary search; a lane walks on from there (a wave spans at most 64 recordings).
__global__ __launch_bounds__(256) void speaker_window_kernel(long n_rec, const long *__restrict__ fo, const long *__restrict__ wo, long n_windows,
                                                             int window_frames, int hop, const unsigned long long *__restrict__ loc,
                                                             const unsigned long long *__restrict__ chunk_sum, long long threshold,
                                                             long long *__restrict__ llr_mean, int *__restrict__ labels)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long g0 = (long)blockIdx.x * 256 + (threadIdx.x & ~63);
    if (g0 >= n_windows) return;
    long r = scan_find(wo, n_rec, g0);
    if (g >= n_windows) return;
    while (wo[r + 1] <= g) ++r;
    const long n_rows = fo[r + 1] - fo[r];
    const long n = n_rows < window_frames ? n_rows : window_frames;       // >= 1: the host refused recordings without rows
    const long s = fo[r] + (g - wo[r]) * hop, e = s + n;
    const unsigned long long qs = s == 0 ? 0ull : loc[s - 1] + chunk_sum[(s - 1) / kLlrScanChunk];
    const unsigned long long qe = loc[e - 1] + chunk_sum[(e - 1) / kLlrScanChunk];
    const long long mean = (long long)(qe - qs) / (long long)n;          // :135
    llr_mean[g] = mean;
    if (labels) labels[g] = mean > threshold ? 1 : 0;                     // :138-141
}

hipError_t launch_speaker_scan(const GmmDev &target, const GmmDev &ubm, const float *mfcc, long n_rows, long n_rec, const long *fo, const long *wo,
                               long n_windows, int window_frames, int hop, long long threshold, unsigned long long *work, long long *llr_mean,
                               int *labels, hipStream_t stream)
{
    if (n_windows <= 0 || n_rows <= 0) return hipSuccess;
    if (target.d != ubm.d || target.k != ubm.k || target.d > kGmmMaxD || target.k > kGmmMaxK || window_frames < 1 || hop < 1) return hipErrorInvalidValue;
    const long n_chunks = (n_rows + kLlrScanChunk - 1) / kLlrScanChunk;
    if (n_chunks >= (1L << 31) || (n_windows + 255) / 256 >= (1L << 31)) return hipErrorInvalidValue;
    unsigned long long *loc = work, *chunk_sum = work + n_rows;
    hipLaunchKernelGGL(speaker_rows_scan_kernel, dim3((unsigned)n_chunks), dim3(256), 0, stream, target, ubm, mfcc, n_rows, loc, chunk_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3(1), dim3(256), 0, stream, chunk_sum, n_chunks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(speaker_window_kernel, dim3((unsigned)((n_windows + 255) / 256)), dim3(256), 0, stream, n_rec, fo, wo, n_windows, window_frames,
                       hop, loc, chunk_sum, threshold, llr_mean, labels);
    return hipGetLastError();
}

}  // namespace dsp
