// svm_kernels.hip -- a12 pooling + a13 RBF-SVM, one wave per clip.
#include <hip/hip_runtime.h>

#include "scan_device.hpp"
#include "svm_kernels.hpp"

#pragma clang fp contract(off)

namespace dsp {

// Most blocks of 64 lanes the per-clip kernels are launched with; each block walks clips blockIdx.x, blockIdx.x + gridDim.x, ...  The
// runtime counts a launch's work-items (grid x block) in 32 bits and silently runs the remainder modulo 2^32: one block per clip
// computed only the first 40 M of 107 M feature rows, the rest of the outputs left as they were.
constexpr long kMaxClipBlocks = 1L << 24;

// cepstrum/scrubjay_infer.c:36-66: per coefficient sum and sum of squares in double over the
// frames in order, mean = s/T, var = q/T - mean^2, std = sqrtf(max(var, 0)).
__global__ __launch_bounds__(64) void mfcc_stats_kernel(const float *__restrict__ mfcc, long n_clips, int T, int n_coef,
                                                        float *__restrict__ feat)
{
    const int c = threadIdx.x;
    if (c >= n_coef) return;
    for (long clip = blockIdx.x; clip < n_clips; clip += gridDim.x) {
        const float *p = mfcc + clip * (long)T * n_coef + c;
        double s = 0.0, q = 0.0;
        for (int t = 0; t < T; ++t) {
            const double v = (double)p[(long)t * n_coef];
            s = s + v;
            q = q + v * v;
        }
        const double mean = s / (double)T;
        const double var = q / (double)T - mean * mean;
        feat[clip * 2L * n_coef + c] = (float)mean;
        feat[clip * 2L * n_coef + n_coef + c] = sqrtf((float)(var > 0 ? var : 0));
    }
}

hipError_t launch_mfcc_stats(const float *mfcc, long n_clips, int T, int n_coef, float *feat, hipStream_t stream)
{
    if (n_clips <= 0) return hipSuccess;
    if (n_coef > 64 || T <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mfcc_stats_kernel, dim3((unsigned)(n_clips < kMaxClipBlocks ? n_clips : kMaxClipBlocks)), dim3(64), 0, stream, mfcc, n_clips, T, n_coef, feat);
    return hipGetLastError();
}

// ONNX Scaler + SVMClassifier (two classes, RBF, Platt): lane s owns support vector s.
__global__ __launch_bounds__(64) void svm_kernel(const SvmModelDev m, const float *__restrict__ feat, long n_clips,
                                                 int *__restrict__ labels, float *__restrict__ decision, float *__restrict__ prob1)
{
    __shared__ float z[256];
    const int lane = threadIdx.x;
    for (long clip = blockIdx.x; clip < n_clips; clip += gridDim.x) {      // (clip is the same for the whole block: the barriers are uniform)
        for (int j = lane; j < m.n_features; j += 64) z[j] = (feat[clip * (long)m.n_features + j] - m.offset[j]) * m.scale[j];
        __syncthreads();
        float term = 0.0f;
        for (int s = lane; s < m.n_sv; s += 64) {
            const float *sv = m.sv + (long)s * m.n_features;
            float d2 = 0.0f;
            for (int j = 0; j < m.n_features; ++j) {
                const float d = z[j] - sv[j];
                d2 = d2 + d * d;
            }
            term = term + m.coef[s] * expf(-m.gamma * d2);
        }
        for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
        if (lane == 0) {
            const float score = term + m.rho;                    // ONNX "sum + rho" = libsvm's sum - model.rho (rho = intercept)
            int label;
            float p1;
            svm_binary_tail(score, m.prob_a, m.prob_b, label, p1);
            labels[clip] = label;
            if (decision) decision[clip] = score;
            if (prob1) prob1[clip] = p1;
        }
        __syncthreads();                                         // z is read until here
    }
}

hipError_t launch_svm_predict(const SvmModelDev &m, const float *feat, long n_clips, int *labels, float *decision,
                              float *prob1, hipStream_t stream)
{
    if (n_clips <= 0) return hipSuccess;
    if (m.n_features > 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(svm_kernel, dim3((unsigned)(n_clips < kMaxClipBlocks ? n_clips : kMaxClipBlocks)), dim3(64), 0, stream, m, feat, n_clips, labels, decision, prob1);
    return hipGetLastError();
}

// ---- window scans of long recordings: mean | std and the SVM per sliding window of MFCC rows (dsp_svm_scan_device, dsp_scrubjay_scanner_*) ----
// Recording r is rows [fo[r], fo[r + 1]) of a ragged matrix, its windows wo[r] .. wo[r + 1) of the scan, its tiles of TW windows
// to[r] .. to[r + 1) (host planner, capi_util.hpp).  Window w of a recording of R rows holds len = min(R, window_frames) rows: first its
// hc = min(head_rows, len) head rows, rows [ho[r] + w hc, + hc) of `head` (stream framing: the window's own first rows, which see zeros
// before the window where the recording's rows see samples), then rows [w hop + hc, w hop + len) of the recording.
// One block of 256 threads per tile.  TW = 64 / 16 / 4 / 1: the tile's rows are staged in LDS once; TW = 0: one window, rows read from
// memory (windows too long for LDS).  Thread per (window, coefficient): mfcc_stats_kernel's float64 sums in row order, head rows first
// (sliding sums would not be bit-exact).  Then wave v takes windows v, v + 4, ... with svm_kernel's lane order (lane s: support vectors
// s, s + 64, ..., the xor butterfly, + rho); lane k of the wave keeps the score of its k-th window, and libsvm's tail runs once per wave,
// lane-parallel.
template <int TW>
__global__ __launch_bounds__(256) void svm_scan_kernel(const SvmModelDev m, const float *__restrict__ mfcc, const float *__restrict__ head, long n_rec,
                                                       const long *__restrict__ fo, const long *__restrict__ wo, const long *__restrict__ to,
                                                       const long *__restrict__ ho, int window_frames, int hop, int head_rows, int *__restrict__ labels,
                                                       float *__restrict__ decision, float *__restrict__ prob1, float *__restrict__ feat)
{
    extern __shared__ float svm_scan_smem[];
    constexpr int NT = TW > 0 ? TW : 1;
    const long r = scan_find(to, n_rec, (long)blockIdx.x);
    const long w0 = ((long)blockIdx.x - to[r]) * NT;
    const long g0 = wo[r] + w0;                                          // the tile's first window in the scan
    const long n_win = wo[r + 1] - wo[r];
    const int nw = (int)(n_win - w0 < NT ? n_win - w0 : NT);
    const long n_rows = fo[r + 1] - fo[r];
    const int len = n_rows < window_frames ? (int)n_rows : window_frames;   // >= 1: the host refuses recordings without rows
    const int hc = head ? (head_rows < len ? head_rows : len) : 0;
    const int nf = m.n_features, nc = nf / 2;
    float *z = svm_scan_smem;                                           // [nw][nf] standardised features
    // the tile's recording rows from its first window's first non-head row: inside the recording (the planner's window count)
    const float *rows = mfcc + (fo[r] + w0 * hop + hc) * nc;
    const float *hrows = hc > 0 ? head + (ho[r] + w0 * hc) * nc : nullptr;
    if constexpr (TW > 0) {
        float *lh = z + (long)NT * nf;
        const long n_head = (long)nw * hc * nc;
        float *lr = lh + n_head;
        const long n_stage = ((long)(nw - 1) * hop + len - hc) * nc;
        for (long i = threadIdx.x; i < n_head; i += 256) lh[i] = hrows[i];
        for (long i = threadIdx.x; i < n_stage; i += 256) lr[i] = rows[i];
        hrows = lh;
        rows = lr;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < nw * nc; i += 256) {
        const int s = i / nc, c = i - s * nc;
        double sum = 0.0, sq = 0.0;
        if (hc > 0) {
            const float *p = hrows + (long)s * hc * nc + c;
            for (int t = 0; t < hc; ++t) {
                const double v = (double)p[(long)t * nc];
                sum = sum + v;
                sq = sq + v * v;
            }
        }
        const float *p = rows + (long)s * hop * nc + c;
        for (int t = 0; t < len - hc; ++t) {
            const double v = (double)p[(long)t * nc];
            sum = sum + v;
            sq = sq + v * v;
        }
        const double mean = sum / (double)len;
        const double var = sq / (double)len - mean * mean;
        const float f_mean = (float)mean, f_std = sqrtf((float)(var > 0 ? var : 0));
        if (feat) {
            feat[(g0 + s) * nf + c] = f_mean;
            feat[(g0 + s) * nf + nc + c] = f_std;
        }
        z[s * nf + c] = (f_mean - m.offset[c]) * m.scale[c];
        z[s * nf + nc + c] = (f_std - m.offset[nc + c]) * m.scale[nc + c];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float score = 0.0f;
    int k = 0;
    for (int s = wave; s < nw; s += 4, ++k) {
        const float *zs = z + s * nf;
        float term = 0.0f;
        for (int sidx = lane; sidx < m.n_sv; sidx += 64) {
            const float *sv = m.sv + (long)sidx * nf;
            float d2 = 0.0f;
            for (int j = 0; j < nf; ++j) {
                const float d = zs[j] - sv[j];
                d2 = d2 + d * d;
            }
            term = term + m.coef[sidx] * expf(-m.gamma * d2);
        }
        for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
        if (lane == k) score = term + m.rho;
    }
    if (lane < k) {
        const long g = g0 + wave + 4 * lane;
        int label;
        float p1;
        svm_binary_tail(score, m.prob_a, m.prob_b, label, p1);
        labels[g] = label;
        if (decision) decision[g] = score;
        if (prob1) prob1[g] = p1;
    }
}

// LDS bytes of a tile of tw windows (tw = 0: one window, rows not staged)
static long svm_scan_lds(int n_features, int window_frames, int hop, int head_rows, int tw)
{
    const long nc = n_features / 2, hc = head_rows < window_frames ? head_rows : window_frames;
    if (tw == 0) return (long)n_features * (long)sizeof(float);
    return ((long)tw * n_features + (long)tw * hc * nc + ((long)(tw - 1) * hop + window_frames) * nc) * (long)sizeof(float);
}

int svm_scan_tile(int n_features, int window_frames, int hop, int head_rows)
{
    for (int tw : {64, 16, 4, 1})
        if (svm_scan_lds(n_features, window_frames, hop, head_rows, tw) <= kSvmScanLdsBytes) return tw;
    return 0;
}

hipError_t launch_svm_scan(const SvmModelDev &m, const float *mfcc, const float *head, long n_rec, const long *fo, const long *wo, const long *to,
                           const long *ho, long n_tiles, int window_frames, int hop, int head_rows, int tw, int *labels, float *decision,
                           float *prob1, float *feat, hipStream_t stream)
{
    if (n_tiles <= 0) return hipSuccess;
    if (m.n_features <= 0 || (m.n_features & 1) || m.n_features > 128 || window_frames < 1 || hop < 1 || head_rows < 0 || (head_rows > 0 && (!head || !ho)) ||
        n_tiles >= (1L << 31) || tw != svm_scan_tile(m.n_features, window_frames, hop, head_rows))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)svm_scan_lds(m.n_features, window_frames, hop, head_rows, tw);
    const dim3 grid((unsigned)n_tiles), block(256);
    if (head_rows == 0) head = nullptr;
    switch (tw) {
    case 64: hipLaunchKernelGGL(svm_scan_kernel<64>, grid, block, lds, stream, m, mfcc, head, n_rec, fo, wo, to, ho, window_frames, hop, head_rows, labels, decision, prob1, feat); break;
    case 16: hipLaunchKernelGGL(svm_scan_kernel<16>, grid, block, lds, stream, m, mfcc, head, n_rec, fo, wo, to, ho, window_frames, hop, head_rows, labels, decision, prob1, feat); break;
    case 4: hipLaunchKernelGGL(svm_scan_kernel<4>, grid, block, lds, stream, m, mfcc, head, n_rec, fo, wo, to, ho, window_frames, hop, head_rows, labels, decision, prob1, feat); break;
    case 1: hipLaunchKernelGGL(svm_scan_kernel<1>, grid, block, lds, stream, m, mfcc, head, n_rec, fo, wo, to, ho, window_frames, hop, head_rows, labels, decision, prob1, feat); break;
    default: hipLaunchKernelGGL(svm_scan_kernel<0>, grid, block, lds, stream, m, mfcc, head, n_rec, fo, wo, to, ho, window_frames, hop, head_rows, labels, decision, prob1, feat); break;
    }
    return hipGetLastError();
}

}  // namespace dsp
