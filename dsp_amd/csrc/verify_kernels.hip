// verify_kernels.hip -- every clip of a ragged matrix of (CMVN'd) feature rows against a float UBM and S enrolled speakers: the mean
// log-sum-exp log-likelihood of each model and the speakers' log-likelihood ratios (score_models / evaluate_dir of the
// reference's speaker/gmm_utils.py: target.score(feats) - ubm.score(feats)).  A speaker is its float32 means [k][d] as enrolment wrote
// them; its inv_covs and log_consts are the UBM's.
//
//   scores      a row per lane.  A block takes one chunk of 256 rows of one clip and one tile of kVerifySpeakerTile speakers (speaker tile
//               0 also the UBM).  A lane holds its row's x[D] in registers; a model's log_consts, centres and inv_covs are the same for
//               the whole block and are read with uniform addresses -- scalar loads into SGPRs, no LDS and no barrier.  Per model the lane
//               computes l_k for k = 0 .. K - 1 into registers (gmm_estep.hpp's l_k, bit for bit), their maximum, the sum of
//               expf(l_k - m) in ascending k and ll = m + logf(S).  No posterior is needed, so nothing crosses lanes per row: the only
//               cross-lane step is one float64 sum of the wave's 64 ll per model -- the adjacent pairwise tree (a butterfly gives every
//               lane the tree's value, a + b being b + a) -- which leaves with a plain store as the partial of (tile, model).
//   finalise    one block per clip adds the clip's tiles in ascending order in float64 and writes llr, ll_ubm, ll_target, and the
//               smallest speaker with the largest llr.
// A clip's tiles are cut from its own first row and every sum has a fixed order, so every output of a (clip, speaker) pair is the same
// bits whatever the batch, the other speakers, the speaker's place among them, the grid and what the workspace held.  No atomics.
//
// The window scan of long recordings scores each row once with the same row_ll into a float32 workspace and sums
// each window's rows from it in the clip's order: its two kernels are below the per-clip ones.
//
// Out of scope: per-speaker variances or weights, a trial list instead of the full matrix, CMVN inside the call, multi-GPU.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gmm_estep.hpp"
#include "verify_kernels.hpp"

namespace dsp {
namespace {

static_assert(kThreads == kVerifyChunkRows && kVerifyTileRows == 64, "a row per lane, a tile per wave");

// the sum over the wave's 64 lanes as the adjacent pairwise tree (1, 2, 4, .. 32 apart), in every lane
__device__ __forceinline__ double tile_sum(double v)
{
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) v += __shfl_xor(v, step, 64);
    return v;
}

// ll of this lane's row x under the model (lc, c, ic), every pointer the same in all lanes of the block; k in 1 .. kGmmMaxK
template <int D>
__device__ __forceinline__ float row_ll(const float (&x)[D], const float *__restrict__ lc, const float *__restrict__ c, const float *__restrict__ ic, int k)
{
    float l[kGmmMaxK];
    float m = -INFINITY;
#pragma unroll
    for (int kk = 0; kk < kGmmMaxK; ++kk) {
        if (kk < k) {                                                // (uniform: a scalar branch)
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) {                            // ascending d
                const float dv = x[j] - c[kk * D + j];
                s = __builtin_fmaf(dv * dv, ic[kk * D + j], s);
            }
            l[kk] = __builtin_fmaf(-0.5f, s, lc[kk]);
            m = fmaxf(m, l[kk]);
        }
    }
    float S = 0.0f;
#pragma unroll
    for (int kk = 0; kk < kGmmMaxK; ++kk)                            // ascending k
        if (kk < k) S += expf(l[kk] - m);
    return m + logf(S);
}

template <int D>
__global__ __launch_bounds__(kThreads) void verify_scores_kernel(const float *__restrict__ feats, const RowSpan *__restrict__ spans, long n_clips,
                                                                 const float *__restrict__ ubm, int k, const float *__restrict__ means, long n_speakers,
                                                                 double *__restrict__ partials)
{
    const long c = blockIdx.x;
    const RowSpan sp = spans[owner_of_unit(spans, n_clips, c)];
    const long r0 = (c - sp.unit0) * kVerifyChunkRows;
    const long left = sp.n - r0;
    const int cnt = left < kVerifyChunkRows ? (int)left : kVerifyChunkRows;
    const int tile = threadIdx.x >> 6;
    if (tile * kVerifyTileRows >= cnt) return;                       // a tile without rows has no partial (no barrier follows)
    const bool present = (int)threadIdx.x < cnt;                     // absent rows of the clip's last tile count 0: they read its last row
    const float *row = feats + (sp.row0 + r0 + (present ? (int)threadIdx.x : cnt - 1)) * D;
    float x[D];
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = row[j];
    const size_t kd = (size_t)k * D, n_models = (size_t)n_speakers + 1;
    const float *lc = ubm, *ic = ubm + k + kd;
    double *dst = partials + ((size_t)c * kVerifyTilesPerChunk + tile) * n_models;
    // models of this block: speaker tile 0 starts at the UBM (model 0), the others at their first speaker (model 1 + s)
    const long first = blockIdx.y == 0 ? 0 : 1 + (long)blockIdx.y * kVerifySpeakerTile;
    const long last = 1 + ((long)blockIdx.y + 1) * kVerifySpeakerTile < (long)n_models ? 1 + ((long)blockIdx.y + 1) * kVerifySpeakerTile : (long)n_models;
#pragma unroll 1
    for (long model = first; model < last; ++model) {
        const float *centres = model == 0 ? ubm + k : means + (size_t)(model - 1) * kd;
        const float ll = row_ll<D>(x, lc, centres, ic, k);
        const double sum = tile_sum(present ? (double)ll : 0.0);
        if ((threadIdx.x & 63) == 0) dst[model] = sum;
    }
}

// a candidate beats the best so far with a larger value, or the same value at a smaller index (a NaN loses to every number)
__device__ __forceinline__ bool beats(float v, int i, float best_v, int best_i)
{
    return i >= 0 && (best_i < 0 || v > best_v || (v == best_v && i < best_i) || (best_v != best_v && v == v));
}

__global__ __launch_bounds__(kThreads) void verify_finalize_kernel(const RowSpan *__restrict__ spans, const double *__restrict__ partials, long n_speakers,
                                                                   float *__restrict__ llr, float *__restrict__ ll_ubm, float *__restrict__ ll_target,
                                                                   int *__restrict__ best, float *__restrict__ best_llr)
{
    __shared__ double ubm_sum;
    __shared__ float top_v[kThreads];
    __shared__ int top_i[kThreads];
    const long clip = blockIdx.x;
    const RowSpan sp = spans[clip];
    const size_t n_models = (size_t)n_speakers + 1;
    const long n_tiles = (sp.n + kVerifyTileRows - 1) / kVerifyTileRows;
    const double *src = partials + (size_t)sp.unit0 * kVerifyTilesPerChunk * n_models;
    const double rows = (double)sp.n;
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (long t = 0; t < n_tiles; ++t) acc += src[(size_t)t * n_models];                  // ascending tile
        ubm_sum = acc;
        if (ll_ubm) ll_ubm[clip] = (float)(acc / rows);
    }
    __syncthreads();
    const double L_u = ubm_sum;
    float mine_v = 0.0f;
    int mine_i = -1;
    for (long s = threadIdx.x; s < n_speakers; s += kThreads) {                               // ascending s within a thread
        double acc = 0.0;
        for (long t = 0; t < n_tiles; ++t) acc += src[(size_t)t * n_models + 1 + s];          // ascending tile
        const float ratio = (float)((acc - L_u) / rows);
        const size_t at = (size_t)clip * (size_t)n_speakers + s;
        if (llr) llr[at] = ratio;
        if (ll_target) ll_target[at] = (float)(acc / rows);
        if (beats(ratio, (int)s, mine_v, mine_i)) { mine_v = ratio; mine_i = (int)s; }
    }
    if (!best && !best_llr) return;
    top_v[threadIdx.x] = mine_v;
    top_i[threadIdx.x] = mine_i;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half && beats(top_v[threadIdx.x + half], top_i[threadIdx.x + half], top_v[threadIdx.x], top_i[threadIdx.x])) {
            top_v[threadIdx.x] = top_v[threadIdx.x + half];
            top_i[threadIdx.x] = top_i[threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (best) best[clip] = top_i[0];
        if (best_llr) best_llr[clip] = top_v[0];
    }
}

// ---- the window scan (dsp_speaker_float_scan_device) ----------------------------------------------------------------------
// scores: verify_scores_kernel's block for a chunk of 256 rows of a piece (the rows of one recording that the windows of a run cover)
// and a tile of speakers: a row per lane, the same row_ll -- but every lane stores its row's float32 ll to the workspace
// ws[model][row - base] (64 consecutive floats per wave and model: one 256-byte line) and nothing crosses lanes.  With hop > window the
// rows between two windows are in no window: their lanes store nothing, and a wave of such rows alone returns.
template <int D>
__global__ __launch_bounds__(kThreads) void scan_scores_kernel(const float *__restrict__ feats, const RowSpan *__restrict__ pieces, long n_pieces,
                                                               const float *__restrict__ ubm, int k, const float *__restrict__ means, long n_speakers,
                                                               int window, int hop, long base, long pitch, float *__restrict__ ws)
{
    const long c = blockIdx.x;
    const RowSpan sp = pieces[owner_of_unit(pieces, n_pieces, c)];
    const long r0 = (c - sp.unit0) * kVerifyChunkRows;
    const long left = sp.n - r0;
    const int cnt = left < kVerifyChunkRows ? (int)left : kVerifyChunkRows;
    const long p = r0 + threadIdx.x;                                 // the row within the piece, which starts at a window's first row
    const bool present = (int)threadIdx.x < cnt && (hop <= window || p % hop < window);
    if (__ballot(present) == 0) return;                              // a wave without a row to score (no barrier follows)
    const float *row = feats + (sp.row0 + r0 + ((int)threadIdx.x < cnt ? (int)threadIdx.x : cnt - 1)) * D;      // absent rows read the chunk's last
    float x[D];
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = row[j];
    const size_t kd = (size_t)k * D;
    const long n_models = n_speakers + 1;
    const float *lc = ubm, *ic = ubm + k + kd;
    float *dst = ws + (sp.row0 + p - base);
    const long first = blockIdx.y == 0 ? 0 : 1 + (long)blockIdx.y * kVerifySpeakerTile;
    const long last = 1 + ((long)blockIdx.y + 1) * kVerifySpeakerTile < n_models ? 1 + ((long)blockIdx.y + 1) * kVerifySpeakerTile : n_models;
#pragma unroll 1
    for (long model = first; model < last; ++model) {
        const float *centres = model == 0 ? ubm + k : means + (size_t)(model - 1) * kd;
        const float ll = row_ll<D>(x, lc, centres, ic, k);
        if (present) dst[(size_t)model * (size_t)pitch] = ll;
    }
}

// the float64 sum of one model's ll over the window's n rows from `src`, as a clip's: tiles of 64 from the window's first row, the
// pairwise tree inside a tile (absent rows 0), the tiles in ascending order -- the same value in every lane
__device__ __forceinline__ double window_sum(const float *__restrict__ src, int n, int lane)
{
    double acc = 0.0;
    for (int t = 0; t < n; t += kVerifyTileRows) acc += tile_sum(t + lane < n ? (double)src[t + lane] : 0.0);
    return acc;
}

// windows: one block per window of the run, its four waves striding over the speakers (each wave sums the UBM for itself: no barrier
// in front of the speakers); the outputs and `best` by verify_finalize_kernel's rule.
__global__ __launch_bounds__(kThreads) void scan_windows_kernel(const RowSpan *__restrict__ wins, long n_pieces, int hop, long base, long pitch,
                                                                const float *__restrict__ ws, long n_speakers, float *__restrict__ llr,
                                                                float *__restrict__ ll_ubm, float *__restrict__ ll_target, int *__restrict__ best,
                                                                float *__restrict__ best_llr)
{
    constexpr int kWaves = kThreads / 64;
    __shared__ float top_v[kWaves];
    __shared__ int top_i[kWaves];
    const long w = blockIdx.x;
    const RowSpan sp = wins[owner_of_unit(wins, n_pieces, w)];      // row0: the piece's first window's first row, n: rows per window
    const float *src = ws + (sp.row0 + (w - sp.unit0) * hop - base);
    const int n = (int)sp.n;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double rows = (double)n;
    const double L_u = window_sum(src, n, lane);
    if (threadIdx.x == 0 && ll_ubm) ll_ubm[w] = (float)(L_u / rows);
    float mine_v = 0.0f;
    int mine_i = -1;
    for (long s = wave; s < n_speakers; s += kWaves) {                                         // ascending s within a wave
        const double acc = window_sum(src + (size_t)(1 + s) * (size_t)pitch, n, lane);
        const float ratio = (float)((acc - L_u) / rows);
        if (lane == 0) {
            const size_t at = (size_t)w * (size_t)n_speakers + s;
            if (llr) llr[at] = ratio;
            if (ll_target) ll_target[at] = (float)(acc / rows);
        }
        if (beats(ratio, (int)s, mine_v, mine_i)) { mine_v = ratio; mine_i = (int)s; }
    }
    if (!best && !best_llr) return;
    if (lane == 0) { top_v[wave] = mine_v; top_i[wave] = mine_i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int o = 1; o < kWaves; ++o)
            if (beats(top_v[o], top_i[o], mine_v, mine_i)) { mine_v = top_v[o]; mine_i = top_i[o]; }
        if (best) best[w] = mine_i;
        if (best_llr) best_llr[w] = mine_v;
    }
}

}  // namespace

hipError_t launch_verify_scan(const float *d_feats, const RowSpan *d_pieces, const RowSpan *d_wins, long n_pieces, long chunks, long windows, int window_frames,
                              int hop_frames, long base, long pitch, const GmmModel &ubm, const float *d_means, long n_speakers, float *d_ws, float *d_llr,
                              float *d_ll_ubm, float *d_ll_target, int *d_best, float *d_best_llr, hipStream_t stream)
{
    constexpr long kMaxBlocks = (1L << 31) - 1;
    if (ubm.k < 1 || ubm.k > kGmmMaxK || n_speakers < 1 || n_speakers > kVerifyMaxSpeakers || n_pieces < 1 || chunks < 1 || chunks > kMaxBlocks ||
        windows < 1 || windows > kMaxBlocks || window_frames < 1 || hop_frames < 1 || pitch < 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)chunks, (unsigned)((n_speakers + kVerifySpeakerTile - 1) / kVerifySpeakerTile));
    const hipError_t e = dispatch_d(ubm.d, [&](auto dc) {
        hipLaunchKernelGGL(scan_scores_kernel<decltype(dc)::value>, grid, dim3(kThreads), 0, stream, d_feats, d_pieces, n_pieces, ubm.block, ubm.k, d_means,
                           n_speakers, window_frames, hop_frames, base, pitch, d_ws);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scan_windows_kernel, dim3((unsigned)windows), dim3(kThreads), 0, stream, d_wins, n_pieces, hop_frames, base, pitch, d_ws, n_speakers, d_llr,
                       d_ll_ubm, d_ll_target, d_best, d_best_llr);
    return hipGetLastError();
}

hipError_t launch_verify(const float *d_feats, const RowSpan *d_spans, long n_clips, long total_chunks, const GmmModel &ubm, const float *d_means,
                         long n_speakers, double *d_partials, float *d_llr, float *d_ll_ubm, float *d_ll_target, int *d_best, float *d_best_llr,
                         hipStream_t stream)
{
    constexpr long kMaxBlocks = (1L << 31) - 1;
    if (ubm.k < 1 || ubm.k > kGmmMaxK || n_speakers < 1 || n_speakers > kVerifyMaxSpeakers || n_clips < 1 || n_clips > kMaxBlocks || total_chunks < 1 ||
        total_chunks > kMaxBlocks)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)total_chunks, (unsigned)((n_speakers + kVerifySpeakerTile - 1) / kVerifySpeakerTile));
    const hipError_t e = dispatch_d(ubm.d, [&](auto dc) {
        hipLaunchKernelGGL(verify_scores_kernel<decltype(dc)::value>, grid, dim3(kThreads), 0, stream, d_feats, d_spans, n_clips, ubm.block, ubm.k, d_means,
                           n_speakers, d_partials);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(verify_finalize_kernel, dim3((unsigned)n_clips), dim3(kThreads), 0, stream, d_spans, d_partials, n_speakers, d_llr, d_ll_ubm, d_ll_target,
                       d_best, d_best_llr);
    return hipGetLastError();
}

}  // namespace dsp
