// trial_kernels.hip -- labelled trials on the GPU (include/dsp_amd.h dsp_trials_evaluate_device).
//
//   trial_stat_*     pass 1: min / max of the finite scores and the class counts, per column and pooled.  Below
//                    kTrialLanesAcrossColumns columns a wavefront folds 4096 rows of one column, 64 consecutive rows per load; from
//                    there on a lane owns a column and a load is 64 consecutive floats of a row.  min / max travel as ordered
//                    unsigned keys under integer atomics
//   trial_hist       pass 2: a block bins 1024 rows of a tile of columns against the columns' thresholds and against the pooled ones
//                    into LDS histograms per class, then adds what is not zero to the global ones.  The tile is every column where
//                    the histograms fit (the block then reads one contiguous stretch), else a power of two of them
//   trial_sweep      a block per column and one for the pooled row: tp_i / fp_i = suffix sums of the bins, correct_i, the first argmax
//   trial_gather     the targets' scores into the compact (column, row) list; clears their pair counts
//   trial_pairs_*    pass 3: a wavefront holds a chunk of rows in registers, target rows of the column as NaN.  Along rows the block
//                    shares one column and a tile of 256 target scores in LDS, and `above` / `equal` of a target over the chunk are
//                    the population counts of two compare masks per register; across columns a lane owns a column, the tile is 32
//                    targets of each of 64 columns and the counts stay in the lane.  One integer atomic per (target, chunk) and count
//   trial_auc        a wavefront per column: fa_above / fa_equal out (-1 for a NaN target), auc_u2 = sum of 2 wins + ties, auc
//   trial_pooled     one block: the pooled row's auc_u2 and auc from the columns'
// Integer atomics only: every sum is the same whatever the order.  Every row and column index is checked before a load.
#include <climits>
#include <cmath>

#include "trial_kernels.hpp"

namespace dsp {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct Range { double lo, hi, step; };
__device__ inline Range range_of(const TrialStat &s, int n)
{
    Range r;
    if (s.max_key == 0) { r.lo = r.hi = r.step = NAN; return r; }
    r.lo = (double)float_of(~s.min_inv);
    r.hi = (double)float_of(s.max_key);
    r.step = trial_step(r.lo, r.hi, n);
    return r;
}

struct Fold {
    unsigned max_key = 0, min_inv = 0;
    unsigned n_target = 0, n_nontarget = 0, n_nan = 0;       // (a wavefront's share: far below 2^32)
    __device__ void take(float x, bool target)
    {
        if (x != x) { ++n_nan; return; }
        if (target) ++n_target; else ++n_nontarget;
        if (is_finite(x)) {
            const unsigned k = key_of(x);
            max_key = max(max_key, k);
            min_inv = max(min_inv, ~k);
        }
    }
    __device__ void across_wave()
    {
        for (int d = 1; d < 64; d <<= 1) {
            max_key = max(max_key, (unsigned)__shfl_xor((int)max_key, d, 64));
            min_inv = max(min_inv, (unsigned)__shfl_xor((int)min_inv, d, 64));
            n_target += (unsigned)__shfl_xor((int)n_target, d, 64);
            n_nontarget += (unsigned)__shfl_xor((int)n_nontarget, d, 64);
            n_nan += (unsigned)__shfl_xor((int)n_nan, d, 64);
        }
    }
    __device__ void into(TrialStat *s) const
    {
        if (max_key) { atomicMax(&s->max_key, max_key); atomicMax(&s->min_inv, min_inv); }
        if (n_target) atomicAdd(&s->n_target, (unsigned long long)n_target);
        if (n_nontarget) atomicAdd(&s->n_nontarget, (unsigned long long)n_nontarget);
        if (n_nan) atomicAdd(&s->n_nan, (unsigned long long)n_nan);
    }
};

// a wavefront per (chunk of kTrialStatRowsTime rows, column)
__global__ __launch_bounds__(kThreads) void trial_stat_time_kernel(const float *__restrict__ scores, const int *__restrict__ truth, long T, long S, long units,
                                                                   TrialStat *__restrict__ stat)
{
    const long unit = block_index() * kWaves + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (unit >= units) return;
    const long chunk = unit / S, s = unit % S;
    const long r0 = chunk * kTrialStatRowsTime, r1 = min(T, r0 + kTrialStatRowsTime);
    Fold f;
    for (long r = r0 + lane; r < r1; r += 64) f.take(scores[r * S + s], truth[r] == (int)s);
    f.across_wave();
    if (lane == 0) { f.into(stat + s); f.into(stat + S); }
}

// a block per (256 rows, group of 64 columns): a lane per column, a wavefront per 64 rows
__global__ __launch_bounds__(kThreads) void trial_stat_columns_kernel(const float *__restrict__ scores, const int *__restrict__ truth, long T, long S, long groups,
                                                                      long units, TrialStat *__restrict__ stat)
{
    const long unit = block_index();
    if (unit >= units) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const long chunk = unit / groups, s = (unit % groups) * 64 + lane;
    const long r0 = chunk * (kWaves * kTrialStatRowsColumns) + wave * kTrialStatRowsColumns, r1 = min(T, r0 + kTrialStatRowsColumns);
    Fold f;
    if (s < S)
        for (long r = r0; r < r1; ++r) f.take(scores[r * S + s], truth[r] == (int)s);
    if (s < S) f.into(stat + s);
    f.across_wave();
    if (lane == 0) f.into(stat + S);
}

// a block per (kTrialHistRows rows, tile of `tile` columns).  Dynamic LDS: double range[tile + 1][4], then unsigned [tile + 1][2][n + 1].
__global__ __launch_bounds__(kThreads) void trial_hist_kernel(const float *__restrict__ scores, const int *__restrict__ truth, long T, long S, int n, int tile,
                                                              long tiles, long units, const TrialStat *__restrict__ stat, unsigned *__restrict__ hist,
                                                              unsigned long long *__restrict__ pooled_hist)
{
    extern __shared__ double lds_range[];
    const long unit = block_index();
    if (unit >= units) return;
    const long c0 = (unit % tiles) * tile, r0 = (unit / tiles) * kTrialHistRows;
    const int w = (int)min((long)tile, S - c0), rows = (int)min((long)kTrialHistRows, T - r0), bins = n + 1;
    unsigned *counts = reinterpret_cast<unsigned *>(lds_range + 4 * (tile + 1));
    for (int c = threadIdx.x; c <= w; c += kThreads) {                 // c == w: the pooled row
        const Range g = range_of(stat[c < w ? c0 + c : S], n);
        lds_range[4 * c] = g.lo;
        lds_range[4 * c + 1] = g.hi;
        lds_range[4 * c + 2] = g.step;
        lds_range[4 * c + 3] = 1.0 / g.step;
    }
    for (int i = threadIdx.x; i < (w + 1) * 2 * bins; i += kThreads) counts[i] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < rows * w; e += kThreads) {
        const int r = e / w, c = e - r * w;
        const float x = scores[(r0 + r) * S + c0 + c];
        if (x != x) continue;
        const int cls = truth[r0 + r] == (int)(c0 + c) ? 0 : 1;
        atomicAdd(&counts[(c * 2 + cls) * bins + trial_bin(x, lds_range[4 * c], lds_range[4 * c + 1], lds_range[4 * c + 2], lds_range[4 * c + 3], n)], 1u);
        atomicAdd(&counts[(w * 2 + cls) * bins + trial_bin(x, lds_range[4 * w], lds_range[4 * w + 1], lds_range[4 * w + 2], lds_range[4 * w + 3], n)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (w + 1) * 2 * bins; i += kThreads) {
        const unsigned v = counts[i];
        if (!v) continue;
        const int c = i / (2 * bins), rest = i - c * 2 * bins;
        if (c < w) atomicAdd(&hist[(c0 + c) * 2 * bins + rest], v);
        else atomicAdd(&pooled_hist[rest], (unsigned long long)v);
    }
}

// a block per column, block S the pooled row.  sweep_tp / sweep_fp / cols may be nullptr.
__global__ __launch_bounds__(kThreads) void trial_sweep_kernel(const TrialStat *__restrict__ stat, const unsigned *__restrict__ hist,
                                                               const unsigned long long *__restrict__ pooled_hist, long S, int n, long *__restrict__ sweep_tp,
                                                               long *__restrict__ sweep_fp, dsp_trial_column *__restrict__ cols)
{
    __shared__ long sum_t[kThreads], sum_f[kThreads], best_v[kThreads];
    __shared__ int best_i[kThreads];
    const long c = blockIdx.x;
    const int tid = threadIdx.x, bins = n + 1;
    const TrialStat st = stat[c];
    const long N = (long)st.n_nontarget;
    auto bin = [&](int cls, int b) -> long { return c < S ? (long)hist[(c * 2 + cls) * bins + b] : (long)pooled_hist[cls * bins + b]; };
    const int per = (n + kThreads - 1) / kThreads, begin = min(n, tid * per), end = min(n, begin + per);
    long mine_t = 0, mine_f = 0;
    for (int i = begin; i < end; ++i) { mine_t += bin(0, i + 1); mine_f += bin(1, i + 1); }
    sum_t[tid] = mine_t;
    sum_f[tid] = mine_f;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {                 // inclusive suffix sums over the threads
        const long add_t = tid + d < kThreads ? sum_t[tid + d] : 0, add_f = tid + d < kThreads ? sum_f[tid + d] : 0;
        __syncthreads();
        sum_t[tid] += add_t;
        sum_f[tid] += add_f;
        __syncthreads();
    }
    long tp = sum_t[tid] - mine_t, fp = sum_f[tid] - mine_f, best = -1;       // what lies behind this thread's thresholds
    int at = INT_MAX;
    for (int i = end - 1; i >= begin; --i) {
        tp += bin(0, i + 1);
        fp += bin(1, i + 1);
        if (sweep_tp) sweep_tp[c * n + i] = tp;
        if (sweep_fp) sweep_fp[c * n + i] = fp;
        const long correct = tp + (N - fp);
        if (correct >= best) { best = correct; at = i; }
    }
    best_v[tid] = best;
    best_i[tid] = at;
    __syncthreads();
    for (int d = kThreads / 2; d >= 1; d >>= 1) {
        if (tid < d) {
            const long ov = best_v[tid + d];
            const int oi = best_i[tid + d];
            if (ov > best_v[tid] || (ov == best_v[tid] && oi < best_i[tid])) { best_v[tid] = ov; best_i[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0 && cols) {
        const Range g = range_of(st, n);
        dsp_trial_column &out = cols[c];
        out.n_target = (long)st.n_target;
        out.n_nontarget = N;
        out.n_nan = (long)st.n_nan;
        out.lo = g.lo;
        out.hi = g.hi;
        out.best_threshold = trial_threshold(g.lo, g.hi, g.step, n, best_i[0]);
        out.best_correct = best_v[0];
        out.best_index = best_i[0];
        out.reserved = 0;
    }
}

__global__ __launch_bounds__(kThreads) void trial_gather_kernel(const float *__restrict__ scores, const int *__restrict__ truth, const int *__restrict__ target_rows,
                                                                long S, long targets, float *__restrict__ target_score, unsigned *__restrict__ above,
                                                                unsigned *__restrict__ equal)
{
    const long j = block_index() * kThreads + threadIdx.x;
    if (j >= targets) return;
    const long r = target_rows[j];
    target_score[j] = scores[r * S + truth[r]];
    above[j] = 0;
    equal[j] = 0;
}

// a block per (4 chunks of kTrialPairRowsTime rows, column): a wavefront per chunk
__global__ __launch_bounds__(kThreads) void trial_pairs_time_kernel(const float *__restrict__ scores, const int *__restrict__ truth, long T, long S, long units,
                                                                    const long *__restrict__ target_offsets, const float *__restrict__ target_score,
                                                                    unsigned *__restrict__ above, unsigned *__restrict__ equal)
{
    __shared__ float tile[kTrialPairTileTime];
    const long unit = block_index();
    if (unit >= units) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const long s = unit % S, base = ((unit / S) * kWaves + wave) * kTrialPairRowsTime;
    const long j0 = target_offsets[s], count = target_offsets[s + 1] - j0;
    if (count == 0) return;                                  // (the whole block)
    float x[kTrialPairRegsTime];
#pragma unroll
    for (int i = 0; i < kTrialPairRegsTime; ++i) {
        const long r = base + i * 64 + lane;
        x[i] = r < T && truth[r] != (int)s ? scores[r * S + s] : NAN;
    }
    for (long t0 = 0; t0 < count; t0 += kTrialPairTileTime) {
        const int m = (int)min((long)kTrialPairTileTime, count - t0);
        __syncthreads();
        if ((int)threadIdx.x < m) tile[threadIdx.x] = target_score[j0 + t0 + threadIdx.x];
        __syncthreads();
        if (base >= T) continue;                             // (a wavefront without rows still serves the barriers)
        for (int k = 0; k < m; ++k) {
            const float xj = tile[k];
            unsigned a = 0, e = 0;
#pragma unroll
            for (int i = 0; i < kTrialPairRegsTime; ++i) {
                a += (unsigned)__popcll(__ballot(x[i] > xj));
                e += (unsigned)__popcll(__ballot(x[i] == xj));
            }
            if (lane == 0) {
                if (a) atomicAdd(&above[j0 + t0 + k], a);
                if (e) atomicAdd(&equal[j0 + t0 + k], e);
            }
        }
    }
}

// a block per (4 chunks of kTrialPairRowsColumns rows, group of 64 columns): a wavefront per chunk, a lane per column
__global__ __launch_bounds__(kThreads) void trial_pairs_columns_kernel(const float *__restrict__ scores, const int *__restrict__ truth, long T, long S, long groups,
                                                                       long units, const long *__restrict__ target_offsets,
                                                                       const float *__restrict__ target_score, unsigned *__restrict__ above,
                                                                       unsigned *__restrict__ equal)
{
    __shared__ float tile[kTrialPairTileColumns * 64];       // [target][column]: a lane reads its own bank
    __shared__ int most;
    const long unit = block_index();
    if (unit >= units) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const long s0 = (unit % groups) * 64, s = s0 + lane, base = ((unit / groups) * kWaves + wave) * kTrialPairRowsColumns;
    const long j0 = s < S ? target_offsets[s] : 0;
    const int count = s < S ? (int)(target_offsets[s + 1] - j0) : 0;     // (at most T < 2^31)
    if (threadIdx.x == 0) most = 0;
    __syncthreads();
    if (count) atomicMax(&most, count);
    __syncthreads();
    const int longest = most;
    if (longest == 0) return;                                // (the whole block)
    float x[kTrialPairRowsColumns];
#pragma unroll
    for (int i = 0; i < kTrialPairRowsColumns; ++i) {
        const long r = base + i;
        x[i] = s < S && r < T && truth[r] != (int)s ? scores[r * S + s] : NAN;
    }
    for (int t0 = 0; t0 < longest; t0 += kTrialPairTileColumns) {
        __syncthreads();
        for (int i = threadIdx.x; i < kTrialPairTileColumns * 64; i += kThreads) {     // (i & 63 == lane: a thread fills its own column)
            const int k = t0 + (i >> 6);
            tile[i] = k < count ? target_score[j0 + k] : NAN;
        }
        __syncthreads();
        if (base >= T) continue;
        const int m = min(kTrialPairTileColumns, count - t0);
        for (int k = 0; k < m; ++k) {
            const float xj = tile[k * 64 + lane];
            unsigned a = 0, e = 0;
#pragma unroll
            for (int i = 0; i < kTrialPairRowsColumns; ++i) {
                a += x[i] > xj ? 1u : 0u;
                e += x[i] == xj ? 1u : 0u;
            }
            if (a) atomicAdd(&above[j0 + t0 + k], a);
            if (e) atomicAdd(&equal[j0 + t0 + k], e);
        }
    }
}

// a wavefront per column.  stat / cols may be nullptr (only the ROC arrays were asked for), fa_above / fa_equal too.
__global__ __launch_bounds__(kThreads) void trial_auc_kernel(const TrialStat *__restrict__ stat, const long *__restrict__ target_offsets,
                                                             const float *__restrict__ target_score, const unsigned *__restrict__ above,
                                                             const unsigned *__restrict__ equal, long S, int *__restrict__ fa_above, int *__restrict__ fa_equal,
                                                             long *__restrict__ u2, long *__restrict__ pn, dsp_trial_column *__restrict__ cols)
{
    const long s = block_index() * kWaves + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (s >= S) return;
    const long N = stat ? (long)stat[s].n_nontarget : 0, P = stat ? (long)stat[s].n_target : 0;
    long sum = 0;
    for (long j = target_offsets[s] + lane; j < target_offsets[s + 1]; j += 64) {
        const float xj = target_score[j];
        const bool nan = xj != xj;
        const long a = above[j], e = equal[j];
        if (fa_above) fa_above[j] = nan ? -1 : (int)a;
        if (fa_equal) fa_equal[j] = nan ? -1 : (int)e;
        if (!nan) sum += 2 * (N - a - e) + e;
    }
    for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0 && cols) {
        u2[s] = sum;
        pn[s] = P * N;
        cols[s].auc_u2 = sum;
        cols[s].auc = P * N ? (double)sum / (double)(2 * P * N) : NAN;
    }
}

__global__ __launch_bounds__(kThreads) void trial_pooled_kernel(const long *__restrict__ u2, const long *__restrict__ pn, long S, dsp_trial_column *__restrict__ cols)
{
    __shared__ long sum_u[kThreads], sum_p[kThreads];
    const int tid = threadIdx.x;
    long u = 0, p = 0;
    for (long s = tid; s < S; s += kThreads) { u += u2[s]; p += pn[s]; }
    sum_u[tid] = u;
    sum_p[tid] = p;
    __syncthreads();
    for (int d = kThreads / 2; d >= 1; d >>= 1) {
        if (tid < d) { sum_u[tid] += sum_u[tid + d]; sum_p[tid] += sum_p[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) {
        cols[S].auc_u2 = sum_u[0];
        cols[S].auc = sum_p[0] ? (double)sum_u[0] / (double)(2 * sum_p[0]) : NAN;
    }
}

}  // namespace

hipError_t launch_trials(const TrialCall &q, const TrialWorkspace &ws, hipStream_t st)
{
    const long T = q.rows, S = q.columns, groups = ceil_div(S, 64);
    const bool across = S >= kTrialLanesAcrossColumns;
    const bool want_sweep = q.cols || q.sweep_tp || q.sweep_fp, want_pairs = q.cols || q.fa_above || q.fa_equal;
    if (want_sweep) {
        hipError_t e = hipMemsetAsync(ws.stat, 0, ws.zeroed, st);
        if (e != hipSuccess) return e;
        if (across) {
            const long units = ceil_div(T, kWaves * kTrialStatRowsColumns) * groups;
            trial_stat_columns_kernel<<<grid_for(units), kThreads, 0, st>>>(q.scores, q.truth, T, S, groups, units, ws.stat);
        } else {
            const long units = ceil_div(T, kTrialStatRowsTime) * S;
            trial_stat_time_kernel<<<grid_for(ceil_div(units, kWaves)), kThreads, 0, st>>>(q.scores, q.truth, T, S, units, ws.stat);
        }
        const int tile = trial_hist_columns(S, q.n);
        const long tiles = ceil_div(S, tile), units = ceil_div(T, kTrialHistRows) * tiles;
        trial_hist_kernel<<<grid_for(units), kThreads, trial_hist_lds_bytes(tile, q.n), st>>>(q.scores, q.truth, T, S, q.n, tile, tiles, units, ws.stat, ws.hist,
                                                                                             ws.pooled_hist);
        trial_sweep_kernel<<<(unsigned)(S + 1), kThreads, 0, st>>>(ws.stat, ws.hist, ws.pooled_hist, S, q.n, q.sweep_tp, q.sweep_fp, q.cols);
    }
    if (want_pairs) {
        if (q.targets > 0) {
            trial_gather_kernel<<<grid_for(ceil_div(q.targets, kThreads)), kThreads, 0, st>>>(q.scores, q.truth, q.target_rows, S, q.targets, ws.target_score,
                                                                                             ws.above, ws.equal);
            if (across) {
                const long units = ceil_div(T, kWaves * kTrialPairRowsColumns) * groups;
                trial_pairs_columns_kernel<<<grid_for(units), kThreads, 0, st>>>(q.scores, q.truth, T, S, groups, units, q.target_offsets, ws.target_score,
                                                                               ws.above, ws.equal);
            } else {
                const long units = ceil_div(T, kWaves * kTrialPairRowsTime) * S;
                trial_pairs_time_kernel<<<grid_for(units), kThreads, 0, st>>>(q.scores, q.truth, T, S, units, q.target_offsets, ws.target_score, ws.above,
                                                                            ws.equal);
            }
        }
        trial_auc_kernel<<<grid_for(ceil_div(S, kWaves)), kThreads, 0, st>>>(q.cols ? ws.stat : nullptr, q.target_offsets, ws.target_score, ws.above, ws.equal, S,
                                                                            q.fa_above, q.fa_equal, ws.u2, ws.pn, q.cols);
        if (q.cols) trial_pooled_kernel<<<1, kThreads, 0, st>>>(ws.u2, ws.pn, S, q.cols);
    }
    return hipGetLastError();
}

}  // namespace dsp
