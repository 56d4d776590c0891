// trial_kernels.hpp -- labelled trials on the GPU (include/dsp_amd.h dsp_trials_evaluate_device): the thresholds of the
// sweep and a score's bin among them, which host and device share, the kernels' constants, the layout of the evaluator's workspace and
// what capi_trials.cpp hands the kernels of trial_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_amd.h"
#include "score_matrix.hpp"

namespace dsp {

constexpr long kTrialMaxColumns = kScoreMaxColumns;          // (check_score_shape's)
constexpr long kTrialMaxRows = kScoreMaxRows;                // exclusive
constexpr long kTrialMaxPairs = 1L << 46;
constexpr int kTrialMinThresholds = 2, kTrialMaxThresholds = 1024;
// below this many columns a wavefront's lanes run along the rows of one column (64 consecutive rows per load, S floats apart with S
// small); from it on they run across columns (64 consecutive floats of one row per load) -- the segmenter's switch
constexpr long kTrialLanesAcrossColumns = 32;
// min / max and class counts: rows one wavefront folds before its atomics
constexpr int kTrialStatRowsTime = 4096;                     // lanes along rows: 64 rows per step
constexpr int kTrialStatRowsColumns = 64;                    // lanes across columns: one row per step (a block of 4 waves: 256 rows)
// histogram: a block takes kTrialHistRows rows of a tile of columns; the tile is as wide as the per-block LDS histograms allow
// (trial_hist_columns: every column of the tile, and the pooled row, owns 2 (n + 1) counters and its lo / hi / step / 1 / step)
constexpr int kTrialHistRows = 1024;
constexpr int kTrialHistLds = 64 * 1024;
// pair counting: the rows a wavefront holds in registers (a chunk) and the targets whose scores a block keeps in LDS at a time
constexpr int kTrialPairRegsTime = 16;
constexpr int kTrialPairRowsTime = 64 * kTrialPairRegsTime;  // lanes along rows: 1024 rows of one column per wavefront
constexpr int kTrialPairTileTime = 256;
constexpr int kTrialPairRowsColumns = 32;                    // lanes across columns: 32 rows of 64 columns per wavefront
constexpr int kTrialPairTileColumns = 32;                    // targets per column

// Threshold i of n between lo and hi, as np.linspace(lo, hi, n) computes it: two roundings (never one fused multiply-add), the last
// one hi itself.
__host__ __device__ inline double trial_threshold(double lo, double hi, double step, int n, int i)
{
#pragma clang fp contract(off)
    if (i == n - 1) return hi;
    const double scaled = (double)i * step;
    return scaled + lo;
}
__host__ __device__ inline double trial_step(double lo, double hi, int n) { return (hi - lo) / (double)(n - 1); }

// A score's bin: the number of thresholds below it, 0 .. n (x is not NaN).  The thresholds never decrease, so those below x are
// 0 .. bin - 1, and tp_i = the targets whose bin is above i.  An estimate from (x - lo) * inv_step (inv_step = 1 / step: only the
// estimate depends on it), settled by exact compares against the thresholds themselves.  lo is NaN where no score is finite:
// nothing is above a NaN.
__host__ __device__ inline int trial_bin(float score, double lo, double hi, double step, double inv_step, int n)
{
    const double x = (double)score;
    if (!(lo == lo) || !(x > lo)) return 0;                  // (-inf, and x == lo: not above t_0)
    if (x > hi) return n;                                    // (+inf: hi is the largest finite score)
    const double e = (x - lo) * inv_step;                    // lo < x <= hi: step > 0, 0 < e
    int k = e >= (double)n ? n : (int)e;
    while (k < n && x > trial_threshold(lo, hi, step, n, k)) ++k;
    while (k > 0 && !(x > trial_threshold(lo, hi, step, n, k - 1))) --k;
    return k;
}

// columns per histogram block: all of them when they fit, else the largest power of two that does
inline int trial_hist_columns(long columns, int n)
{
    const long per = 2L * (n + 1) * 4 + 4 * 8;               // counters, and lo / hi / step / 1 / step
    long fit = kTrialHistLds / per - 1;                      // (one more for the pooled row)
    if (fit > 64) fit = 64;
    if (fit >= columns) return (int)columns;
    int p = 1;
    while (2 * p <= fit) p *= 2;
    return p;
}
inline size_t trial_hist_lds_bytes(int tile, int n) { return (size_t)(tile + 1) * (2 * (size_t)(n + 1) * 4 + 4 * 8); }

// min / max as ordered keys (an unsigned that grows with the float, -0 before +0) under integer atomics: max_key = the largest key,
// min_inv = the largest ~key; both 0: no finite score.  Counts of the non-NaN trials per class, and of the NaN ones.
struct TrialStat {
    unsigned max_key, min_inv;
    unsigned long long n_target, n_nontarget, n_nan;
};

// The workspace, laid out by trial_layout over one grow-only buffer (score_matrix.hpp Carver).  `zeroed` bytes from its start are
// cleared by every call that reads them; the rest is written before it is read.
struct TrialWorkspace {
    TrialStat *stat = nullptr;                               // [S + 1], the last one pooled                        (zeroed)
    unsigned *hist = nullptr;                                // [S][2][n + 1]: class 0 = target                      (zeroed)
    unsigned long long *pooled_hist = nullptr;               // [2][n + 1]                                           (zeroed)
    float *target_score = nullptr;                           // [targets]
    unsigned *above = nullptr, *equal = nullptr;             // [targets]
    long *u2 = nullptr, *pn = nullptr;                       // [S]: a column's auc_u2 and P N
    size_t zeroed = 0;
};
inline TrialWorkspace trial_layout(Carver &c, long columns, int n, long targets)
{
    TrialWorkspace w;
    w.stat = c.take<TrialStat>((size_t)columns + 1);
    w.hist = c.take<unsigned>((size_t)columns * 2 * (n + 1));
    w.pooled_hist = c.take<unsigned long long>(2 * (size_t)(n + 1));
    w.zeroed = c.at;
    w.target_score = c.take<float>((size_t)targets);
    w.above = c.take<unsigned>((size_t)targets);
    w.equal = c.take<unsigned>((size_t)targets);
    w.u2 = c.take<long>((size_t)columns);
    w.pn = c.take<long>((size_t)columns);
    return w;
}
inline size_t trial_workspace_bytes(long columns, int n, long targets) { Carver c; trial_layout(c, columns, n, targets); return c.at; }
inline TrialWorkspace trial_carve(char *p, long columns, int n, long targets) { Carver c{p}; return trial_layout(c, columns, n, targets); }

// What one call needs on the device.  truth[T], target_offsets[S + 1] and target_rows[targets] are the device copies of the host's
// arrays.  Everything is enqueued on `stream`; nothing waits for it.
struct TrialCall {
    const float *scores;
    const int *truth;
    const long *target_offsets;
    const int *target_rows;
    long rows, columns, targets;
    int n;                                                   // thresholds
    dsp_trial_column *cols;                                  // [S + 1], may be nullptr
    long *sweep_tp, *sweep_fp;                               // [S + 1][n], may be nullptr
    int *fa_above, *fa_equal;                                // [targets], may be nullptr
};
hipError_t launch_trials(const TrialCall &call, const TrialWorkspace &ws, hipStream_t stream);

}  // namespace dsp
