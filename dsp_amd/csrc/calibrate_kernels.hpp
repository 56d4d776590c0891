// calibrate_kernels.hpp -- score calibration on the GPU (include/dsp_amd.h dsp_calibration_*): the kernels' constants, the
// reduction tree as a function of the shape, the layout of the calibrator's workspace and what capi_calibrate.cpp hands the kernels of
// calibrate_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/dsp_amd.h"
#include "trial_kernels.hpp"

namespace dsp {

constexpr int kCalMaxIter = 10000;
constexpr int kCalMaxHalvings = 30;
// the statistics pass, its two layouts (the switch is the trials': kTrialLanesAcrossColumns).  Lanes along rows: a wavefront folds
// kCalRowsTime rows of one column and writes one partial.  Lanes across columns: a wavefront folds kCalRowsColumns rows of 64 columns,
// a block of four wavefronts writes one partial.
constexpr int kCalRowsTime = 1024;
constexpr int kCalRowsColumns = 64;
constexpr int kCalBlockRowsColumns = 4 * kCalRowsColumns;
// every level of the tree above the statistics adds kCalFanIn consecutive partials in ascending order; the solve kernel adds the last
// kCalFanIn at most
constexpr int kCalFanIn = 16;

// One partial sum: per class (0 = target, 1 = non-target) the objective's sum of softplus, the gradient's sum over phi = (x, 1, l) and
// the upper triangle of the Hessian's sum (xx, x1, xl, 11, 1l, ll) -- unweighted: prior / P and (1 - prior) / N come in the solve
// kernel, from the counts of the same pass.
constexpr int kCalSums = 10;                                 // doubles per class
constexpr int kCalCounts = 3;                                // targets, non-targets, excluded
struct CalPartial {
    double sum[2 * kCalSums];                                // class 0, then class 1
    long n[kCalCounts];
};
constexpr int kCalWords = 2 * kCalSums + kCalCounts;         // 8-byte words of a partial: the doubles, then the counts
static_assert(sizeof(CalPartial) == kCalWords * 8, "a partial is 23 words");

// The fit's state, on the device from the first pass to the last.  `report` is what the host reads back.
struct CalState {
    double theta[3], base[3], step[3];
    double objective_base;
    int halvings, pending, done, reserved;
    dsp_calibration_report report;
};

// partials the statistics pass writes
inline long cal_units(long rows, long columns)
{
    if (columns >= kTrialLanesAcrossColumns) return ceil_div(rows, kCalBlockRowsColumns) * ceil_div(columns, 64);
    return ceil_div(rows, kCalRowsTime) * columns;
}
// partials of every level together: the statistics', then each reduction's, down to kCalFanIn or fewer
inline long cal_partials(long rows, long columns)
{
    long n = cal_units(rows, columns), total = n;
    while (n > kCalFanIn) { n = ceil_div(n, kCalFanIn); total += n; }
    return total;
}
inline size_t cal_workspace_bytes(long rows, long columns) { return 256 + (size_t)cal_partials(rows, columns) * sizeof(CalPartial); }

// What a fit needs on the device.  truth[T] and duration[T] (nullptr: the two-parameter model) are the device copies of the host's
// arrays; state and partials lie in the workspace.  Everything is enqueued on the stream; nothing waits for it.
struct CalFit {
    const float *scores;
    const int *truth;
    const double *duration;
    long rows, columns;
    double prior, tol;
    int max_iter;
    dsp_calibration init;
    CalState *state;
    CalPartial *partials;
};
hipError_t launch_calibration_fit(const CalFit &fit, hipStream_t stream);
hipError_t launch_calibration_apply(const float *scores, const double *duration, long rows, long columns, dsp_calibration params, float *out,
                                    hipStream_t stream);

}  // namespace dsp
