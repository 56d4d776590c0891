// score_matrix.hpp -- what the stages on a [rows][columns] float32 score matrix share (segments, 3.18 labelled trials,
// 3.19 calibration, 3.24 cohort normalisation): the C ABI's checks of a matrix of labelled trials, the launchers' grids, the kernels'
// small device helpers, and the carver that lays a workspace out.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <string>

#include "../../include/dsp_amd.h"

namespace dsp {

int capi_fail(int code, const std::string &msg);   // sets dsp_last_error() for this thread, returns code

// ---- host checks: a matrix of labelled trials (truth[r] = the row's true column, or -1) ---------------------------------------------

constexpr long kScoreMaxColumns = 1L << 19;
constexpr long kScoreMaxRows = 1L << 31;                     // exclusive
constexpr double kScoreMaxTrials = 35184372088832.0;         // 2^45, exclusive: the grids (a block takes 1024 rows of 4 columns at least)

inline int check_score_shape(long n_rows, long n_columns)
{
    if (n_columns < 1 || n_columns > kScoreMaxColumns) return capi_fail(DSP_EINVAL, "n_columns must be 1 .. 2^19");
    if (n_rows < 0) return capi_fail(DSP_EINVAL, "n_rows < 0");
    if (n_rows >= kScoreMaxRows) return capi_fail(DSP_EINVAL, "2^31 rows or more");
    return DSP_OK;
}

inline int check_truth(const int *truth, long n_rows, long n_columns)
{
    for (long r = 0; r < n_rows; ++r)
        if (truth[r] < -1 || truth[r] >= n_columns)
            return capi_fail(DSP_EINVAL, "truth[" + std::to_string(r) + "] = " + std::to_string(truth[r]) + " is neither -1 nor a column");
    return DSP_OK;
}

inline int check_trial_count(long n_rows, long n_columns)
{
    return (double)n_rows * (double)n_columns >= kScoreMaxTrials ? capi_fail(DSP_EINVAL, "2^45 trials or more in one call") : DSP_OK;
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// a grid of `blocks` blocks (at most 2^36) as x * y; the kernels count them with block_index() and return past `blocks`
inline dim3 grid_for(long blocks)
{
    const long x = std::min<long>(std::max<long>(blocks, 1), 1L << 20);
    return dim3((unsigned)x, (unsigned)ceil_div(std::max<long>(blocks, 1), x));
}

// ---- device helpers -----------------------------------------------------------------------------------------------------------------

#ifdef __HIP__
__device__ inline long block_index() { return (long)blockIdx.y * gridDim.x + blockIdx.x; }

// a float as an ordered key: an unsigned that grows with the float, -0 before +0 (min / max under integer atomics, radix select)
__device__ inline unsigned key_of(float x)
{
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float float_of(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

__device__ inline bool is_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }
__device__ inline bool is_finite(double x) { return fabs(x) <= DBL_MAX; }
#endif

// ---- the carver -----------------------------------------------------------------------------------------------------------------------

// A workspace's layout is written once, as a function that takes its parts from a Carver in order.  Walked over no buffer it counts
// the bytes (`at` afterwards); walked over the buffer it hands out the parts, every one on a 256-byte boundary.
struct Carver {
    char *base = nullptr;
    size_t at = 0;
    template <class T> T *take(size_t count)
    {
        T *part = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += (count * sizeof(T) + 255) & ~(size_t)255;
        return part;
    }
};

}  // namespace dsp
