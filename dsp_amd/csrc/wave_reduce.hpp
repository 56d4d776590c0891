// wave_reduce.hpp -- the max and the sum of one float over the 64 lanes of a wavefront, left in every lane with equal bits: what the
// statistics kernels of enroll_kernels.hip and ubm_kernels.hip normalise a row's posteriors with.
#pragma once

#include <hip/hip_runtime.h>

#include "mfcc_device.hpp"

namespace dsp {
namespace {

// the wave's max / sum in every lane: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror (after each step the lanes of a group
// hold the group's value, so the mirrored lane's is the other group's), then the neighbouring 16-lane row and the other half-wave by
// permlane swaps.  Both operands of every step are the same pair in both lanes: every lane ends with the same bits.
__device__ __forceinline__ float wave_max(float v)
{
    v = fmaxf(v, dpp<DPP_QUAD_1032>(v));
    v = fmaxf(v, dpp<DPP_QUAD_2301>(v));
    v = fmaxf(v, dpp<DPP_ROW_HALF_MIRROR>(v));
    v = fmaxf(v, dpp<DPP_ROW_MIRROR>(v));
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp<DPP_QUAD_1032>(v);
    v += dpp<DPP_QUAD_2301>(v);
    v += dpp<DPP_ROW_HALF_MIRROR>(v);
    v += dpp<DPP_ROW_MIRROR>(v);
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);               // (even row) + (odd row) in both
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);            // (lower half) + (upper half) in both
}

}  // namespace
}  // namespace dsp
