// gmm_estep.hpp -- the float32 E-step of a diagonal GMM for the statistics kernels of enroll_kernels.hip and ubm_kernels.hip (DESIGN.md
// 3.11): a chunk of rows staged in LDS, lane k of a wave owning component k of a GmmModel, per row the lane's posterior and the row's
// log-likelihood.  What is accumulated from them is each kernel's own.  Also the D dispatch, the owner of a ragged launch's unit, the
// wave-order and the ascending float64 sums (verify_kernels.hip, a row per lane, takes those and restates l_k).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "gmm_model.hpp"
#include "mfcc_device.hpp"
#include "span_find.hpp"

namespace dsp {
namespace {

constexpr int kThreads = 256;    // every kernel of the two files: four wavefronts
constexpr int kRowLd = 16;       // floats per staged row: 16-byte reads of a row, whatever d
static_assert(kRowLd >= kGmmMaxD && kRowLd % 4 == 0, "a staged row holds every d and is read in float4");

// the wave's max / sum in every lane: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror (after each step the lanes of a group
// hold the group's value, so the mirrored lane's is the other group's), then the neighbouring 16-lane row (even, odd) and the other
// half-wave (lower, upper) by permlane swaps.  Both operands of every step are the same pair in both lanes: the same bits in every lane.
template <class Op>
__device__ __forceinline__ float wave_all(float v, Op op)
{
    v = op(v, dpp<DPP_QUAD_1032>(v));
    v = op(v, dpp<DPP_QUAD_2301>(v));
    v = op(v, dpp<DPP_ROW_HALF_MIRROR>(v));
    v = op(v, dpp<DPP_ROW_MIRROR>(v));
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return op(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float wave_max(float v) { return wave_all(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ float wave_sum(float v) { return wave_all(v, [](float a, float b) { return a + b; }); }

// the recording / speaker / clip that owns unit u of a ragged launch (spans[n] with a first unit `unit0` each, enroll_kernels.hpp RowSpan):
// the last one whose first unit is <= u (those without rows own no unit): span_find.hpp's owner_of
template <class Span>
__device__ inline long owner_of_unit(const Span *spans, long n, long u)
{
    return owner_of(n, u, [spans](long i) { return spans[i].unit0; });
}

// rows [0, cnt) of src[cnt][D] into the block's LDS image xs[rows of the chunk][Ld]; a barrier follows before any row is read
template <int D, int Ld = kRowLd>
__device__ __forceinline__ void stage_rows(float *xs, const float *__restrict__ src, int cnt)
{
    for (int i = threadIdx.x; i < cnt * D; i += kThreads) {
        const int r = i / D;
        xs[r * Ld + (i - r * D)] = src[i];
    }
}

// component `lane` of the model in this lane's registers; lanes at or above k: l = -inf, e = 0
template <int D>
struct LaneGmm {
    float lc, c[D], ic[D];
    __device__ __forceinline__ LaneGmm(const GmmModel &m, int lane)
    {
        const bool live = lane < m.k;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            c[j] = live ? m.means()[lane * D + j] : 0.0f;
            ic[j] = live ? m.inv_covs()[lane * D + j] : 0.0f;
        }
        lc = live ? m.log_consts()[lane] : -INFINITY;
    }
};

// row r of the staged chunk into x[] (every lane reads the same address: a broadcast) -> this lane's posterior of the row; ll, the same
// in every lane, is the row's log-likelihood under the model
template <int D>
__device__ __forceinline__ float row_posterior(const float *xs, int r, const LaneGmm<D> &g, float (&x)[4 * ((D + 3) / 4)], float &ll)
{
#pragma unroll
    for (int q = 0; q < (D + 3) / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(xs + r * kRowLd + 4 * q);
        x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {                                    // ascending d
        const float dv = x[j] - g.c[j];
        s = __builtin_fmaf(dv * dv, g.ic[j], s);
    }
    const float l = __builtin_fmaf(-0.5f, s, g.lc);
    const float m = wave_max(l);
    const float e = expf(l - m);
    const float S = wave_sum(e);
    const float p = e / S;
    ll = m + logf(S);
    return p;
}

// entry i of what each of the block's waves left in LDS, `pitch` apart, added in wave order 0, 1, 2, 3
template <class T>
__device__ __forceinline__ T sum_waves(const T *part, int pitch, int i)
{
    T v = part[i];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) v += part[w * pitch + i];
    return v;
}

// sums[i] = partials[0][i] + partials[1][i] + ... (`count` partials, `stride` apart, ascending, float64), i in [0, len) over the block
template <class T>
__device__ __forceinline__ void sum_partials(const T *__restrict__ partials, long count, size_t stride, int len, double *sums)
{
    for (int i = threadIdx.x; i < len; i += kThreads) {
        double acc = 0.0;
        for (long c = 0; c < count; ++c) acc += (double)partials[(size_t)c * stride + i];
        sums[i] = acc;
    }
}

// what f(std::integral_constant<int, D>) returns for the D in 1 .. kGmmMaxD that equals d; any other d: hipErrorInvalidValue and no call
template <int D = 1, class F>
hipError_t dispatch_d(int d, F &&f)
{
    if constexpr (D <= kGmmMaxD) return d == D ? f(std::integral_constant<int, D>{}) : dispatch_d<D + 1>(d, f);
    return hipErrorInvalidValue;
}

}  // namespace
}  // namespace dsp
