// ubm_kernels.hpp -- EM training of a diagonal GMM, the speaker chain's UBM (include/dsp_amd.h dsp_ubm_*): what the host
// code of capi_ubm.cpp hands the kernels of ubm_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "gmm_model.hpp"

namespace dsp {

// The reduction tree of one E-step, a function of the row count n alone:
//   chunk c  = rows [c C, min(n, (c + 1) C)), C = kUbmChunkRows: float32, the four waves' interleaved rows combined in wave order
//   group g  = chunks [g G, (g + 1) G), G = kUbmGroupChunks: one block, the chunks' float32 sums added in ascending order in float64
//   super s  = groups [s S, (s + 1) S), S = kUbmSuperGroups: float64, ascending
//   total    = the supers, ascending, in float64 (the M-step's block)
// Neither the grid, nor the CU count, nor what the workspace held before enters.
constexpr int kUbmChunkRows = 256;
constexpr int kUbmGroupChunks = 16;
constexpr int kUbmSuperGroups = 32;
inline long ubm_groups(long n) { return (n + (long)kUbmChunkRows * kUbmGroupChunks - 1) / ((long)kUbmChunkRows * kUbmGroupChunks); }
inline long ubm_supers(long n) { return (ubm_groups(n) + kUbmSuperGroups - 1) / kUbmSuperGroups; }

// one partial: [k][2 d + 1] doubles (N_k, F_k[0..d), G_k[0..d)) and the sum of the rows' ll behind them
inline size_t ubm_partial_doubles(int k, int d) { return (size_t)k * (2 * d + 1) + 1; }
// the float64 parameters between iterations: w[k], mu[k][d], var[k][d], log_const[k]
inline size_t ubm_param_doubles(int k, int d) { return (size_t)k * (2 * d + 2); }
template <class F> struct UbmParams {
    F *block;                // ubm_param_doubles, on the host or the device
    int k, d;
    __host__ __device__ F *w() const { return block; }
    __host__ __device__ F *mu() const { return block + k; }
    __host__ __device__ F *var() const { return block + k + (size_t)k * d; }
    __host__ __device__ F *log_const() const { return block + k + 2 * (size_t)k * d; }
};

// what the launches of one fit share on the device: `done` is tested first by every kernel of every later iteration
struct UbmCtrl {
    int done, converged, n_iter, pad;
    double prev_lower_bound;
};

struct UbmFit {
    const float *feats;      // [n][d]
    long n;
    double *params;          // ubm_param_doubles
    GmmModelOut model;       // the float32 E-step model of the next iteration: log_const, c = float32(mu), ic = float32(1 / var)
    double *groups;          // [ubm_groups(n)][ubm_partial_doubles]
    double *supers;          // [ubm_supers(n)][ubm_partial_doubles]
    double *lower_bounds;    // [max_iter]
    UbmCtrl *ctrl;
    double tol, reg_covar;
};

// iterations [first, first + count) of EM: per iteration the statistics, the supers and the M-step, all on `stream`, no host round trip
hipError_t launch_ubm_iterations(const UbmFit &fit, int first, int count, hipStream_t stream);

}  // namespace dsp
