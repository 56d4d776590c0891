// stoptrain_kernels.hpp -- training the stop-word net on the GPU (include/dsp_amd.h dsp_stop_train_*): the caps, the
// library's random draws (shared by the host helpers of capi_stoptrain.cpp and the kernels of stoptrain_kernels.hip, so that both are
// one definition), what a run looks like on the device and what the host hands the kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dsp_amd.h"

namespace dsp {

constexpr long kStopTrainMaxRows = 65536;
constexpr int kStopTrainMaxUnits = 16;
constexpr int kStopTrainMaxBatch = 256;
constexpr int kStopTrainMaxEpochs = 10000;
constexpr long kStopTrainMaxRuns = 4096;
constexpr int kStopTrainBlock = 256;               // one workgroup per run: one wavefront per SIMD
constexpr int kStopTrainSub = 32;                  // samples whose layers 2-4 are in LDS at a time
constexpr int kStopTrainPoll = 8;                  // the host looks at the stop flags every 8 epochs
constexpr uint64_t kStopTrainGolden = 0x9E3779B97F4A7C15ull;

// ---- random numbers: splitmix64's finaliser, as dsp_kmeans_* and dsp_svm_folds use it ---------------------------------------------------
__host__ __device__ inline uint64_t stop_train_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t stop_train_draw(uint64_t seed, uint64_t stream, uint64_t counter)
{
    return stop_train_mix(stop_train_mix(seed + (stream + 1) * kStopTrainGolden) + (counter + 1) * kStopTrainGolden);
}
__host__ __device__ inline double stop_train_uniform(uint64_t seed, uint64_t stream, uint64_t counter)
{
    return (double)(stop_train_draw(seed, stream, counter) >> 11) * 0x1.0p-53;
}
// element i of the epoch's permutation of 0 .. n - 1: a 4-round Feistel network on the smallest even number of bits (>= 2) covering n,
// cycle-walked until the value is below n
__host__ __device__ inline uint32_t stop_train_order_at(uint32_t n, uint64_t key_epoch, uint32_t i)
{
    int half = 1;
    while (((uint64_t)1 << (2 * half)) < n) ++half;
    const uint32_t mask = ((uint32_t)1 << half) - 1;
    uint32_t x = i;
    do {
        uint32_t l = x >> half, r = x & mask;
        for (int k = 0; k < 4; ++k) {
            const uint32_t f = (uint32_t)(stop_train_mix(key_epoch + (uint64_t)(k + 1) * kStopTrainGolden + r)) & mask;
            const uint32_t t = l ^ f;
            l = r;
            r = t;
        }
        x = (l << half) | r;
    } while (x >= n);
    return x;
}
// the initial value of flat parameter `index`: Glorot-uniform on stream 0 (`limit` = sqrt(6 / (fan_in + fan_out)) of its layer)
__host__ __device__ inline double stop_train_glorot(uint64_t seed, uint64_t index, double limit)
{
    return (2.0 * stop_train_uniform(seed, 0, index) - 1.0) * limit;
}

// The model shape as the kernels read it.  The small parameters -- everything behind kernel1 in the flat order: bias1, kernel2, bias2,
// kernel3, bias3, kernel4, bias4 -- are n_small values; o_* are their offsets among them.
struct StopTrainShape {
    int n_coef, max_frames, t_used, f_used;        // f_used = n_coef * t_used: used feature c * t_used + t is input c * max_frames + t
    int u1, u2, u3, n_small;
    int o_w2, o_b2, o_w3, o_b3, o_w4, o_b4;        // (bias1 is at 0)
    long n_in, n_params;
    double limit[4];                               // Glorot limits of the four kernels
};

inline StopTrainShape stop_train_shape(int n_coef, int max_frames, const int *units, int t_used)
{
    StopTrainShape s{};
    s.n_coef = n_coef; s.max_frames = max_frames; s.t_used = t_used; s.f_used = n_coef * t_used;
    s.u1 = units[0]; s.u2 = units[1]; s.u3 = units[2];
    s.o_w2 = s.u1; s.o_b2 = s.o_w2 + s.u1 * s.u2; s.o_w3 = s.o_b2 + s.u2; s.o_b3 = s.o_w3 + s.u2 * s.u3; s.o_w4 = s.o_b3 + s.u3; s.o_b4 = s.o_w4 + s.u3;
    s.n_small = s.o_b4 + 1;
    s.n_in = (long)n_coef * max_frames;
    s.n_params = s.n_in * s.u1 + s.n_small;
    long fan = s.n_in;
    for (int l = 0; l < 4; ++l) {
        s.limit[l] = sqrt(6.0 / (double)(fan + units[l]));
        fan = units[l];
    }
    return s;
}
// doubles of one run's slab: kernel1 over the used features and the small parameters, each as weights | Adam m | Adam v | best snapshot
inline size_t stop_train_slab(const StopTrainShape &s) { return 4 * ((size_t)s.f_used * s.u1 + s.n_small); }

// One run as the kernels read it.  members[train_first .. + n_train) and members[val_first .. + n_val) are its rows, ascending.
struct StopTrainRun {
    long train_first, val_first;
    int n_train, n_val;
    uint64_t seed;
    double lr;
    double rate[3], keep_scale[3];                 // dropout rate and 1 / (1 - rate) per hidden layer
    int batch, epochs, patience, restore_best;
};

// what a run carries from one epoch's launch to the next
struct StopTrainState {
    double best, last_loss;
    long step;                                     // Adam's t - 1 = optimiser steps taken
    int wait, best_epoch, n_epochs, status;
};

// mean[j], scale[j] of all n_in inputs (float64 sums over rows[0 .. n_rows), nullptr: all rows; inputs past t_used: 0 and 1)
hipError_t launch_stop_train_scaler(const float *mfcc, const long *offsets, const StopTrainShape &s, const int *rows, long n_rows, float *mean,
                                    float *scale, hipStream_t stream);
// z[n][f_used] = (x - mean) / (scale == 0 ? 1 : scale) in float32
hipError_t launch_stop_train_standardise(const float *mfcc, const long *offsets, long n, const StopTrainShape &s, const float *mean,
                                         const float *scale, float *z, hipStream_t stream);
// the initial slab, state and history (NaN) of every run
hipError_t launch_stop_train_init(const StopTrainShape &s, const StopTrainRun *runs, long n_runs, int max_epochs, double *slabs,
                                  StopTrainState *states, int *stop, double *history, hipStream_t stream);
// one epoch of every run that has not stopped: its steps, the validation pass, early stopping and the snapshot
hipError_t launch_stop_train_epoch(const StopTrainShape &s, const float *z, const int *labels, const int *members, const StopTrainRun *runs,
                                   long n_runs, int epoch, int max_epochs, double *slabs, StopTrainState *states, int *stop, double *history,
                                   hipStream_t stream);
// the returned weights of every run as params[P][n_params], prob[P][n] (nullptr: not wanted) and the results
hipError_t launch_stop_train_finish(const StopTrainShape &s, const float *z, long n, const int *labels, const int *members,
                                    const StopTrainRun *runs, long n_runs, const double *slabs, const StopTrainState *states, double *params,
                                    double *prob, dsp_stop_train_result *results, hipStream_t stream);

}  // namespace dsp
