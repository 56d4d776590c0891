// gmm_stats.hpp -- what the trainers of ubm_kernels.hip (EM) and kmeans_kernels.hip (Lloyd) share behind their statistics kernels, each
// once: the supers' sum over the reduction tree of ubm_kernels.hpp, the launch of a statistics pass with it, and the M-step (DESIGN.md
// 3.12, 3.15).  The two statistics kernels themselves stay apart, each in its trainer's file.
#pragma once

#include <cfloat>

#include "gmm_estep.hpp"
#include "ubm_kernels.hpp"

namespace dsp {
namespace {

// block s adds the partials of groups [s S, (s + 1) S), S = kUbmSuperGroups, `len` doubles each, in ascending order; nothing once *done
// (the first int of the trainer's control word; null: always)
__global__ __launch_bounds__(kThreads) void gmm_supers_kernel(const double *__restrict__ groups, long n_groups, int len, const int *__restrict__ done,
                                                              double *__restrict__ supers)
{
    if (done && *done) return;
    const long g0 = (long)blockIdx.x * kUbmSuperGroups;
    const long g1 = g0 + kUbmSuperGroups < n_groups ? g0 + kUbmSuperGroups : n_groups;
    sum_partials(groups + (size_t)g0 * len, g1 - g0, (size_t)len, len, supers + (size_t)blockIdx.x * len);      // ascending group
}

// the statistics of n rows into `groups`, then `supers`: stats(D as an integral_constant, grid, block, LDS bytes) launches the trainer's
// statistics kernel; `len` is the doubles of one partial.  The trainer's single-block kernel, which adds the supers, follows.
template <class Stats>
hipError_t launch_group_stats(int k, int d, long n, size_t len, const int *done, double *groups, double *supers, hipStream_t stream, Stats &&stats)
{
    const long n_groups = ubm_groups(n), n_supers = ubm_supers(n);
    if (k < 1 || k > kGmmMaxK || n < 1 || n_groups > (1L << 30)) return hipErrorInvalidValue;
    const hipError_t e = dispatch_d(d, [&](auto dc) {
        stats(dc, dim3((unsigned)n_groups), dim3(kThreads), (size_t)(kThreads / 64) * k * (2 * d + 1) * sizeof(float));
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gmm_supers_kernel, dim3((unsigned)n_supers), dim3(kThreads), 0, stream, groups, n_groups, (int)len, done, supers);
    return hipGetLastError();
}

// The M-step of a single block, every thread of it: sums[k][2 d + 1] (N_k, F_k, G_k centred on the float32 means c that the model
// holds) -> sklearn's _estimate_gaussian_parameters (diag) in float64: w, mu, var, log_const into `params`, and the next float32 E-step
// model lc, c = float32(mu), ic = float32(1 / var).  The caller's barrier stands between the writes of `sums` and this.
__device__ __forceinline__ void gmm_mstep(const double *sums, double reg_covar, const UbmParams<double> &params, const GmmModelOut &model)
{
    __shared__ double n_total;
    const int k = model.k, d = model.d, T = 2 * d + 1;
    constexpr double kTiny = 10.0 * DBL_EPSILON;                      // sklearn: nk = resp.sum(axis=0) + 10 * np.finfo(resp.dtype).eps
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int kk = 0; kk < k; ++kk) t += sums[kk * T] + kTiny;    // ascending k
        n_total = t;
    }
    __syncthreads();
    double *w = params.w(), *mu = params.mu(), *var = params.var(), *lcd = params.log_const();
    float *lc = model.log_consts(), *c = model.means(), *ic = model.inv_covs();
    if (threadIdx.x < k) {
        const int kk = threadIdx.x;
        const double *st = sums + kk * T;
        const double n1 = st[0] + kTiny, r = st[0] / n1;
        double log_det = 0.0;
        for (int j = 0; j < d; ++j) {                                 // ascending d
            const double cj = (double)c[kk * d + j];                  // what the statistics were centred on
            const double delta = st[1 + j] / n1;
            const double mean = r * cj + delta;
            const double e2 = st[1 + d + j] / n1 + 2.0 * cj * delta + r * cj * cj;
            const double v = e2 - mean * mean + reg_covar;
            mu[kk * d + j] = mean;
            var[kk * d + j] = v;
            c[kk * d + j] = (float)mean;
            ic[kk * d + j] = (float)(1.0 / v);
            log_det += log(2.0 * M_PI * v);
        }
        const double wk = n1 / n_total;
        const double l = log(wk) - 0.5 * log_det;
        w[kk] = wk;
        lcd[kk] = l;
        lc[kk] = (float)l;
    }
}

}  // namespace
}  // namespace dsp
