// ubm_kernels.hip -- EM for a diagonal GMM on a device matrix of feature rows: the UBM that enrolment and the integer scorer start from
// (GaussianMixture(covariance_type="diag") of the reference's 2fa/audio/speaker/train_ubm.py, its M-step and its stop).
//
// Per iteration, from the float64 parameters w, mu, var the float32 E-step model log_const, c = float32(mu), ic = float32(1 / var); then
//   statistics  one block per group of kUbmGroupChunks chunks of kUbmChunkRows rows.  Lane k of a wave owns component k -- c_k, ic_k and the
//               accumulators N_k, F_k[d], G_k[d] in registers; per row the posterior p of gmm_estep.hpp's E-step, then
//               N += p, F += p (x - c), G += (p (x - c)) (x - c): moments centred on c (E[x^2] - mean^2 in float32 goes negative at the
//               variance floor).  Per chunk the four waves combine through LDS in wave order and every thread adds the chunk's float32
//               sums it owns to float64 accumulators; the group's partial leaves with plain stores.
//   supers      gmm_stats.hpp's: block s adds groups [s S, (s + 1) S) in ascending order, float64
//   M-step      one block adds the supers in ascending order, does gmm_stats.hpp's M-step (sklearn's _estimate_gaussian_parameters, diag,
//               in float64: the next parameters and the next float32 model), and writes lower_bounds[i] and the stop decision
// The tree depends on n alone (ubm_kernels.hpp) and there are no atomics: a fit is the same bits whatever the grid or the workspace.
// Every kernel tests UbmCtrl::done first, so max_iter iterations are enqueued without a host round trip and those after the stop do nothing.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gmm_stats.hpp"

namespace dsp {
namespace {

template <int D>
__global__ __launch_bounds__(kThreads, 4) void ubm_stats_kernel(const float *__restrict__ feats, long n, GmmModel model,
                                                             const UbmCtrl *__restrict__ ctrl, double *__restrict__ groups)
{
    constexpr int W = kThreads / 64, T = 2 * D + 1, S = (kGmmMaxK * T + kThreads - 1) / kThreads;
    __shared__ __attribute__((aligned(16))) float xs[kUbmChunkRows * kRowLd];
    extern __shared__ float part[];                                  // per wave: [k][T] (dynamic: W k T floats, so that k = 32 keeps 4 blocks per CU)
    __shared__ double ll_part[W];                                    // per wave: its rows' sum of ll (wave-uniform)
    if (ctrl->done) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = model.k;
    const bool live = lane < k;
    const LaneGmm<D> g(model, lane);
    const int n_stats = k * T, P = n_stats;
    double acc[S], ll_acc = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = 0.0;
    const long row0 = (long)blockIdx.x * kUbmGroupChunks * kUbmChunkRows;
    for (int cc = 0; cc < kUbmGroupChunks; ++cc) {
        const long r0 = row0 + (long)cc * kUbmChunkRows;
        if (r0 >= n) break;
        const long left = n - r0;
        const int cnt = left < kUbmChunkRows ? (int)left : kUbmChunkRows;
        stage_rows<D>(xs, feats + r0 * D, cnt);
        float N = 0.0f, F[D], G[D];
#pragma unroll
        for (int j = 0; j < D; ++j) F[j] = G[j] = 0.0f;
        double ll_sum = 0.0;
        __syncthreads();
        for (int r = wave; r < cnt; r += W) {
            float x[4 * ((D + 3) / 4)], ll;
            const float p = row_posterior<D>(xs, r, g, x, ll);
            ll_sum += (double)ll;
            N += p;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float dv = x[j] - g.c[j];
                const float pd = p * dv;
                F[j] += pd;
                G[j] = __builtin_fmaf(pd, dv, G[j]);
            }
        }
        float *mine = part + wave * P + lane * T;
        if (live) {
            mine[0] = N;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                mine[1 + j] = F[j];
                mine[1 + D + j] = G[j];
            }
        }
        if (lane == 0) ll_part[wave] = ll_sum;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int i = threadIdx.x + s * kThreads;
            if (i < n_stats) acc[s] += (double)sum_waves(part, P, i);      // ascending chunk
        }
        if (threadIdx.x == 0) ll_acc += sum_waves(ll_part, 1, 0);
        // the next chunk's rows may be staged at once: every wave left xs before the barrier above, and `part` is written again only
        // behind the next one
    }
    double *dst = groups + (size_t)blockIdx.x * ((size_t)n_stats + 1);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int i = threadIdx.x + s * kThreads;
        if (i < n_stats) dst[i] = acc[s];
    }
    if (threadIdx.x == 0) dst[n_stats] = ll_acc;
}

__global__ __launch_bounds__(kThreads) void ubm_mstep_kernel(const double *__restrict__ supers, long n_supers, long n, int iter, double tol,
                                                             double reg_covar, double *__restrict__ params, GmmModelOut model,
                                                             double *__restrict__ lower_bounds, UbmCtrl *__restrict__ ctrl)
{
    __shared__ double sums[kGmmMaxK * (2 * kGmmMaxD + 1) + 1];
    if (ctrl->done) return;
    const int n_stats = model.k * (2 * model.d + 1);
    sum_partials(supers, n_supers, (size_t)n_stats + 1, n_stats + 1, sums);      // ascending super
    __syncthreads();
    gmm_mstep(sums, reg_covar, UbmParams<double>{params, model.k, model.d}, model);
    if (threadIdx.x == 0) {
        const double lb = sums[n_stats] / (double)n;
        lower_bounds[iter] = lb;
        ctrl->n_iter = iter + 1;
        if (fabs(lb - ctrl->prev_lower_bound) < tol) {                // (-inf before the first iteration: never below tol)
            ctrl->converged = 1;
            ctrl->done = 1;
        }
        ctrl->prev_lower_bound = lb;
    }
}

}  // namespace

hipError_t launch_ubm_iterations(const UbmFit &f, int first, int count, hipStream_t stream)
{
    for (int it = first; it < first + count; ++it) {
        hipError_t e = launch_group_stats(f.model.k, f.model.d, f.n, ubm_partial_doubles(f.model.k, f.model.d), &f.ctrl->done, f.groups, f.supers, stream, [&](auto dc, dim3 grid, dim3 block, size_t lds) {
            hipLaunchKernelGGL(ubm_stats_kernel<decltype(dc)::value>, grid, block, lds, stream, f.feats, f.n, GmmModel{f.model.block, f.model.k, f.model.d}, f.ctrl, f.groups);
        });
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ubm_mstep_kernel, dim3(1), dim3(kThreads), 0, stream, f.supers, ubm_supers(f.n), f.n, it, f.tol, f.reg_covar, f.params, f.model, f.lower_bounds, f.ctrl);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dsp
