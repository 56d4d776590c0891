// kmeans_kernels.hip -- the k-means start of UBM training on a device matrix of feature rows (what sklearn's
// GaussianMixture(init_params="kmeans", n_init=...) does before EM in the reference's 2fa/audio/speaker/train_ubm.py).
//
// Lloyd: one iteration is the UBM statistics pass of ubm_kernels.hip with a hard posterior.  Lane k of a wave owns centre k; per row
//   s_k = sum_d (x_d - c_kd)^2 in float32 (ascending d, fused multiply-add), the label is the lowest lane that holds the wave's minimum,
//   and that lane alone adds 1, (x - c) and (x - c)^2 to its N, F, G.  The chunk / group / super tree, the float32-in-chunk and
//   float64-above-it rule and the control word are those of the EM kernels, and the supers' kernel and the launch are gmm_stats.hpp's;
//   the inertia (float32 in the chunk) and the number of rows whose label changed (an integer, exact) ride behind the statistics in
//   every partial.
//   update      one block adds the supers and moves the centres in float64: c + F / N, an empty cluster keeps its centre; then the stop
//   final pass  the same statistics against the final centres, then gmm_stats.hpp's M-step on them (dsp_amd.h step 4): the GMM start,
//               written into the float64 parameter block and the float32 E-step model that EM reads
// Seeding (greedy k-means++): a row per thread.  Per step one pass over the rows folds the last winner into m[i], evaluates the step's
//   proposals at once and leaves one set of chunk and group sums per proposal; one block then adds the supers, picks the winner, and
//   walks the winner's sums top down (supers, groups, chunks, rows) to the next step's proposals.
#include <hip/hip_runtime.h>

#include <cmath>

#include "gmm_stats.hpp"
#include "kmeans_kernels.hpp"

namespace dsp {
namespace {

__device__ __forceinline__ float wave_min(float v) { return wave_all(v, [](float a, float b) { return fminf(a, b); }); }

template <int D>
__global__ __launch_bounds__(kThreads, 4) void kmeans_stats_kernel(const float *__restrict__ feats, long n, GmmModel model, const KmeansCtrl *__restrict__ ctrl,
                                                                int final_pass, int *__restrict__ labels, double *__restrict__ groups)
{
    constexpr int W = kThreads / 64, T = 2 * D + 1, S = (kGmmMaxK * T + kThreads - 1) / kThreads;
    __shared__ __attribute__((aligned(16))) float xs[kUbmChunkRows * kRowLd];
    extern __shared__ float part[];                                  // per wave: [k][T]
    __shared__ float inertia_part[W];                                // per wave: its rows' sum of s_label (wave-uniform)
    __shared__ int label_of[kUbmChunkRows];
    __shared__ int changed_part[W];
    if (!final_pass && ctrl->done) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = model.k;
    const bool live = lane < k;
    float c[D];
#pragma unroll
    for (int j = 0; j < D; ++j) c[j] = live ? model.means()[lane * D + j] : 0.0f;
    const int n_stats = k * T, P = n_stats;
    double acc[S], inertia_acc = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = 0.0;
    int changed = 0;                                                 // wave-uniform
    const long row0 = (long)blockIdx.x * kUbmGroupChunks * kUbmChunkRows;
    for (int cc = 0; cc < kUbmGroupChunks; ++cc) {
        const long r0 = row0 + (long)cc * kUbmChunkRows;
        if (r0 >= n) break;
        const long left = n - r0;
        const int cnt = left < kUbmChunkRows ? (int)left : kUbmChunkRows;
        stage_rows<D>(xs, feats + r0 * D, cnt);
        float N = 0.0f, F[D], G[D], inertia = 0.0f;
#pragma unroll
        for (int j = 0; j < D; ++j) F[j] = G[j] = 0.0f;
        __syncthreads();
        for (int r = wave; r < cnt; r += W) {
            float x[4 * ((D + 3) / 4)];
#pragma unroll
            for (int q = 0; q < (D + 3) / 4; ++q) {
                const float4 v = *reinterpret_cast<const float4 *>(xs + r * kRowLd + 4 * q);
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) {                            // ascending d
                const float dv = x[j] - c[j];
                s = __builtin_fmaf(dv, dv, s);
            }
            s = live ? s : INFINITY;
            const float best = wave_min(s);
            const unsigned long long at = __ballot(s == best);
            const int label = at ? __ffsll(at) - 1 : 0;               // ties to the lowest k (no lane at all: a row that is not finite)
            const bool mine = lane == label;
            inertia += best;
            N += mine ? 1.0f : 0.0f;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float dv = mine ? x[j] - c[j] : 0.0f;
                F[j] += dv;
                G[j] = __builtin_fmaf(dv, dv, G[j]);
            }
            if (lane == 0) label_of[r] = label;
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
        if (lane == 0) inertia_part[wave] = inertia;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int i = threadIdx.x + s * kThreads;
            if (i < n_stats) acc[s] += (double)sum_waves(part, P, i);      // ascending chunk
        }
        if (threadIdx.x == 0) inertia_acc += (double)sum_waves(inertia_part, 1, 0);
        bool moved = false;
        if ((int)threadIdx.x < cnt) {                                 // row r0 + thread: one coalesced read and write of the labels
            const int now = label_of[threadIdx.x];
            moved = labels[r0 + threadIdx.x] != now;
            labels[r0 + threadIdx.x] = now;
        }
        changed += __popcll(__ballot(moved));
        // the next chunk's rows may be staged at once: every wave left xs before the barrier above; `part`, inertia_part and label_of
        // are written again only behind the next one
    }
    if (lane == 0) changed_part[wave] = changed;
    __syncthreads();
    double *dst = groups + (size_t)blockIdx.x * ((size_t)n_stats + 2);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int i = threadIdx.x + s * kThreads;
        if (i < n_stats) dst[i] = acc[s];
    }
    if (threadIdx.x == 0) {
        dst[n_stats] = inertia_acc;
        dst[n_stats + 1] = (double)(changed_part[0] + changed_part[1] + changed_part[2] + changed_part[3]);
    }
}
static_assert(kThreads / 64 == 4, "changed_part is added as four waves");

__global__ __launch_bounds__(kThreads) void kmeans_update_kernel(const double *__restrict__ supers, long n_supers, int iter, int max_iter, double shift_limit,
                                                                 double *__restrict__ centres, GmmModelOut model, KmeansCtrl *__restrict__ ctrl)
{
    __shared__ double sums[kGmmMaxK * (2 * kGmmMaxD + 1) + 2];
    __shared__ double shift[kGmmMaxK];
    if (ctrl->done) return;
    const int k = model.k, d = model.d, T = 2 * d + 1, n_stats = k * T;
    sum_partials(supers, n_supers, (size_t)n_stats + 2, n_stats + 2, sums);      // ascending super
    __syncthreads();
    float *c = model.means();
    if (threadIdx.x < k) {
        const int kk = threadIdx.x;
        const double *st = sums + kk * T;
        double moved = 0.0;
        for (int j = 0; j < d; ++j) {                                 // ascending d
            const double old = centres[kk * d + j];
            const double now = st[0] > 0.0 ? (double)c[kk * d + j] + st[1 + j] / st[0] : old;      // an empty cluster keeps its centre
            moved += (now - old) * (now - old);
            centres[kk * d + j] = now;
            c[kk * d + j] = (float)now;
        }
        shift[kk] = moved;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int kk = 0; kk < k; ++kk) total += shift[kk];           // ascending k
        ctrl->n_iter = iter + 1;
        if (sums[n_stats + 1] == 0.0) {                               // no label changed: sklearn's strict convergence, tested first
            ctrl->reason = kKmeansStopStrict;
            ctrl->done = 1;
        } else if (total <= shift_limit) {
            ctrl->reason = kKmeansStopTol;
            ctrl->done = 1;
        } else if (iter + 1 >= max_iter) {
            ctrl->reason = kKmeansStopMaxIter;
            ctrl->done = 1;
        }
    }
}

// the statistics of the final labels -> the GMM start: gmm_stats.hpp's M-step, with p in {0, 1}
__global__ __launch_bounds__(kThreads) void kmeans_gmm_start_kernel(const double *__restrict__ supers, long n_supers, double reg_covar, double *__restrict__ params,
                                                                    GmmModelOut model, double *__restrict__ counts, KmeansCtrl *__restrict__ ctrl)
{
    __shared__ double sums[kGmmMaxK * (2 * kGmmMaxD + 1) + 2];
    const int k = model.k, T = 2 * model.d + 1, n_stats = k * T;
    sum_partials(supers, n_supers, (size_t)n_stats + 2, n_stats + 2, sums);      // ascending super
    __syncthreads();
    if (threadIdx.x == 0) {
        int empty = 0;
        for (int kk = 0; kk < k; ++kk) empty += sums[kk * T] == 0.0;
        ctrl->n_empty = empty;
        ctrl->inertia = sums[n_stats];
    }
    if (threadIdx.x < k) counts[threadIdx.x] = sums[threadIdx.x * T];
    gmm_mstep(sums, reg_covar, UbmParams<double>{params, k, model.d}, model);
}

// --- seeding ---

constexpr int kSeedLd = 17;      // floats per staged row: a row per thread, an odd pitch keeps the lanes on different banks

template <int D>
__device__ __forceinline__ float sq_dist(const float (&x)[D], const float *c)
{
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {                                    // ascending d
        const float dv = x[j] - c[j];
        s = __builtin_fmaf(dv, dv, s);
    }
    return s;
}

// a child of [first, first + count) by the cumulative walk: the first whose sum exceeds what is left of r, children without a sum never;
// past the end (rounding) the last child with a sum, and r = inf so that the levels below do the same.  -1: no child has a sum.
template <class T>
__device__ inline long walk_down(const T *sums, long first, long count, double &r)
{
    long last = -1;
    for (long i = first; i < first + count; ++i) {
        const double v = (double)sums[i];
        if (!(v > 0.0)) continue;
        last = i;
        if (r < v) return i;
        r -= v;
    }
    r = INFINITY;
    return last;
}

template <int D>
__global__ __launch_bounds__(kThreads) void kmeans_seed_pass_kernel(const float *__restrict__ feats, long n, int step, int n_cand, float *__restrict__ m,
                                                                    const KmeansSeedCtrl *__restrict__ ctrl, double *__restrict__ chunks, long n_chunks,
                                                                    double *__restrict__ groups, long n_groups)
{
    constexpr int TR = kKmeansMaxTrials, SEG = kKmeansSegmentRows, NSEG = kUbmChunkRows / SEG;
    __shared__ float xs[kUbmChunkRows * kSeedLd];
    __shared__ float cx[(TR + 1) * kRowLd];                           // the last winner, then the proposals
    __shared__ float v[TR][kUbmChunkRows];
    __shared__ double seg[TR][NSEG];
    __shared__ double chunk_sum[TR][kUbmGroupChunks];
    if (ctrl->failed) return;
    if ((int)threadIdx.x < (n_cand + 1) * D) {
        const int q = threadIdx.x / D, j = threadIdx.x - q * D;
        const long row = q == 0 ? (step > 0 ? ctrl->rows[step - 1] : -1) : ctrl->cand[q - 1];
        cx[q * kRowLd + j] = row >= 0 && row < n ? feats[row * D + j] : 0.0f;
    }
    const long row0 = (long)blockIdx.x * kUbmGroupChunks * kUbmChunkRows;
    int n_here = 0;
    for (int cc = 0; cc < kUbmGroupChunks; ++cc) {
        const long r0 = row0 + (long)cc * kUbmChunkRows;
        if (r0 >= n) break;
        n_here = cc + 1;
        const long left = n - r0;
        const int cnt = left < kUbmChunkRows ? (int)left : kUbmChunkRows;
        stage_rows<D, kSeedLd>(xs, feats + r0 * D, cnt);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            float x[D];
#pragma unroll
            for (int j = 0; j < D; ++j) x[j] = xs[threadIdx.x * kSeedLd + j];
            const float mi = step > 0 ? fminf(m[r0 + threadIdx.x], sq_dist<D>(x, cx)) : INFINITY;
            m[r0 + threadIdx.x] = mi;
            for (int q = 0; q < n_cand; ++q) v[q][threadIdx.x] = fminf(mi, sq_dist<D>(x, cx + (q + 1) * kRowLd));
        } else {
            for (int q = 0; q < n_cand; ++q) v[q][threadIdx.x] = 0.0f;
        }
        __syncthreads();
        if ((int)threadIdx.x < n_cand * NSEG) {                       // float64 from the row up: 16 rows to a segment, ascending
            const int q = threadIdx.x / NSEG, sg = threadIdx.x - q * NSEG;
            double acc = 0.0;
            for (int i = 0; i < SEG; ++i) acc += (double)v[q][sg * SEG + i];
            seg[q][sg] = acc;
        }
        __syncthreads();
        if ((int)threadIdx.x < n_cand) {                              // the segments, ascending
            double acc = 0.0;
            for (int sg = 0; sg < NSEG; ++sg) acc += seg[threadIdx.x][sg];
            chunk_sum[threadIdx.x][cc] = acc;
            chunks[(size_t)threadIdx.x * n_chunks + (size_t)blockIdx.x * kUbmGroupChunks + cc] = acc;
        }
        // xs and v are written again only behind the next chunk's barriers, seg behind two of them
    }
    __syncthreads();
    if ((int)threadIdx.x < n_cand) {
        double acc = 0.0;
        for (int cc = 0; cc < n_here; ++cc) acc += chunk_sum[threadIdx.x][cc];      // ascending chunk
        groups[(size_t)threadIdx.x * n_groups + blockIdx.x] = acc;
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void kmeans_seed_pick_kernel(const float *__restrict__ feats, long n, int step, int n_cand, int n_next,
                                                                    const float *__restrict__ m, const double *__restrict__ chunks, long n_chunks,
                                                                    const double *__restrict__ groups, long n_groups, double *__restrict__ supers, long n_supers,
                                                                    const double *__restrict__ u_next, KmeansSeedCtrl *__restrict__ ctrl)
{
    constexpr int TR = kKmeansMaxTrials;
    __shared__ double total[TR], left_of[TR];
    __shared__ long chunk_of[TR];
    __shared__ int winner, stop;
    __shared__ float wx[kRowLd], mv[kUbmChunkRows];
    if (ctrl->failed) return;
    for (long i = threadIdx.x; i < (long)n_cand * n_supers; i += kThreads) {
        const long q = i / n_supers, s = i - q * n_supers;
        const long g0 = s * kUbmSuperGroups, g1 = g0 + kUbmSuperGroups < n_groups ? g0 + kUbmSuperGroups : n_groups;
        double acc = 0.0;
        for (long g = g0; g < g1; ++g) acc += groups[(size_t)q * n_groups + g];      // ascending group
        supers[(size_t)q * n_supers + s] = acc;
    }
    __syncthreads();
    if ((int)threadIdx.x < n_cand) {
        double acc = 0.0;
        for (long s = 0; s < n_supers; ++s) acc += supers[(size_t)threadIdx.x * n_supers + s];      // ascending super
        total[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int w = 0;
        for (int q = 1; q < n_cand; ++q)
            if (total[q] < total[w]) w = q;                           // ties to the lowest trial
        winner = w;
        ctrl->rows[step] = ctrl->cand[w];
        ctrl->pot[step] = total[w];
        stop = n_next == 0;
        if (n_next > 0 && !(total[w] > 0.0)) {                        // every row sits on a chosen centre: fewer than k distinct rows
            ctrl->failed = 1;
            ctrl->failed_step = step + 1;
            stop = 1;
        }
    }
    __syncthreads();
    if (stop) return;
    const int w = winner;
    const long won = ctrl->rows[step];
    if ((int)threadIdx.x < D) wx[threadIdx.x] = feats[won * D + threadIdx.x];
    if ((int)threadIdx.x < n_next) {
        double r = u_next[threadIdx.x] * total[w];
        const long s = walk_down(supers + (size_t)w * n_supers, 0, n_supers, r);
        const long g0 = s * kUbmSuperGroups;
        const long g = s < 0 ? -1 : walk_down(groups + (size_t)w * n_groups, g0, (g0 + kUbmSuperGroups < n_groups ? g0 + kUbmSuperGroups : n_groups) - g0, r);
        const long c0 = g * kUbmGroupChunks;
        chunk_of[threadIdx.x] = g < 0 ? -1 : walk_down(chunks + (size_t)w * n_chunks, c0, (c0 + kUbmGroupChunks < n_chunks ? c0 + kUbmGroupChunks : n_chunks) - c0, r);
        left_of[threadIdx.x] = r;
    }
    __syncthreads();
    for (int t = 0; t < n_next; ++t) {
        const long r0 = chunk_of[t] * kUbmChunkRows, row = r0 + threadIdx.x;
        float mi = 0.0f;
        if (r0 >= 0 && row < n) {                                     // m with the winner folded in, as the next pass will store it
            float x[D];
#pragma unroll
            for (int j = 0; j < D; ++j) x[j] = feats[row * D + j];
            mi = fminf(m[row], sq_dist<D>(x, wx));
        }
        mv[threadIdx.x] = mi;
        __syncthreads();
        if ((int)threadIdx.x == t) {
            double r = left_of[t];
            const long i = r0 >= 0 ? walk_down(mv, 0, kUbmChunkRows, r) : -1;
            ctrl->cand[t] = i >= 0 ? r0 + i : -1;
            if (i < 0) {                                              // a sum above a chunk without a row: cannot happen, and must not go on
                ctrl->failed = 2;
                ctrl->failed_step = step + 1;
            }
        }
        __syncthreads();
    }
}

// the labelled statistics and their supers; the final pass runs whatever KmeansCtrl::done says
hipError_t launch_kmeans_stats(const KmeansFit &f, int final_pass, hipStream_t stream)
{
    return launch_group_stats(f.model.k, f.model.d, f.n, kmeans_partial_doubles(f.model.k, f.model.d), final_pass ? nullptr : &f.ctrl->done, f.groups, f.supers, stream,
                              [&](auto dc, dim3 grid, dim3 block, size_t lds) {
                                  hipLaunchKernelGGL(kmeans_stats_kernel<decltype(dc)::value>, grid, block, lds, stream, f.feats, f.n,
                                                     GmmModel{f.model.block, f.model.k, f.model.d}, f.ctrl, final_pass, f.labels, f.groups);
                              });
}

}  // namespace

hipError_t launch_kmeans_iterations(const KmeansFit &f, int first, int count, hipStream_t stream)
{
    for (int it = first; it < first + count; ++it) {
        hipError_t e = launch_kmeans_stats(f, 0, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kmeans_update_kernel, dim3(1), dim3(kThreads), 0, stream, f.supers, ubm_supers(f.n), it, f.max_iter, f.shift_limit, f.centres, f.model, f.ctrl);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_kmeans_final(const KmeansFit &f, hipStream_t stream)
{
    const hipError_t e = launch_kmeans_stats(f, 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmeans_gmm_start_kernel, dim3(1), dim3(kThreads), 0, stream, f.supers, ubm_supers(f.n), f.reg_covar, f.params, f.model, f.counts, f.ctrl);
    return hipGetLastError();
}

hipError_t launch_kmeans_seeding(const KmeansSeed &s, long row0, hipStream_t stream)
{
    const long n_chunks = kmeans_chunks(s.n), n_groups = ubm_groups(s.n), n_supers = ubm_supers(s.n);
    if (s.k < 1 || s.k > kGmmMaxK || s.n < s.k || n_groups > (1L << 30) || s.trials < 1 || s.trials > kKmeansMaxTrials || row0 < 0 || row0 >= s.n)
        return hipErrorInvalidValue;
    return dispatch_d(s.d, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        for (int step = 0; step < s.k; ++step) {
            const int n_cand = step == 0 ? 1 : s.trials, n_next = step + 1 < s.k ? s.trials : 0;      // step 0: the one row the host drew
            hipLaunchKernelGGL(kmeans_seed_pass_kernel<D>, dim3((unsigned)n_groups), dim3(kThreads), 0, stream, s.feats, s.n, step, n_cand, s.m, s.ctrl, s.chunks,
                               n_chunks, s.groups, n_groups);
            hipLaunchKernelGGL(kmeans_seed_pick_kernel<D>, dim3(1), dim3(kThreads), 0, stream, s.feats, s.n, step, n_cand, n_next, s.m, s.chunks, n_chunks, s.groups,
                               n_groups, s.supers, n_supers, s.u + (size_t)(step + 1 < s.k ? step + 1 : step) * kKmeansMaxTrials, s.ctrl);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

}  // namespace dsp
