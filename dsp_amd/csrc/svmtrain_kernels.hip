// svmtrain_kernels.hip -- training the scrub-jay RBF-SVM (include/dsp_amd.h dsp_svm_train_*).  Everything after the
// float32 Scaler is float64.  No atomics and no communication between blocks: every sum is taken by one block over a tree its shape
// fixes (a lane's elements ascending, a 6-level xor butterfly inside the wavefront, the wavefronts' partials ascending), so a problem's
// results are the same bits whatever else shares the launch.
#include <climits>

#include "svmtrain_kernels.hpp"

namespace dsp {
namespace {

constexpr int kWaves = kSvmTrainBlock / 64;
constexpr double kTau = 1e-12;                                 // libsvm's TAU

__device__ inline double wave_sum(double v)
{
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// the block's sum in every thread; `scratch` holds kWaves doubles and is free again after the second barrier
__device__ inline double block_sum(double v, double *scratch)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = scratch[0];
    for (int w = 1; w < kWaves; ++w) s += scratch[w];
    __syncthreads();
    return s;
}

__device__ inline double block_max(double v, double *scratch)
{
    for (int s = 32; s > 0; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = scratch[0];
    for (int w = 1; w < kWaves; ++w) m = fmax(m, scratch[w]);
    __syncthreads();
    return m;
}

// (value, index) candidates: the larger value wins, of equal values the lower index
__device__ inline void take_better(double &v, int &i, double v2, int i2)
{
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

__device__ inline void wave_argmax(double &v, int &i)
{
    for (int s = 32; s > 0; s >>= 1) {
        const double v2 = __shfl_xor(v, s, 64);
        const int i2 = __shfl_xor(i, s, 64);
        take_better(v, i, v2, i2);
    }
}

__device__ inline double rbf(double gamma, double d2) { return exp(-gamma * d2); }
// the solver's kernel value: float64, or rounded to float32 as libsvm rounds the rows of Q it caches (svm.cpp Qfloat)
__device__ inline double rbf_q(double gamma, double d2, int q_float32)
{
    const double k = rbf(gamma, d2);
    return q_float32 ? (double)(float)k : k;
}

// ---- Scaler ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSvmTrainBlock) void svm_scaler_kernel(const float *__restrict__ feat, int nf, const int *__restrict__ rows, long n_rows,
                                                                    float *__restrict__ offset, float *__restrict__ scale)
{
    __shared__ double scratch[kWaves];
    const int f = blockIdx.x;
    double s = 0.0;
    for (long k = threadIdx.x; k < n_rows; k += kSvmTrainBlock) s += (double)feat[(size_t)(rows ? rows[k] : k) * nf + f];
    const double mean = block_sum(s, scratch) / (double)n_rows;
    s = 0.0;
    for (long k = threadIdx.x; k < n_rows; k += kSvmTrainBlock) {
        const double d = (double)feat[(size_t)(rows ? rows[k] : k) * nf + f] - mean;
        s = fma(d, d, s);
    }
    const double sd = sqrt(block_sum(s, scratch) / (double)n_rows);
    if (threadIdx.x == 0) {
        offset[f] = (float)mean;
        scale[f] = sd > 0.0 ? (float)(1.0 / sd) : 1.0f;
    }
}

__global__ void svm_standardise_kernel(const float *__restrict__ feat, long total, int nf, const float *__restrict__ offset,
                                       const float *__restrict__ scale, float *__restrict__ z)
{
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const int f = (int)(k % nf);
    z[k] = __fmul_rn(__fsub_rn(feat[k], offset[f]), scale[f]);
}

// ---- distances -------------------------------------------------------------------------------------------------------------------------
// 16 x 16 tiles of the upper triangle; a tile off the diagonal is written twice, as D2[i][j] and D2[j][i].  An element is the same
// chain of fma over the features whichever tile holds it, and (a - b)^2 == (b - a)^2 exactly: the matrix is symmetric bit for bit.
__global__ __launch_bounds__(256) void svm_distance_kernel(const float *__restrict__ z, int n, int nf, double *__restrict__ d2)
{
    if (blockIdx.x < blockIdx.y) return;
    const int i = blockIdx.y * 16 + threadIdx.y, j = blockIdx.x * 16 + threadIdx.x;
    if (i >= n || j >= n) return;
    const float *zi = z + (size_t)i * nf, *zj = z + (size_t)j * nf;
    double acc = 0.0;
    for (int f = 0; f < nf; ++f) {
        const double d = (double)zi[f] - (double)zj[f];
        acc = fma(d, d, acc);
    }
    d2[(size_t)i * n + j] = acc;
    if (blockIdx.x != blockIdx.y) d2[(size_t)j * n + i] = acc;
}

// ---- SMO -------------------------------------------------------------------------------------------------------------------------------
// libsvm's Solver (svm.cpp) without shrinking, one workgroup per problem.  Member t of the problem is row rows[t] of D2; its gradient
// G[t], alpha A[t] and y Y[t] stay in LDS for the problem's lifetime, Q_it = y_i y_t exp(-gamma D2[rows[i]][rows[t]]) is formed from the
// row of D2 as it is read.  Thread x owns members x, x + 256, ...
__global__ __launch_bounds__(kSvmTrainBlock) void svm_smo_kernel(const double *__restrict__ d2, int n, const int *__restrict__ members,
                                                                 const SvmTrainProblem *__restrict__ problems, const int *__restrict__ labels,
                                                                 double eps, int max_iter, int q_float32, double *__restrict__ coef,
                                                                 dsp_svm_train_result *__restrict__ results)
{
    extern __shared__ double lds[];
    __shared__ double s_val[2][kWaves], s_max[kWaves], s_sum[kWaves];
    __shared__ int s_idx[2][kWaves];
    const SvmTrainProblem pr = problems[blockIdx.x];
    const int m = pr.n_members, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (pr.status != DSP_SVM_TRAIN_CONVERGED) {
        if (tid == 0) results[blockIdx.x] = dsp_svm_train_result{0.0, 0.0, 0.0, 0, 0, 0, pr.status};
        return;
    }
    const int *rows = members + pr.first;
    double *G = lds, *A = lds + m;
    signed char *Y = reinterpret_cast<signed char *>(lds + 2 * (size_t)m);
    for (int t = tid; t < m; t += kSvmTrainBlock) {
        G[t] = -1.0;
        A[t] = 0.0;
        Y[t] = labels[rows[t]] == 0 ? 1 : -1;
    }
    __syncthreads();
    const double inf = __builtin_inf();
    int iter = 0, status = DSP_SVM_TRAIN_CONVERGED;
    double gap = 0.0;
    for (;;) {
        // i: the maximum of -y G over I_up
        double best = -inf;
        int bi = INT_MAX;
        for (int t = tid; t < m; t += kSvmTrainBlock) {
            const int y = Y[t];
            const double a = A[t];
            if (y > 0 ? a < pr.c[0] : a > 0.0) {
                const double v = y > 0 ? -G[t] : G[t];
                if (v > best) { best = v; bi = t; }
            }
        }
        wave_argmax(best, bi);
        if (lane == 0) { s_val[0][wave] = best; s_idx[0][wave] = bi; }
        __syncthreads();
        double gmax = s_val[0][0];
        int i = s_idx[0][0];
        for (int w = 1; w < kWaves; ++w) take_better(gmax, i, s_val[0][w], s_idx[0][w]);
        if (i == INT_MAX) { gap = 0.0; break; }                                  // (uniform: no candidate, nothing to improve)
        // j: the second-order rule over I_low with row i, and the maximum of y G there
        const int yi = Y[i];
        const double *di = d2 + (size_t)rows[i] * n;
        double obj = -inf, gmax2 = -inf;                                         // obj = +grad_diff^2 / quad, maximised
        int bj = INT_MAX;
        for (int t = tid; t < m; t += kSvmTrainBlock) {
            const int y = Y[t];
            const double a = A[t];
            if (y > 0 ? a > 0.0 : a < pr.c[1]) {
                const double v = y > 0 ? G[t] : -G[t];
                gmax2 = fmax(gmax2, v);
                const double gd = gmax + v;
                if (gd > 0.0) {
                    double quad = 2.0 - 2.0 * rbf_q(pr.gamma, di[rows[t]], q_float32);
                    if (!(quad > 0.0)) quad = kTau;
                    const double o = gd * gd / quad;
                    if (o > obj) { obj = o; bj = t; }
                }
            }
        }
        wave_argmax(obj, bj);
        for (int s = 32; s > 0; s >>= 1) gmax2 = fmax(gmax2, __shfl_xor(gmax2, s, 64));
        if (lane == 0) { s_val[1][wave] = obj; s_idx[1][wave] = bj; s_max[wave] = gmax2; }
        __syncthreads();
        obj = s_val[1][0];
        int j = s_idx[1][0];
        gmax2 = s_max[0];
        for (int w = 1; w < kWaves; ++w) {
            take_better(obj, j, s_val[1][w], s_idx[1][w]);
            gmax2 = fmax(gmax2, s_max[w]);
        }
        gap = gmax + gmax2;
        if (j == INT_MAX || gap < eps) break;
        if (iter >= max_iter) { status = DSP_SVM_TRAIN_MAX_ITER; break; }
        // the two-variable update, computed by every thread alike
        const int yj = Y[j];
        const double ci = pr.c[yi > 0 ? 0 : 1], cj = pr.c[yj > 0 ? 0 : 1];
        const double gi = G[i], gj = G[j], ai0 = A[i], aj0 = A[j];
        double ai = ai0, aj = aj0;
        double quad = 2.0 - 2.0 * rbf_q(pr.gamma, di[rows[j]], q_float32);
        if (!(quad > 0.0)) quad = kTau;
        if (yi != yj) {
            const double delta = (-gi - gj) / quad, diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) {
                if (aj < 0.0) { aj = 0.0; ai = diff; }
            } else if (ai < 0.0) { ai = 0.0; aj = -diff; }
            if (diff > ci - cj) {
                if (ai > ci) { ai = ci; aj = ci - diff; }
            } else if (aj > cj) { aj = cj; ai = cj + diff; }
        } else {
            const double delta = (gi - gj) / quad, sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > ci) {
                if (ai > ci) { ai = ci; aj = sum - ci; }
            } else if (aj < 0.0) { aj = 0.0; ai = sum; }
            if (sum > cj) {
                if (aj > cj) { aj = cj; ai = sum - cj; }
            } else if (ai < 0.0) { ai = 0.0; aj = sum; }
        }
        const double wi = (double)yi * (ai - ai0), wj = (double)yj * (aj - aj0);
        __syncthreads();                                                         // every thread has read G and A of i and j
        if (tid == 0) { A[i] = ai; A[j] = aj; }
        const double *dj = d2 + (size_t)rows[j] * n;
        for (int t = tid; t < m; t += kSvmTrainBlock) {
            const int r = rows[t];
            const double q = rbf_q(pr.gamma, di[r], q_float32) * wi + rbf_q(pr.gamma, dj[r], q_float32) * wj;
            G[t] += Y[t] > 0 ? q : -q;
        }
        ++iter;
        __syncthreads();
    }
    // rho (libsvm's calculate_rho), the counts and the objective; the alphas
    double sum_free = 0.0, ub = inf, lb = -inf, n_free = 0.0, n_sv = 0.0, n_bounded = 0.0, objective = 0.0;
    for (int t = tid; t < m; t += kSvmTrainBlock) {
        const int y = Y[t];
        const double a = A[t], g = G[t], yg = y > 0 ? g : -g;
        const bool upper = a >= pr.c[y > 0 ? 0 : 1], lower = a <= 0.0;
        if (upper) {
            if (y < 0) ub = fmin(ub, yg); else lb = fmax(lb, yg);
        } else if (lower) {
            if (y > 0) ub = fmin(ub, yg); else lb = fmax(lb, yg);
        } else {
            sum_free += yg;
            n_free += 1.0;
        }
        n_sv += a > 0.0;
        n_bounded += upper;
        objective += a * (g - 1.0);
        coef[(size_t)blockIdx.x * n + rows[t]] = y > 0 ? a : -a;
    }
    sum_free = block_sum(sum_free, s_sum);
    n_free = block_sum(n_free, s_sum);
    n_sv = block_sum(n_sv, s_sum);
    n_bounded = block_sum(n_bounded, s_sum);
    objective = block_sum(objective, s_sum);
    ub = -block_max(-ub, s_sum);
    lb = block_max(lb, s_sum);
    if (tid == 0) {
        const double r = n_free > 0.0 ? sum_free / n_free : (ub + lb) / 2.0;
        results[blockIdx.x] = dsp_svm_train_result{-r, objective / 2.0, gap, iter, (int)n_sv, (int)n_bounded, status};
    }
}

// ---- decisions -------------------------------------------------------------------------------------------------------------------------
// dec[p][r] = sum over p's members t with coef != 0, ascending, of coef_t exp(-gamma D2[rows[t]][r]), + rho: a thread per row, and the
// rows of D2 read along r (the matrix is symmetric)
__global__ __launch_bounds__(256) void svm_decision_kernel(const double *__restrict__ d2, int n, const int *__restrict__ members,
                                                           const SvmTrainProblem *__restrict__ problems, const double *__restrict__ coef,
                                                           const dsp_svm_train_result *__restrict__ results, double *__restrict__ dec)
{
    const SvmTrainProblem pr = problems[blockIdx.y];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double *out = dec + (size_t)blockIdx.y * n;
    if (pr.status != DSP_SVM_TRAIN_CONVERGED) { out[r] = pr.fill; return; }
    const int *rows = members + pr.first;
    const double *cf = coef + (size_t)blockIdx.y * n;
    double acc = 0.0;
    for (int t = 0; t < pr.n_members; ++t) {
        const int row = rows[t];
        const double c = cf[row];
        if (c != 0.0) acc += c * rbf(pr.gamma, d2[(size_t)row * n + r]);
    }
    out[r] = acc + results[blockIdx.y].rho;
}

__global__ void svm_gather_cv_kernel(const double *__restrict__ dec, int n, const int *__restrict__ fold_ids, double *__restrict__ dec_cv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dec_cv[i] = dec[(size_t)fold_ids[i] * n + i];
}

// ---- Platt -----------------------------------------------------------------------------------------------------------------------------
// libsvm's sigmoid_train with its constants; label 0 is the positive class
__device__ inline double platt_objective(const double *__restrict__ dec, const int *__restrict__ labels, const int *__restrict__ rows, long n,
                                         double a, double b, double hi, double lo, double *scratch)
{
    double s = 0.0;
    for (long k = threadIdx.x; k < n; k += kSvmTrainBlock) {
        const long r = rows ? rows[k] : k;
        const double t = labels[r] == 0 ? hi : lo, f = dec[r] * a + b;
        s += f >= 0.0 ? t * f + log(1.0 + exp(-f)) : (t - 1.0) * f + log(1.0 + exp(f));
    }
    return block_sum(s, scratch);
}

__global__ __launch_bounds__(kSvmTrainBlock) void svm_platt_kernel(const double *__restrict__ dec, const int *__restrict__ labels,
                                                                   const int *__restrict__ rows, long n, SvmPlattOut *__restrict__ out)
{
    __shared__ double scratch[kWaves];
    double p1 = 0.0;
    for (long k = threadIdx.x; k < n; k += kSvmTrainBlock) p1 += labels[rows ? rows[k] : k] == 0;
    const double prior1 = block_sum(p1, scratch), prior0 = (double)n - prior1;
    const double hi = (prior1 + 1.0) / (prior1 + 2.0), lo = 1.0 / (prior0 + 2.0);
    const double min_step = 1e-10, sigma = 1e-12, eps = 1e-5;
    double a = 0.0, b = log((prior0 + 1.0) / (prior1 + 1.0));
    double fval = platt_objective(dec, labels, rows, n, a, b, hi, lo, scratch);
    int iter = 0;
    for (; iter < kSvmPlattMaxIter; ++iter) {
        double h11 = 0.0, h22 = 0.0, h21 = 0.0, g1 = 0.0, g2 = 0.0;
        for (long k = threadIdx.x; k < n; k += kSvmTrainBlock) {
            const long r = rows ? rows[k] : k;
            const double x = dec[r], t = labels[r] == 0 ? hi : lo, f = x * a + b;
            double p, q;
            if (f >= 0.0) {
                const double e = exp(-f);
                p = e / (1.0 + e);
                q = 1.0 / (1.0 + e);
            } else {
                const double e = exp(f);
                p = 1.0 / (1.0 + e);
                q = e / (1.0 + e);
            }
            const double w = p * q, d1 = t - p;
            h11 += x * x * w;
            h22 += w;
            h21 += x * w;
            g1 += x * d1;
            g2 += d1;
        }
        h11 = sigma + block_sum(h11, scratch);
        h22 = sigma + block_sum(h22, scratch);
        h21 = block_sum(h21, scratch);
        g1 = block_sum(g1, scratch);
        g2 = block_sum(g2, scratch);
        if (fabs(g1) < eps && fabs(g2) < eps) break;
        const double det = h11 * h22 - h21 * h21;
        const double da = -(h22 * g1 - h21 * g2) / det, db = -(-h21 * g1 + h11 * g2) / det, gd = g1 * da + g2 * db;
        double step = 1.0;
        while (step >= min_step) {
            const double na = a + step * da, nb = b + step * db;
            const double nf = platt_objective(dec, labels, rows, n, na, nb, hi, lo, scratch);
            if (nf < fval + 0.0001 * step * gd) { a = na; b = nb; fval = nf; break; }
            step /= 2.0;
        }
        if (step < min_step) break;                                               // (the line search fails)
    }
    if (threadIdx.x == 0) *out = SvmPlattOut{a, b, iter, 0};
}

}  // namespace

hipError_t launch_svm_scaler_fit(const float *feat, int n_features, const int *rows, long n_rows, float *offset, float *scale, hipStream_t stream)
{
    hipLaunchKernelGGL(svm_scaler_kernel, dim3(n_features), dim3(kSvmTrainBlock), 0, stream, feat, n_features, rows, n_rows, offset, scale);
    return hipGetLastError();
}

hipError_t launch_svm_distances(const float *feat, long n, int n_features, const float *offset, const float *scale, float *z, double *d2,
                                hipStream_t stream)
{
    const long total = n * n_features;
    hipLaunchKernelGGL(svm_standardise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, feat, total, n_features, offset, scale, z);
    const unsigned tiles = (unsigned)((n + 15) / 16);
    hipLaunchKernelGGL(svm_distance_kernel, dim3(tiles, tiles), dim3(16, 16), 0, stream, z, (int)n, n_features, d2);
    return hipGetLastError();
}

hipError_t launch_svm_smo(const double *d2, long n, const int *members, const SvmTrainProblem *problems, long n_problems, int max_members,
                          const int *labels, double eps, int max_iter, int q_float32, double *coef, dsp_svm_train_result *results, hipStream_t stream)
{
    const size_t lds = svm_smo_lds_bytes(max_members);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(svm_smo_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(svm_smo_kernel, dim3((unsigned)n_problems), dim3(kSvmTrainBlock), lds, stream, d2, (int)n, members, problems, labels, eps,
                       max_iter, q_float32, coef, results);
    return hipGetLastError();
}

hipError_t launch_svm_decisions(const double *d2, long n, const int *members, const SvmTrainProblem *problems, long n_problems,
                                const double *coef, const dsp_svm_train_result *results, double *dec, hipStream_t stream)
{
    hipLaunchKernelGGL(svm_decision_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_problems), dim3(256), 0, stream, d2, (int)n, members, problems,
                       coef, results, dec);
    return hipGetLastError();
}

hipError_t launch_svm_gather_cv(const double *dec, long n, const int *fold_ids, double *dec_cv, hipStream_t stream)
{
    hipLaunchKernelGGL(svm_gather_cv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dec, (int)n, fold_ids, dec_cv);
    return hipGetLastError();
}

hipError_t launch_svm_platt(const double *dec, const int *labels, const int *rows, long n_rows, SvmPlattOut *out, hipStream_t stream)
{
    hipLaunchKernelGGL(svm_platt_kernel, dim3(1), dim3(kSvmTrainBlock), 0, stream, dec, labels, rows, n_rows, out);
    return hipGetLastError();
}

}  // namespace dsp
