// stoptrain_kernels.hip -- training the stop-word net (include/dsp_amd.h dsp_stop_train_*): many Keras-style fits per
// launch, one workgroup per run.  Everything after the float32 Scaler is float64.  No atomics and no communication between blocks: every
// sum is taken by one block in an order its shape fixes (a lane's features ascending, a 6-level xor butterfly inside the wavefront, the
// four wavefronts' partials as (0 + 1) + (2 + 3); batch samples and validation rows ascending), so a run's outputs are the same bits
// whatever else shares the launch.
//
// A run's layer-1 kernel, its Adam moments and the best snapshot live in the run's slab in HBM (f_used x u1 doubles each); lanes own the
// features lane, lane + 256, ...  Layers 2-4 and bias1 (the "small" parameters, at most 577) are in LDS during a launch, their moments and
// snapshot in the slab behind layer 1's.
#include <algorithm>
#include <cmath>

#include "stoptrain_kernels.hpp"

namespace dsp {
namespace {

constexpr int kBlock = kStopTrainBlock, kWaves = kBlock / 64, kSub = kStopTrainSub, kU = kStopTrainMaxUnits, kMaxSmall = 16 + 272 + 272 + 17;
constexpr double kBeta1 = 0.9, kBeta2 = 0.999, kAdamEps = 1e-7;

__device__ inline double wave_sum(double v)
{
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ inline double block_sum(double v, double *scratch)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    __syncthreads();
    return s;
}

// input c * max_frames + t of clip `row` of the ragged matrix: frames past the clip's end are 0
__device__ inline float clip_input(const float *__restrict__ mfcc, const long *__restrict__ offsets, long row, int c, int t, int n_coef)
{
    const long r0 = offsets[row], r1 = offsets[row + 1];
    return t < r1 - r0 ? mfcc[(size_t)(r0 + t) * n_coef + c] : 0.0f;
}

// ---- Scaler and the standardised rows -------------------------------------------------------------------------------------------------
// one block per input; the sums are float64, a lane's rows ascending, without contraction so that the restatement can take the same tree
__global__ __launch_bounds__(kBlock) void stop_train_scaler_kernel(const float *__restrict__ mfcc, const long *__restrict__ offsets, StopTrainShape s,
                                                                   const int *__restrict__ rows, long n_rows, float *__restrict__ mean_out,
                                                                   float *__restrict__ scale_out)
{
    __shared__ double scratch[kWaves];
    const long j = blockIdx.x;
    const int c = (int)(j / s.max_frames), t = (int)(j - (long)c * s.max_frames);
    if (t >= s.t_used) {                                         // zero for every clip
        if (threadIdx.x == 0) { mean_out[j] = 0.0f; scale_out[j] = 1.0f; }
        return;
    }
    double sum = 0.0;
    for (long k = threadIdx.x; k < n_rows; k += kBlock) sum = __dadd_rn(sum, (double)clip_input(mfcc, offsets, rows ? rows[k] : k, c, t, s.n_coef));
    const double mean = block_sum(sum, scratch) / (double)n_rows;
    sum = 0.0;
    for (long k = threadIdx.x; k < n_rows; k += kBlock) {
        const double d = __dsub_rn((double)clip_input(mfcc, offsets, rows ? rows[k] : k, c, t, s.n_coef), mean);
        sum = __dadd_rn(sum, __dmul_rn(d, d));
    }
    const double sd = sqrt(block_sum(sum, scratch) / (double)n_rows);
    if (threadIdx.x == 0) {
        mean_out[j] = (float)mean;
        scale_out[j] = sd > 0.0 ? (float)sd : 1.0f;
    }
}

__global__ void stop_train_standardise_kernel(const float *__restrict__ mfcc, const long *__restrict__ offsets, long n, StopTrainShape s,
                                              const float *__restrict__ mean, const float *__restrict__ scale, float *__restrict__ z)
{
    const size_t total = (size_t)n * s.f_used;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const long row = (long)(e / s.f_used);
        const int f = (int)(e - (size_t)row * s.f_used), c = f / s.t_used, t = f - c * s.t_used;
        const long j = (long)c * s.max_frames + t;
        const float div = scale[j] == 0.0f ? 1.0f : scale[j];
        z[e] = (clip_input(mfcc, offsets, row, c, t, s.n_coef) - mean[j]) / div;     // the inference kernels' expression (consumer_kernels.hip)
    }
}

// ---- a run's pieces ----------------------------------------------------------------------------------------------------------------------
struct Slab {
    double *w1, *m1, *v1, *best1, *ws, *ms, *vs, *bests;
};
__device__ inline Slab slab_of(double *slabs, const StopTrainShape &s, long p)
{
    const size_t n1 = (size_t)s.f_used * s.u1;
    double *b = slabs + (size_t)p * (4 * (n1 + s.n_small));
    return Slab{b, b + n1, b + 2 * n1, b + 3 * n1, b + 4 * n1, b + 4 * n1 + s.n_small, b + 4 * n1 + 2 * s.n_small, b + 4 * n1 + 3 * s.n_small};
}

// flat index of used feature f's kernel1 row
__device__ inline long full_input(const StopTrainShape &s, int f)
{
    const int c = f / s.t_used;
    return (long)c * s.max_frames + (f - c * s.t_used);
}

// the Glorot limit of small parameter k (0 for a bias)
__device__ inline double small_limit(const StopTrainShape &s, int k)
{
    if (k < s.o_w2) return 0.0;
    if (k < s.o_b2) return s.limit[1];
    if (k < s.o_w3) return 0.0;
    if (k < s.o_b3) return s.limit[2];
    if (k < s.o_w4) return 0.0;
    if (k < s.o_b4) return s.limit[3];
    return 0.0;
}

// The LDS of the epoch and finish kernels: 57 KB.
struct Lds {
    double a1[kStopTrainMaxBatch * kU];            // layer 1 of the batch: pre-activation, then activation (dropout applied), then delta
    double h2[kSub * kU], h3[kSub * kU], d1[kSub * kU], d2[kSub * kU], d3[kSub * kU];     // the sub-batch's layers 2-3 and deltas
    double d4[kSub];
    double loss[kStopTrainMaxBatch];
    double logit[kStopTrainMaxBatch];
    double small[kMaxSmall];
    double xch[kWaves * 32];
    int row[kStopTrainMaxBatch];
    int alive[3 * kU];
};

// layer 1 of samples lds.row[0 .. B): a1[b][j] = bias1[j] + sum_f z[row_b][f] w1[f][j].  CH = 32 / U1P samples at a time, so that the
// partial sums of a chunk are 32 registers a lane.
template <int U1P>
__device__ inline void layer1_forward(const StopTrainShape &s, const float *__restrict__ z, const double *w1, int B, Lds &lds)
{
    constexpr int CH = 32 / U1P;
    const int u1 = s.u1, fu = s.f_used;
    for (int c0 = 0; c0 < B; c0 += CH) {
        double acc[CH][U1P];
        size_t zr[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            zr[c] = (size_t)lds.row[c0 + c < B ? c0 + c : c0] * fu;
#pragma unroll
            for (int j = 0; j < U1P; ++j) acc[c][j] = 0.0;
        }
        for (int f = threadIdx.x; f < fu; f += kBlock) {
            double w[U1P];
#pragma unroll
            for (int j = 0; j < U1P; ++j) w[j] = j < u1 ? w1[(size_t)f * u1 + j] : 0.0;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const double x = (double)z[zr[c] + f];
#pragma unroll
                for (int j = 0; j < U1P; ++j) acc[c][j] = fma(x, w[j], acc[c][j]);
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int j = 0; j < U1P; ++j) {
                const double v = wave_sum(acc[c][j]);
                if ((threadIdx.x & 63) == 0) lds.xch[(threadIdx.x >> 6) * 32 + c * U1P + j] = v;
            }
        __syncthreads();
        if (threadIdx.x < 32) {
            const int c = threadIdx.x / U1P, j = threadIdx.x - c * U1P;
            if (c0 + c < B && j < u1)
                lds.a1[(c0 + c) * kU + j] = ((lds.xch[threadIdx.x] + lds.xch[32 + threadIdx.x]) + (lds.xch[64 + threadIdx.x] + lds.xch[96 + threadIdx.x])) + lds.small[j];
        }
        __syncthreads();
    }
}

__device__ inline double dropped(double h, bool train, double rate, double keep_scale, uint64_t seed, uint64_t gstep, int layer, int slot, int unit)
{
    if (!train || !(rate > 0.0)) return h;
    const uint64_t counter = (((gstep * 3 + (uint64_t)layer) * 256 + (uint64_t)slot) * 16 + (uint64_t)unit);
    return stop_train_uniform(seed, 2, counter) >= rate ? h * keep_scale : 0.0;
}

// Layers 2-4 of batch sample `slot` (sub-batch position sb), from its layer-1 pre-activations in lds.a1: the activations are left in
// a1 / h2 / h3, the logit is returned.  alive (may be nullptr): units with a positive activation are marked.
__device__ inline double sample_forward(const StopTrainShape &s, const StopTrainRun &run, Lds &lds, int slot, int sb, bool train, uint64_t gstep, bool mark)
{
    double *h1 = lds.a1 + slot * kU, *h2 = lds.h2 + sb * kU, *h3 = lds.h3 + sb * kU;
    const double *w2 = lds.small + s.o_w2, *b2 = lds.small + s.o_b2, *w3 = lds.small + s.o_w3, *b3 = lds.small + s.o_b3, *w4 = lds.small + s.o_w4;
    for (int j = 0; j < s.u1; ++j) {
        const double pre = h1[j];
        h1[j] = dropped(pre > 0.0 ? pre : 0.0, train, run.rate[0], run.keep_scale[0], run.seed, gstep, 0, slot, j);
        if (mark && h1[j] > 0.0) lds.alive[j] = 1;
    }
    for (int o = 0; o < s.u2; ++o) {
        double a = b2[o];
        for (int i = 0; i < s.u1; ++i) a = fma(h1[i], w2[i * s.u2 + o], a);
        h2[o] = dropped(a > 0.0 ? a : 0.0, train, run.rate[1], run.keep_scale[1], run.seed, gstep, 1, slot, o);
        if (mark && h2[o] > 0.0) lds.alive[kU + o] = 1;
    }
    for (int o = 0; o < s.u3; ++o) {
        double a = b3[o];
        for (int i = 0; i < s.u2; ++i) a = fma(h2[i], w3[i * s.u3 + o], a);
        h3[o] = dropped(a > 0.0 ? a : 0.0, train, run.rate[2], run.keep_scale[2], run.seed, gstep, 2, slot, o);
        if (mark && h3[o] > 0.0) lds.alive[2 * kU + o] = 1;
    }
    double a = lds.small[s.o_b4];
    for (int i = 0; i < s.u3; ++i) a = fma(h3[i], w4[i], a);
    return a;
}

__device__ inline double bce_from_logit(double a, double y) { return fmax(a, 0.0) - a * y + log1p(exp(-fabs(a))); }
__device__ inline double sigmoid(double a)
{
    const double e = exp(-fabs(a));
    return a >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// the deltas of sample `slot` behind sample_forward: d4, d3, d2 and d1 of the sub-batch
__device__ inline void sample_backward(const StopTrainShape &s, const StopTrainRun &run, Lds &lds, int slot, int sb, double dlogit)
{
    const double *h1 = lds.a1 + slot * kU, *h2 = lds.h2 + sb * kU, *h3 = lds.h3 + sb * kU;
    double *d1 = lds.d1 + sb * kU, *d2 = lds.d2 + sb * kU, *d3 = lds.d3 + sb * kU;
    const double *w2 = lds.small + s.o_w2, *w3 = lds.small + s.o_w3, *w4 = lds.small + s.o_w4;
    lds.d4[sb] = dlogit;
    for (int i = 0; i < s.u3; ++i) d3[i] = h3[i] > 0.0 ? dlogit * w4[i] * run.keep_scale[2] : 0.0;
    for (int i = 0; i < s.u2; ++i) {
        double g = 0.0;
        for (int o = 0; o < s.u3; ++o) g = fma(d3[o], w3[i * s.u3 + o], g);
        d2[i] = h2[i] > 0.0 ? g * run.keep_scale[1] : 0.0;
    }
    for (int i = 0; i < s.u1; ++i) {
        double g = 0.0;
        for (int o = 0; o < s.u2; ++o) g = fma(d2[o], w2[i * s.u2 + o], g);
        d1[i] = h1[i] > 0.0 ? g * run.keep_scale[0] : 0.0;
    }
}

// the sub-batch's share of the gradient of small parameter k: samples ascending
__device__ inline double small_gradient(const StopTrainShape &s, const Lds &lds, int k, int slot0, int count, double g)
{
    const double *out;
    const double *in = nullptr;
    int in_stride = kU, o, i = 0;
    if (k < s.o_w2) { out = lds.d1; o = k; }
    else if (k < s.o_b2) { out = lds.d2; in = lds.a1 + slot0 * kU; i = (k - s.o_w2) / s.u2; o = (k - s.o_w2) - i * s.u2; }
    else if (k < s.o_w3) { out = lds.d2; o = k - s.o_b2; }
    else if (k < s.o_b3) { out = lds.d3; in = lds.h2; i = (k - s.o_w3) / s.u3; o = (k - s.o_w3) - i * s.u3; }
    else if (k < s.o_w4) { out = lds.d3; o = k - s.o_b3; }
    else if (k < s.o_b4) { out = lds.d4; in = lds.h3; i = k - s.o_w4; o = 0; }
    else { out = lds.d4; o = 0; }
    const int out_stride = k >= s.o_w4 ? 1 : kU;
    for (int b = 0; b < count; ++b) g = in ? fma(in[b * in_stride + i], out[b * out_stride + o], g) : g + out[b * out_stride + o];
    return g;
}

__device__ inline void adam(double &w, double &m, double &v, double g, double lr_t)
{
    m = kBeta1 * m + (1.0 - kBeta1) * g;
    v = kBeta2 * v + (1.0 - kBeta2) * (g * g);
    w -= lr_t * m / (sqrt(v) + kAdamEps);
}

// the logits of rows[0 .. count) (nullptr: rows first, first + 1, ...) without dropout into lds.logit, a chunk of at most 256
template <int U1P>
__device__ inline void eval_chunk(const StopTrainShape &s, const StopTrainRun &run, const float *__restrict__ z, const double *w1,
                                  const int *__restrict__ rows, long first, int count, Lds &lds, bool mark)
{
    for (int b = threadIdx.x; b < count; b += kBlock) lds.row[b] = rows ? rows[first + b] : (int)(first + b);
    __syncthreads();
    layer1_forward<U1P>(s, z, w1, count, lds);
    for (int b0 = 0; b0 < count; b0 += kSub) {
        const int sb = threadIdx.x;
        if (sb < kSub && b0 + sb < count) lds.logit[b0 + sb] = sample_forward(s, run, lds, b0 + sb, sb, false, 0, mark);
    }
    __syncthreads();
}

// ---- the kernels ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void stop_train_init_kernel(StopTrainShape s, const StopTrainRun *__restrict__ runs, int max_epochs,
                                                                 double *slabs, StopTrainState *__restrict__ states, int *__restrict__ stop,
                                                                 double *__restrict__ history)
{
    const long p = blockIdx.x;
    const StopTrainRun run = runs[p];
    const Slab sl = slab_of(slabs, s, p);
    for (int e = threadIdx.x; e < s.f_used * s.u1; e += kBlock) {
        const int f = e / s.u1, j = e - f * s.u1;
        const double w = stop_train_glorot(run.seed, (uint64_t)(full_input(s, f) * s.u1 + j), s.limit[0]);
        sl.w1[e] = w; sl.best1[e] = w; sl.m1[e] = 0.0; sl.v1[e] = 0.0;
    }
    for (int k = threadIdx.x; k < s.n_small; k += kBlock) {
        const double lim = small_limit(s, k);
        const double w = lim > 0.0 ? stop_train_glorot(run.seed, (uint64_t)(s.n_in * s.u1 + k), lim) : 0.0;
        sl.ws[k] = w; sl.bests[k] = w; sl.ms[k] = 0.0; sl.vs[k] = 0.0;
    }
    for (int e = threadIdx.x; e < 2 * max_epochs; e += kBlock) history[(size_t)p * 2 * max_epochs + e] = __builtin_nan("");
    if (threadIdx.x == 0) {
        const int status = run.n_train == 0 ? DSP_STOP_TRAIN_EMPTY : (run.n_val == 0 ? DSP_STOP_TRAIN_NO_VALIDATION : DSP_STOP_TRAIN_MAX_EPOCHS);
        states[p] = StopTrainState{__builtin_inf(), __builtin_nan(""), 0, 0, -1, 0, status};
        stop[p] = run.n_train == 0;
    }
}

template <int U1P>
__global__ __launch_bounds__(kBlock) void stop_train_epoch_kernel(StopTrainShape s, const float *__restrict__ z, const int *__restrict__ labels,
                                                                  const int *__restrict__ members, const StopTrainRun *__restrict__ runs, int epoch,
                                                                  int max_epochs, double *slabs, StopTrainState *__restrict__ states,
                                                                  int *__restrict__ stop, double *__restrict__ history)
{
    const long p = blockIdx.x;
    if (stop[p]) return;
    __shared__ Lds lds;
    __shared__ double sh_sum[2];
    const StopTrainRun run = runs[p];
    const Slab sl = slab_of(slabs, s, p);
    StopTrainState st = states[p];
    for (int k = threadIdx.x; k < s.n_small; k += kBlock) lds.small[k] = sl.ws[k];
    __syncthreads();
    const uint64_t key = stop_train_draw(run.seed, 1, (uint64_t)epoch);
    const int n_steps = (run.n_train + run.batch - 1) / run.batch;
    double epoch_loss = 0.0;                                     // (thread 0's)
    for (int step = 0; step < n_steps; ++step) {
        const int B = min(run.batch, run.n_train - step * run.batch);
        const uint64_t gstep = (uint64_t)st.step;
        for (int b = threadIdx.x; b < B; b += kBlock)
            lds.row[b] = members[run.train_first + stop_train_order_at((uint32_t)run.n_train, key, (uint32_t)(step * run.batch + b))];
        __syncthreads();
        layer1_forward<U1P>(s, z, sl.w1, B, lds);
        // layers 2-4 forward and backward, a sub-batch at a time; every thread owns up to three small parameters' gradients
        double g[3] = {0.0, 0.0, 0.0};
        for (int b0 = 0; b0 < B; b0 += kSub) {
            const int count = min(kSub, B - b0), sb = threadIdx.x;
            if (sb < count) {
                const int slot = b0 + sb;
                const double y = (double)labels[lds.row[slot]];
                const double a = sample_forward(s, run, lds, slot, sb, true, gstep, false);
                lds.loss[slot] = bce_from_logit(a, y);
                sample_backward(s, run, lds, slot, sb, (sigmoid(a) - y) / (double)B);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int k = threadIdx.x + q * kBlock;
                if (k < s.n_small) g[q] = small_gradient(s, lds, k, b0, count, g[q]);
            }
            __syncthreads();
            // layer 1's deltas take the place of its activations
            for (int e = threadIdx.x; e < count * kU; e += kBlock) lds.a1[b0 * kU + e] = lds.d1[e];
            __syncthreads();
        }
        const double t = (double)(st.step + 1);
        const double lr_t = run.lr * sqrt(1.0 - pow(kBeta2, t)) / (1.0 - pow(kBeta1, t));
        // layer 1: a lane's features, batch samples ascending, then Adam in place
        for (int f = threadIdx.x; f < s.f_used; f += kBlock) {
            double g1[U1P];
#pragma unroll
            for (int j = 0; j < U1P; ++j) g1[j] = 0.0;
            for (int b = 0; b < B; ++b) {
                const double x = (double)z[(size_t)lds.row[b] * s.f_used + f];
#pragma unroll
                for (int j = 0; j < U1P; ++j)
                    if (j < s.u1) g1[j] = fma(x, lds.a1[b * kU + j], g1[j]);
            }
#pragma unroll
            for (int j = 0; j < U1P; ++j)
                if (j < s.u1) {
                    const size_t e = (size_t)f * s.u1 + j;
                    double w = sl.w1[e], m = sl.m1[e], v = sl.v1[e];
                    adam(w, m, v, g1[j], lr_t);
                    sl.w1[e] = w; sl.m1[e] = m; sl.v1[e] = v;
                }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = threadIdx.x + q * kBlock;
            if (k < s.n_small) {
                double w = lds.small[k], m = sl.ms[k], v = sl.vs[k];
                adam(w, m, v, g[q], lr_t);
                lds.small[k] = w; sl.ms[k] = m; sl.vs[k] = v;
            }
        }
        if (threadIdx.x == 0) {
            double sum = 0.0;
            for (int b = 0; b < B; ++b) sum += lds.loss[b];
            epoch_loss += sum / (double)B * (double)B;
        }
        ++st.step;
        __syncthreads();                                         // the step's stores to w1 and small are visible to the block
    }
    // validation: rows ascending, dropout off
    double val_sum = 0.0;                                        // (thread 0's)
    for (long v0 = 0; v0 < run.n_val; v0 += kStopTrainMaxBatch) {
        const int count = (int)min((long)kStopTrainMaxBatch, run.n_val - v0);
        eval_chunk<U1P>(s, run, z, sl.w1, members + run.val_first, v0, count, lds, false);
        if (threadIdx.x == 0)
            for (int b = 0; b < count; ++b) val_sum += bce_from_logit(lds.logit[b], (double)labels[lds.row[b]]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sh_sum[0] = epoch_loss / (double)run.n_train;
        sh_sum[1] = run.n_val ? val_sum / (double)run.n_val : __builtin_nan("");
    }
    __syncthreads();
    const double loss = sh_sum[0], val_loss = sh_sum[1];
    // early stopping as Keras's callback keeps it; every thread takes the same decision
    st.last_loss = loss;
    st.n_epochs = epoch + 1;
    bool done = epoch + 1 >= run.epochs;
    if (run.n_val) {
        if (val_loss < st.best) {
            st.best = val_loss; st.best_epoch = epoch; st.wait = 0;
            for (int e = threadIdx.x; e < s.f_used * s.u1; e += kBlock) sl.best1[e] = sl.w1[e];
            for (int k = threadIdx.x; k < s.n_small; k += kBlock) sl.bests[k] = lds.small[k];
        } else if (++st.wait >= run.patience) {
            done = true;
            st.status = DSP_STOP_TRAIN_CONVERGED_EARLY;
        }
    }
    for (int k = threadIdx.x; k < s.n_small; k += kBlock) sl.ws[k] = lds.small[k];
    if (threadIdx.x == 0) {
        history[((size_t)p * max_epochs + epoch) * 2] = loss;
        history[((size_t)p * max_epochs + epoch) * 2 + 1] = val_loss;
        states[p] = st;
        if (done) stop[p] = 1;
    }
}

template <int U1P>
__global__ __launch_bounds__(kBlock) void stop_train_finish_kernel(StopTrainShape s, const float *__restrict__ z, long n, const int *__restrict__ labels,
                                                                   const int *__restrict__ members, const StopTrainRun *__restrict__ runs,
                                                                   double *slabs, const StopTrainState *__restrict__ states,
                                                                   double *__restrict__ params, double *__restrict__ prob,
                                                                   dsp_stop_train_result *__restrict__ results)
{
    __shared__ Lds lds;
    __shared__ int sh_count;
    const long p = blockIdx.x;
    const StopTrainRun run = runs[p];
    const Slab sl = slab_of(slabs, s, p);
    const StopTrainState st = states[p];
    // Keras 3's on_train_end: the best snapshot when there is one and restore_best is set, else the last weights
    const bool best = run.restore_best && run.n_val && st.best_epoch >= 0;
    const double *w1 = best ? sl.best1 : sl.w1, *small = best ? sl.bests : sl.ws;
    for (int k = threadIdx.x; k < s.n_small; k += kBlock) lds.small[k] = small[k];
    for (int k = threadIdx.x; k < 3 * kU; k += kBlock) lds.alive[k] = 0;
    if (threadIdx.x == 0) sh_count = 0;
    __syncthreads();
    // the flat parameters: kernel1 rows of the unused inputs keep their initial draw
    double *out = params + (size_t)p * s.n_params;
    for (long e = threadIdx.x; e < s.n_in * s.u1; e += kBlock) {
        const long j = e / s.u1;
        const int u = (int)(e - j * s.u1), c = (int)(j / s.max_frames), t = (int)(j - (long)c * s.max_frames);
        out[e] = t < s.t_used ? w1[(size_t)(c * s.t_used + t) * s.u1 + u] : stop_train_glorot(run.seed, (uint64_t)e, s.limit[0]);
    }
    for (int k = threadIdx.x; k < s.n_small; k += kBlock) out[s.n_in * s.u1 + k] = lds.small[k];
    // P(stop) of every row of the dataset
    if (prob)
        for (long r0 = 0; r0 < n; r0 += kStopTrainMaxBatch) {
            const int count = (int)min((long)kStopTrainMaxBatch, n - r0);
            eval_chunk<U1P>(s, run, z, w1, nullptr, r0, count, lds, false);
            for (int b = threadIdx.x; b < count; b += kBlock) prob[(size_t)p * n + r0 + b] = sigmoid(lds.logit[b]);
            __syncthreads();
        }
    // the validation rows on the right side of 0.5
    for (long v0 = 0; v0 < run.n_val; v0 += kStopTrainMaxBatch) {
        const int count = (int)min((long)kStopTrainMaxBatch, run.n_val - v0);
        eval_chunk<U1P>(s, run, z, w1, members + run.val_first, v0, count, lds, false);
        if (threadIdx.x == 0)
            for (int b = 0; b < count; ++b) sh_count += (sigmoid(lds.logit[b]) > 0.5) == (labels[lds.row[b]] == 1);
        __syncthreads();
    }
    // hidden units that are 0 on every training row (several lanes may store the same 1)
    for (long v0 = 0; v0 < run.n_train; v0 += kStopTrainMaxBatch) {
        const int count = (int)min((long)kStopTrainMaxBatch, run.n_train - v0);
        eval_chunk<U1P>(s, run, z, w1, members + run.train_first, v0, count, lds, true);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int dead = 0;
        for (int j = 0; j < s.u1; ++j) dead += !lds.alive[j];
        for (int j = 0; j < s.u2; ++j) dead += !lds.alive[kU + j];
        for (int j = 0; j < s.u3; ++j) dead += !lds.alive[2 * kU + j];
        dsp_stop_train_result r;
        r.best_val_loss = st.best_epoch >= 0 ? st.best : __builtin_nan("");
        r.last_loss = st.last_loss;
        r.n_epochs = st.n_epochs;
        r.best_epoch = st.best_epoch;
        r.status = st.status;
        r.val_correct = sh_count;
        r.n_dead_units = run.n_train ? dead : 0;
        r.reserved = 0;
        results[p] = r;
    }
}

int padded_units(int u1) { return u1 <= 4 ? 4 : (u1 <= 8 ? 8 : 16); }

}  // namespace

hipError_t launch_stop_train_scaler(const float *mfcc, const long *offsets, const StopTrainShape &s, const int *rows, long n_rows, float *mean,
                                    float *scale, hipStream_t stream)
{
    hipLaunchKernelGGL(stop_train_scaler_kernel, dim3((unsigned)s.n_in), dim3(kBlock), 0, stream, mfcc, offsets, s, rows, n_rows, mean, scale);
    return hipGetLastError();
}

hipError_t launch_stop_train_standardise(const float *mfcc, const long *offsets, long n, const StopTrainShape &s, const float *mean,
                                         const float *scale, float *z, hipStream_t stream)
{
    const size_t total = (size_t)n * s.f_used;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(stop_train_standardise_kernel, dim3(blocks), dim3(256), 0, stream, mfcc, offsets, n, s, mean, scale, z);
    return hipGetLastError();
}

hipError_t launch_stop_train_init(const StopTrainShape &s, const StopTrainRun *runs, long n_runs, int max_epochs, double *slabs,
                                  StopTrainState *states, int *stop, double *history, hipStream_t stream)
{
    hipLaunchKernelGGL(stop_train_init_kernel, dim3((unsigned)n_runs), dim3(kBlock), 0, stream, s, runs, max_epochs, slabs, states, stop, history);
    return hipGetLastError();
}

hipError_t launch_stop_train_epoch(const StopTrainShape &s, const float *z, const int *labels, const int *members, const StopTrainRun *runs,
                                   long n_runs, int epoch, int max_epochs, double *slabs, StopTrainState *states, int *stop, double *history,
                                   hipStream_t stream)
{
    const dim3 grid((unsigned)n_runs), block(kBlock);
    switch (padded_units(s.u1)) {
    case 4: hipLaunchKernelGGL(stop_train_epoch_kernel<4>, grid, block, 0, stream, s, z, labels, members, runs, epoch, max_epochs, slabs, states, stop, history); break;
    case 8: hipLaunchKernelGGL(stop_train_epoch_kernel<8>, grid, block, 0, stream, s, z, labels, members, runs, epoch, max_epochs, slabs, states, stop, history); break;
    default: hipLaunchKernelGGL(stop_train_epoch_kernel<16>, grid, block, 0, stream, s, z, labels, members, runs, epoch, max_epochs, slabs, states, stop, history); break;
    }
    return hipGetLastError();
}

hipError_t launch_stop_train_finish(const StopTrainShape &s, const float *z, long n, const int *labels, const int *members,
                                    const StopTrainRun *runs, long n_runs, const double *slabs, const StopTrainState *states, double *params,
                                    double *prob, dsp_stop_train_result *results, hipStream_t stream)
{
    const dim3 grid((unsigned)n_runs), block(kBlock);
    double *sl = const_cast<double *>(slabs);
    switch (padded_units(s.u1)) {
    case 4: hipLaunchKernelGGL(stop_train_finish_kernel<4>, grid, block, 0, stream, s, z, n, labels, members, runs, sl, states, params, prob, results); break;
    case 8: hipLaunchKernelGGL(stop_train_finish_kernel<8>, grid, block, 0, stream, s, z, n, labels, members, runs, sl, states, params, prob, results); break;
    default: hipLaunchKernelGGL(stop_train_finish_kernel<16>, grid, block, 0, stream, s, z, n, labels, members, runs, sl, states, params, prob, results); break;
    }
    return hipGetLastError();
}

}  // namespace dsp
