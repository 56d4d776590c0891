// calibrate_kernels.hip -- score calibration on the GPU (include/dsp_amd.h dsp_calibration_*).
//
//   cal_init        one thread: the state of a fit -- theta = init, nothing pending, the report cleared
//   cal_stat_*      the statistics pass at the state's theta: per trial one float64 exp and one log1p give softplus, the sigmoid and
//                   sigma (1 - sigma); per class the sums of the objective, of the gradient over phi = (x, 1, l) and of the Hessian's
//                   upper triangle, float64, and the class counts as integers.  Below kTrialLanesAcrossColumns columns a wavefront
//                   folds kCalRowsTime rows of one column, a lane every 64th row in ascending order; from there on a lane owns a
//                   column, a wavefront folds kCalRowsColumns rows and a block's four wavefronts add in wave order.  Lanes combine by
//                   a butterfly of fixed order.  One partial per wavefront or block, written with plain stores
//   cal_reduce      a level of the tree: node i adds partials [i kCalFanIn, (i + 1) kCalFanIn) in ascending order
//   cal_solve       one block adds the last kCalFanIn partials at most, weights the classes by prior / P and (1 - prior) / N, and one
//                   thread moves the state machine: reject and halve, accept and stop, or accept and solve H d = g by Cholesky
//   cal_apply       out = (float)(A x + B + C l), float64, unfused
// The tree depends on (T, S) alone and there are no float atomics: a fit is the same bits whatever the stream or the workspace.
// theta arrives through the state and tau as an argument: both are uniform, the compiler loads them through the scalar cache.
// Every kernel of a fit tests CalState::done first, so max_iter passes are enqueued without a host round trip and those behind the end
// leave at once.  Every row and column index is checked before a load.
#include <cmath>

#include "calibrate_kernels.hpp"

namespace dsp {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kApplyPerThread = 16;

struct Theta { double a, b, c, tau; };

// a lane's share of a partial
struct Fold {
    double sum[2 * kCalSums];
    unsigned n[kCalCounts];                                  // (a wavefront's share: far below 2^32)
    __device__ Fold()
    {
#pragma unroll
        for (int i = 0; i < 2 * kCalSums; ++i) sum[i] = 0.0;
#pragma unroll
        for (int i = 0; i < kCalCounts; ++i) n[i] = 0;
    }
    template <bool L> __device__ void take(float score, bool target, double l, const Theta &t)
    {
        const double x = (double)score;
        if (!is_finite(x)) { ++n[2]; return; }
        double c = t.a * x + t.b;
        if (L) c += t.c * l;
        const double z = c + t.tau, u = target ? -z : z;     // the trial's loss is softplus(u)
        const double e = exp(-fabs(u)), inv = 1.0 / (1.0 + e);
        const double big = inv, small = e * inv;             // sigma(|u|), sigma(-|u|)
        const double loss = fmax(u, 0.0) + log1p(e);
        const double sig = u >= 0.0 ? big : small;           // sigma(u) = d loss / d u
        const double dl = target ? -sig : sig;               // d loss / d c
        const double w = big * small;                        // sigma (1 - sigma) = d^2 loss / d c^2
        const double v[kCalSums] = {loss, dl * x, dl, L ? dl * l : 0.0, w * x * x, w * x, L ? w * x * l : 0.0, w, L ? w * l : 0.0, L ? w * l * l : 0.0};
#pragma unroll
        for (int i = 0; i < kCalSums; ++i) {
            sum[i] += target ? v[i] : 0.0;
            sum[kCalSums + i] += target ? 0.0 : v[i];
        }
        n[0] += target ? 1u : 0u;
        n[1] += target ? 0u : 1u;
    }
    __device__ void across_wave()
    {
        for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
            for (int i = 0; i < 2 * kCalSums; ++i) sum[i] += __shfl_xor(sum[i], d, 64);
#pragma unroll
            for (int i = 0; i < kCalCounts; ++i) n[i] += (unsigned)__shfl_xor((int)n[i], d, 64);
        }
    }
};

__device__ inline Theta theta_of(const CalState *__restrict__ state, double tau) { return Theta{state->theta[0], state->theta[1], state->theta[2], tau}; }

__global__ void cal_init_kernel(CalState *__restrict__ state, dsp_calibration init)
{
    const double p[3] = {init.a, init.b, init.c};
    for (int i = 0; i < 3; ++i) {
        state->theta[i] = state->base[i] = p[i];
        state->step[i] = 0.0;
    }
    state->objective_base = NAN;
    state->halvings = state->pending = state->done = state->reserved = 0;
    dsp_calibration_report &rep = state->report;
    rep.params = init;
    rep.n_target = rep.n_nontarget = rep.n_excluded = 0;
    rep.objective_start = rep.objective = rep.last_step = NAN;
    rep.n_iter = rep.n_rejected = rep.reserved = 0;
    rep.status = DSP_CAL_MAX_ITER;
}

// a wavefront per (chunk of kCalRowsTime rows, column): unit = chunk S + column
template <bool L>
__global__ __launch_bounds__(kThreads) void cal_stat_time_kernel(const float *__restrict__ scores, const int *__restrict__ truth, const double *__restrict__ duration,
                                                                 long T, long S, long units, const CalState *__restrict__ state, double tau,
                                                                 CalPartial *__restrict__ out)
{
    if (state->done) return;
    const long unit = block_index() * kWaves + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (unit >= units) return;
    const Theta t = theta_of(state, tau);
    const long chunk = unit / S, s = unit % S;
    const long r0 = chunk * kCalRowsTime, r1 = min(T, r0 + kCalRowsTime);
    Fold f;
    for (long r = r0 + lane; r < r1; r += 64) f.take<L>(scores[r * S + s], truth[r] == (int)s, L ? duration[r] : 0.0, t);
    f.across_wave();
    if (lane == 0) {
        CalPartial &p = out[unit];
#pragma unroll
        for (int i = 0; i < 2 * kCalSums; ++i) p.sum[i] = f.sum[i];
#pragma unroll
        for (int i = 0; i < kCalCounts; ++i) p.n[i] = (long)f.n[i];
    }
}

// a block per (kCalBlockRowsColumns rows, group of 64 columns): unit = chunk groups + group; a lane per column, a wavefront per
// kCalRowsColumns rows
template <bool L>
__global__ __launch_bounds__(kThreads) void cal_stat_columns_kernel(const float *__restrict__ scores, const int *__restrict__ truth, const double *__restrict__ duration,
                                                                    long T, long S, long groups, long units, const CalState *__restrict__ state, double tau,
                                                                    CalPartial *__restrict__ out)
{
    __shared__ double part_sum[kWaves][2 * kCalSums];
    __shared__ long part_n[kWaves][kCalCounts];
    if (state->done) return;
    const long unit = block_index();
    if (unit >= units) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const Theta t = theta_of(state, tau);
    const long chunk = unit / groups, s = (unit % groups) * 64 + lane;
    const long r0 = chunk * kCalBlockRowsColumns + (long)wave * kCalRowsColumns, r1 = min(T, r0 + kCalRowsColumns);
    Fold f;
    if (s < S)
        for (long r = r0; r < r1; ++r) f.take<L>(scores[r * S + s], truth[r] == (int)s, L ? duration[r] : 0.0, t);
    f.across_wave();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 2 * kCalSums; ++i) part_sum[wave][i] = f.sum[i];
#pragma unroll
        for (int i = 0; i < kCalCounts; ++i) part_n[wave][i] = (long)f.n[i];
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < 2 * kCalSums) {
        double acc = 0.0;
        for (int w = 0; w < kWaves; ++w) acc += part_sum[w][i];          // ascending wave
        out[unit].sum[i] = acc;
    } else if (i < kCalWords) {
        long acc = 0;
        for (int w = 0; w < kWaves; ++w) acc += part_n[w][i - 2 * kCalSums];
        out[unit].n[i - 2 * kCalSums] = acc;
    }
}

// word `word` of partials [first, last) added in ascending order
__device__ inline void add_partials(const CalPartial *__restrict__ in, long first, long last, int word, CalPartial *out)
{
    if (word < 2 * kCalSums) {
        double acc = 0.0;
        for (long c = first; c < last; ++c) acc += in[c].sum[word];
        out->sum[word] = acc;
    } else {
        long acc = 0;
        for (long c = first; c < last; ++c) acc += in[c].n[word - 2 * kCalSums];
        out->n[word - 2 * kCalSums] = acc;
    }
}

// a thread per (node, word)
__global__ __launch_bounds__(kThreads) void cal_reduce_kernel(const CalPartial *__restrict__ in, long n_in, long n_out, const CalState *__restrict__ state,
                                                              CalPartial *__restrict__ out)
{
    if (state->done) return;
    const long at = block_index() * kThreads + threadIdx.x, node = at / kCalWords;
    if (node >= n_out) return;
    const long first = node * kCalFanIn;
    add_partials(in, first, min(n_in, first + kCalFanIn), (int)(at % kCalWords), out + node);
}

// H d = g by Cholesky, H's upper triangle as xx x1 xl 11 1l ll, n = 2: without l.  false: a pivot that is not above 0, or a d that is
// not finite
__device__ bool cal_cholesky(int n, const double *H, const double *g, double *d)
{
#pragma clang fp contract(off)
    if (!(H[0] > 0.0)) return false;
    const double l00 = sqrt(H[0]), l10 = H[1] / l00, p1 = H[3] - l10 * l10;
    if (!(p1 > 0.0)) return false;
    const double l11 = sqrt(p1), y0 = g[0] / l00, y1 = (g[1] - l10 * y0) / l11;
    if (n == 2) {
        d[2] = 0.0;
        d[1] = y1 / l11;
        d[0] = (y0 - l10 * d[1]) / l00;
    } else {
        const double l20 = H[2] / l00, l21 = (H[4] - l20 * l10) / l11, p2 = H[5] - l20 * l20 - l21 * l21;
        if (!(p2 > 0.0)) return false;
        const double l22 = sqrt(p2), y2 = (g[2] - l20 * y0 - l21 * y1) / l22;
        d[2] = y2 / l22;
        d[1] = (y1 - l21 * d[2]) / l11;
        d[0] = (y0 - l10 * d[1] - l20 * d[2]) / l00;
    }
    return is_finite(d[0]) && is_finite(d[1]) && is_finite(d[2]);
}

__device__ void cal_finish(CalState *st, int status, const double *theta, double objective)
{
    st->report.params = dsp_calibration{theta[0], theta[1], theta[2]};
    st->report.objective = objective;
    st->report.status = status;
    st->done = 1;
}

// the state machine of include/dsp_amd.h, after pass `iter` whose sums are `tot`
__device__ void cal_advance(const CalPartial &tot, int iter, int max_iter, int n_par, double prior, double tol, dsp_calibration init, CalState *st)
{
#pragma clang fp contract(off)
    dsp_calibration_report &rep = st->report;
    const long P = tot.n[0], N = tot.n[1];
    rep.n_target = P;
    rep.n_nontarget = N;
    rep.n_excluded = tot.n[2];
    rep.n_iter = iter + 1;
    if (P == 0 || N == 0) {
        const double p[3] = {init.a, init.b, init.c};
        cal_finish(st, DSP_CAL_NO_CLASS, p, NAN);
        return;
    }
    const double wp = prior / (double)P, wn = (1.0 - prior) / (double)N;
    const double J = wp * tot.sum[0] + wn * tot.sum[kCalSums];
    double g[3], H[6];
    for (int i = 0; i < 3; ++i) g[i] = wp * tot.sum[1 + i] + wn * tot.sum[kCalSums + 1 + i];
    for (int i = 0; i < 6; ++i) H[i] = wp * tot.sum[4 + i] + wn * tot.sum[kCalSums + 4 + i];
    if (iter == 0) rep.objective_start = J;
    const bool last = iter == max_iter - 1;
    if (st->pending && !(J <= st->objective_base)) {         // rejected: half the step again
        ++rep.n_rejected;
        if (++st->halvings > kCalMaxHalvings) { cal_finish(st, DSP_CAL_STALLED, st->base, st->objective_base); return; }
        const double scale = 1.0 / (double)(1L << st->halvings);
        for (int i = 0; i < 3; ++i) st->theta[i] = st->base[i] - st->step[i] * scale;
        if (last) cal_finish(st, DSP_CAL_MAX_ITER, st->base, st->objective_base);
        return;
    }
    if (st->pending) {
        double moved = 0.0;
        for (int i = 0; i < n_par; ++i) moved = fmax(moved, fabs(st->theta[i] - st->base[i]));
        rep.last_step = moved;
        if (moved <= tol) { cal_finish(st, DSP_CAL_CONVERGED, st->theta, J); return; }
    }
    for (int i = 0; i < 3; ++i) st->base[i] = st->theta[i];
    st->objective_base = J;
    st->halvings = 0;
    bool ok = is_finite(J);
    for (int i = 0; i < 3; ++i) ok = ok && is_finite(g[i]);
    for (int i = 0; i < 6; ++i) ok = ok && is_finite(H[i]);
    double d[3];
    if (!ok || !cal_cholesky(n_par, H, g, d)) { cal_finish(st, DSP_CAL_SINGULAR, st->base, J); return; }
    for (int i = 0; i < 3; ++i) {
        st->step[i] = d[i];
        st->theta[i] = st->base[i] - d[i];
    }
    st->pending = 1;
    if (last) cal_finish(st, DSP_CAL_MAX_ITER, st->base, J);
}

__global__ __launch_bounds__(64) void cal_solve_kernel(const CalPartial *__restrict__ top, int n_top, int iter, int max_iter, int n_par, double prior, double tol,
                                                       dsp_calibration init, CalState *state)
{
    __shared__ CalPartial tot;
    if (state->done) return;
    if ((int)threadIdx.x < kCalWords) add_partials(top, 0, n_top, (int)threadIdx.x, &tot);
    __syncthreads();
    if (threadIdx.x == 0) cal_advance(tot, iter, max_iter, n_par, prior, tol, init, state);
}

// a block per kThreads kApplyPerThread consecutive trials; scores and out may be the same buffer (a thread reads a trial, then writes it)
template <bool L>
__global__ __launch_bounds__(kThreads) void cal_apply_kernel(const float *scores, const double *__restrict__ duration, long total, long S, long blocks,
                                                             dsp_calibration p, float *out)
{
#pragma clang fp contract(off)
    const long b = block_index();
    if (b >= blocks) return;
    long i = b * (kThreads * kApplyPerThread) + threadIdx.x;
    long r = L ? i / S : 0, c = L ? i - r * S : 0;           // the trial's row and column, kept by steps of kThreads trials
    const long step_r = kThreads / S, step_c = kThreads % S;
    for (int k = 0; k < kApplyPerThread && i < total; ++k) {
        const double scaled = p.a * (double)scores[i];
        double v = scaled + p.b;
        if (L) {
            const double term = p.c * duration[r];           // (i < total: r < T)
            v = v + term;
        }
        out[i] = (float)v;
        i += kThreads;
        if (L) {
            r += step_r;
            c += step_c;
            if (c >= S) { c -= S; ++r; }
        }
    }
}

}  // namespace

hipError_t launch_calibration_fit(const CalFit &q, hipStream_t st)
{
    const long T = q.rows, S = q.columns, units = cal_units(T, S), groups = ceil_div(S, 64);
    if (T < 1 || S < 1 || units > (1L << 36)) return hipErrorInvalidValue;
    const bool across = S >= kTrialLanesAcrossColumns, with_l = q.duration != nullptr;
    const double tau = std::log(q.prior / (1.0 - q.prior));
    cal_init_kernel<<<1, 1, 0, st>>>(q.state, q.init);
    for (int it = 0; it < q.max_iter; ++it) {
        if (across) {
            auto kernel = with_l ? cal_stat_columns_kernel<true> : cal_stat_columns_kernel<false>;
            kernel<<<grid_for(units), kThreads, 0, st>>>(q.scores, q.truth, q.duration, T, S, groups, units, q.state, tau, q.partials);
        } else {
            auto kernel = with_l ? cal_stat_time_kernel<true> : cal_stat_time_kernel<false>;
            kernel<<<grid_for(ceil_div(units, kWaves)), kThreads, 0, st>>>(q.scores, q.truth, q.duration, T, S, units, q.state, tau, q.partials);
        }
        CalPartial *level = q.partials;
        long n = units;
        while (n > kCalFanIn) {
            const long m = ceil_div(n, kCalFanIn);
            cal_reduce_kernel<<<grid_for(ceil_div(m * kCalWords, kThreads)), kThreads, 0, st>>>(level, n, m, q.state, level + n);
            level += n;
            n = m;
        }
        cal_solve_kernel<<<1, 64, 0, st>>>(level, (int)n, it, q.max_iter, with_l ? 3 : 2, q.prior, q.tol, q.init, q.state);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_calibration_apply(const float *scores, const double *duration, long rows, long columns, dsp_calibration params, float *out, hipStream_t st)
{
    const long total = rows * columns, blocks = ceil_div(total, (long)kThreads * kApplyPerThread);
    if (rows < 1 || columns < 1) return hipErrorInvalidValue;
    if (duration) cal_apply_kernel<true><<<grid_for(blocks), kThreads, 0, st>>>(scores, duration, total, columns, blocks, params, out);
    else cal_apply_kernel<false><<<grid_for(blocks), kThreads, 0, st>>>(scores, duration, total, columns, blocks, params, out);
    return hipGetLastError();
}

}  // namespace dsp
