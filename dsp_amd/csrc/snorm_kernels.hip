// snorm_kernels.hip -- cohort normalisation of speaker scores on the GPU (include/dsp_amd.h dsp_cohort_stats_device,
// dsp_score_normalize_device).
//
//   snorm_stat_vector    a block per cohort vector, its 256 lanes along the vector (element i at src[i * elem_stride]: the rows of a
//                        matrix, or the columns of a matrix narrower than kSnormLanesAcrossColumns).  An exact radix select on the
//                        ordered keys -- four 8-bit digit passes over a 256-bin LDS histogram (integer atomics), the bin of the K'-th
//                        largest found by one wavefront's suffix scan -- then the two float64 tree passes: a wavefront per 64-leaf tile
//                        (a butterfly of __shfl_xor is the adjacent pairwise tree, the add being commutative), the 64 tile sums of a
//                        chunk by the same butterfly, the chunks added in order by one lane.  Vectors of up to kSnormResident values are
//                        read once into LDS; longer ones are read again by every pass
//   snorm_stat_columns   a block per 64 adjacent columns, a lane per column, the four wavefronts taking eight rows at a time in turn:
//                        every load is a 256-byte row segment.  The digit histograms lie [bin][column] in LDS (a wavefront's atomics fall on 64
//                        different banks); each wavefront sums a quarter of a column's bins and the one that holds the K'-th largest
//                        scans its 64.  The tree over the row index with the lanes along columns: a wavefront takes an aligned quarter
//                        (1024 rows) of a chunk, sums 8 rows as a fixed tree and pushes the group sums onto a binary counter of 7
//                        partials held in registers (every index a constant after unrolling), the four quarter sums are paired in LDS
//   snorm_apply_*        z = (x - mean_col) / sigma'_col, t = (x - mean_row) / sigma'_row, out = z, t or 0.5 (z + t): float64, never
//                        fused, rounded once.  Flat for narrow matrices; from kSnormApplyTiled columns on a thread owns a column of a
//                        tile and reads its statistic once, the row's statistic being one broadcast load per row
// No float atomics and no fused multiply-add: a record depends on its vector alone, whatever its place, its axis, the grid and the
// stream.  Every row and column index is checked before a load or a store.
#include <cmath>
#include <mutex>

#include "snorm_kernels.hpp"

#pragma clang fp contract(off)

namespace dsp {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ inline double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ inline int selected_of(int top_k, int n_finite) { return (top_k == 0 || top_k > n_finite) ? n_finite : top_k; }

// the adjacent pairwise tree over the 64 lanes' values, in every lane
__device__ inline double wave_tree(double x)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = x + __shfl_xor(x, d, 64);
    return x;
}

__device__ inline void write_record(dsp_cohort_stat *out, double mean, double sd, float threshold, int n_finite, int n_selected, int n_above)
{
    out->mean = mean;
    out->std = sd;
    out->threshold = threshold;
    out->n_finite = n_finite;
    out->n_selected = n_selected;
    out->n_above = n_above;
}
__device__ inline void write_empty_record(dsp_cohort_stat *out) { write_record(out, quiet_nan(), quiet_nan(), __uint_as_float(0x7fc00000u), 0, 0, 0); }

// mean and std from the tree sums, every product and sum rounded on its own
__device__ inline double mean_of(double A, int e, float theta, int n_selected)
{
    const double copies = (double)e * (double)theta;
    return (A + copies) / (double)n_selected;
}
__device__ inline double std_of(double Q, int e, float theta, double mean, int n_selected)
{
    const double dt = (double)theta - mean, p = dt * dt, copies = (double)e * p;
    return sqrt((Q + copies) / (double)n_selected);
}
// the leaf of v: which = 0 its value, 1 its squared distance from the mean; +0.0 unless v is finite and above the threshold's key
__device__ inline double leaf_of(float v, unsigned theta_key, int which, double mean)
{
    if (!is_finite(v) || !(key_of(v) > theta_key)) return 0.0;
    if (which == 0) return (double)v;
    const double d = (double)v - mean;
    return d * d;
}

// ---- a block per vector ---------------------------------------------------------------------------------------------------------------

template <bool Resident>
__global__ __launch_bounds__(kThreads) void snorm_stat_vector_kernel(const float *__restrict__ cohort, long vectors, long n, long vec_stride, long elem_stride,
                                                                     int top_k, dsp_cohort_stat *__restrict__ stats)
{
    extern __shared__ float lds_values[];                    // Resident: the vector's n values
    __shared__ unsigned hist[256];
    __shared__ unsigned found[4];                            // digit, what is left of K' inside it, the keys above it, n_finite
    __shared__ double tile_sum[64];
    __shared__ double shared_mean;
    const long vec = block_index();
    if (vec >= vectors) return;
    const float *src = cohort + vec * vec_stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (Resident) {
        for (long i = tid; i < n; i += kThreads) lds_values[i] = src[i * elem_stride];
        __syncthreads();
    }
    auto value = [&](long i) { return Resident ? lds_values[i] : src[i * elem_stride]; };

    // the key of the K'-th largest finite value, one digit per pass from the top
    unsigned prefix = 0, want = 0, above = 0;
    int n_finite = 0, n_selected = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (long i = tid; i < n; i += kThreads) {
            const float v = value(i);
            if (!is_finite(v)) continue;
            const unsigned key = key_of(v);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {                                     // lane l holds bins 255 - 4 l ... 252 - 4 l, the largest first
            unsigned c[4], t = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * lane - j]; t += c[j]; }
            unsigned incl = t;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = (unsigned)__shfl_up((int)incl, d, 64);
                if (lane >= d) incl += o;
            }
            const unsigned total = (unsigned)__shfl((int)incl, 63, 64);
            unsigned k = want;
            if (pass == 0) {
                k = (unsigned)selected_of(top_k, (int)total);
                if (lane == 0) found[3] = total;
            }
            unsigned running = incl - t;
            // (no finite value, total == 0 in pass 0: nothing is found, found[0 .. 2] stay unwritten and the block returns below)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (total != 0 && running < k && running + c[j] >= k) {
                    found[0] = (unsigned)(255 - 4 * lane - j);
                    found[1] = k - running;
                    found[2] = running;
                }
                running += c[j];
            }
        }
        __syncthreads();
        if (pass == 0) {
            n_finite = (int)found[3];
            n_selected = selected_of(top_k, n_finite);
            if (n_finite == 0) {                             // (the whole block: found[3] is the same for every thread)
                if (tid == 0) write_empty_record(&stats[vec]);
                return;
            }
        }
        prefix = (prefix << 8) | found[0];
        want = found[1];
        above += found[2];
    }
    const unsigned theta_key = prefix;
    const float theta = float_of(theta_key);
    const int e = (int)want;                                 // the copies of theta that belong to the selection

    double mean = 0.0, sums[2] = {0.0, 0.0};
    for (int which = 0; which < 2; ++which) {
        double total = 0.0;
        for (long c0 = 0; c0 < n; c0 += kSnormChunk) {
            for (int t = wave; t < 64; t += kWaves) {
                const long i0 = c0 + (long)t * 64;
                if (i0 >= n) {                               // a tile of absent leaves
                    if (lane == 0) tile_sum[t] = 0.0;
                    continue;
                }
                const long i = i0 + lane;
                const double x = wave_tree(i < n ? leaf_of(value(i), theta_key, which, mean) : 0.0);
                if (lane == 0) tile_sum[t] = x;
            }
            __syncthreads();
            if (wave == 0) {
                const double y = wave_tree(tile_sum[lane]);
                total = c0 == 0 ? y : total + y;
            }
            __syncthreads();
        }
        sums[which] = total;
        if (which == 0) {
            if (tid == 0) shared_mean = mean_of(total, e, theta, n_selected);
            __syncthreads();
            mean = shared_mean;
        }
    }
    if (tid == 0) write_record(&stats[vec], mean, std_of(sums[1], e, theta, mean, n_selected), theta, n_finite, n_selected, (int)above);
}

// ---- a block per 64 adjacent columns ---------------------------------------------------------------------------------------------------

// the sum of 1024 consecutive rows (an aligned quarter of a chunk) from row r0, a lane per column, over the tree of the row index
__device__ inline double quarter_tree(const float *__restrict__ cohort, long M, long S, long col, bool live, long r0, unsigned theta_key, int which, double mean)
{
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, out = 0.0;
#pragma nounroll
    for (int grp = 0; grp < 128; ++grp) {
        const long r = r0 + (long)grp * 8;
        double x = 0.0;
        if (r < M) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (live && r + j < M) ? cohort[(r + j) * S + col] : 0.0f;
            double l[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) l[j] = (live && r + j < M) ? leaf_of(v[j], theta_key, which, mean) : 0.0;
            x = ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7]));
        }
        bool carry = true;                                   // push the group's sum: a binary counter over the group index
#pragma unroll
        for (int level = 0; level < 7; ++level) {
            if (carry) {
                if ((grp >> level) & 1) x = s[level] + x;
                else { s[level] = x; carry = false; }
            }
        }
        out = x;                                             // (group 127 carries through every level: the quarter's sum)
    }
    return out;
}

__global__ __launch_bounds__(kThreads) void snorm_stat_columns_kernel(const float *__restrict__ cohort, long M, long S, long tiles, int top_k,
                                                                      dsp_cohort_stat *__restrict__ stats)
{
    extern __shared__ unsigned hist[];                       // [256 bins][64 columns]
    __shared__ unsigned quarter[kWaves][kSnormTileColumns];
    __shared__ unsigned col_prefix[kSnormTileColumns], col_want[kSnormTileColumns], col_above[kSnormTileColumns], col_finite[kSnormTileColumns];
    __shared__ double part[kWaves][kSnormTileColumns];
    __shared__ double col_mean[kSnormTileColumns];
    const long tile = block_index();
    if (tile >= tiles) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long col = tile * kSnormTileColumns + lane;
    const bool live = col < S;
    if (wave == 0) col_prefix[lane] = col_want[lane] = col_above[lane] = col_finite[lane] = 0;

    // Registers: 255 VGPRs, no scratch, one wavefront per SIMD (a block per CU, which the 68.5 KiB of LDS nearly asks for anyway).
    // That is the whole budget of __launch_bounds__(256): asking for two wavefronts per SIMD (__launch_bounds__(256, 2)) spills 2
    // VGPRs to 12 bytes of scratch, and keeping the pass loops rolled (below) changes nothing.  If a compiler update tips this
    // kernel into scratch, shrink the eight-row batches of the digit pass and of quarter_tree to four before anything else.
#pragma nounroll
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 256 * kSnormTileColumns; i += kThreads) hist[i] = 0;
        __syncthreads();
        const unsigned prefix = col_prefix[lane], want_in = col_want[lane];
        if (live) {                                          // eight rows per step: eight loads in flight (the counts do not depend on the order)
            for (long r0 = (long)wave * 8; r0 < M; r0 += kWaves * 8) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = r0 + j < M ? cohort[(r0 + j) * S + col] : __uint_as_float(0x7fc00000u);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (!is_finite(v[j])) continue;
                    const unsigned key = key_of(v[j]);
                    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * kSnormTileColumns + lane], 1u);
                }
            }
        }
        __syncthreads();
        unsigned q = 0;                                      // wavefront w: bins 255 - 64 w ... 192 - 64 w of every column
        for (int j = 0; j < 64; ++j) q += hist[(255 - 64 * wave - j) * kSnormTileColumns + lane];
        quarter[wave][lane] = q;
        __syncthreads();
        unsigned total = 0, running = 0, k = want_in;
        for (int w = 0; w < kWaves; ++w) total += quarter[w][lane];
        if (pass == 0) k = (unsigned)selected_of(top_k, (int)total);
        int target = -1;
        unsigned base = 0;
        for (int w = 0; w < kWaves; ++w) {
            const unsigned c = quarter[w][lane];
            if (total != 0 && running < k && running + c >= k) { target = w; base = running; }
            running += c;
        }
        if (pass == 0 && wave == 0) col_finite[lane] = total;
        if (target == wave) {                                // one thread per column with a finite value
            running = base;
            unsigned digit = 0, left = 0, over = 0;
            for (int j = 0; j < 64; ++j) {
                const unsigned c = hist[(255 - 64 * wave - j) * kSnormTileColumns + lane];
                if (running < k && running + c >= k) { digit = (unsigned)(255 - 64 * wave - j); left = k - running; over = running; }
                running += c;
            }
            col_prefix[lane] = (prefix << 8) | digit;
            col_want[lane] = left;
            col_above[lane] += over;
        }
        __syncthreads();
    }
    const unsigned theta_key = col_prefix[lane];
    const float theta = float_of(theta_key);
    const int e = (int)col_want[lane], n_above = (int)col_above[lane], n_finite = (int)col_finite[lane];
    const int n_selected = selected_of(top_k, n_finite);
    const bool counted = live && n_finite > 0;

    double mean = 0.0, sums[2] = {0.0, 0.0};
#pragma nounroll
    for (int which = 0; which < 2; ++which) {
        double total = 0.0;
        for (long c0 = 0; c0 < M; c0 += kSnormChunk) {
            const long r0 = c0 + (long)wave * (kSnormChunk / kWaves);
            part[wave][lane] = r0 < M ? quarter_tree(cohort, M, S, col, counted, r0, theta_key, which, mean) : 0.0;
            __syncthreads();
            if (wave == 0) {
                const double y = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
                total = c0 == 0 ? y : total + y;
            }
            __syncthreads();
        }
        sums[which] = total;
        if (which == 0) {
            if (wave == 0) col_mean[lane] = counted ? mean_of(total, e, theta, n_selected) : 0.0;
            __syncthreads();
            mean = col_mean[lane];
        }
    }
    if (wave == 0 && live) {
        if (n_finite == 0) write_empty_record(&stats[col]);
        else write_record(&stats[col], mean, std_of(sums[1], e, theta, mean, n_selected), theta, n_finite, n_selected, n_above);
    }
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------------

struct Side { double mean, sigma; };
__device__ inline Side side_of(const dsp_cohort_stat *s, double std_floor)
{
    Side out;
    out.mean = s->n_finite > 0 ? s->mean : quiet_nan();
    const double sd = s->std;
    out.sigma = sd > std_floor ? sd : std_floor;
    return out;
}
__device__ inline float normalised(float score, int mode, Side row, Side col)
{
    const double x = (double)score;
    double z = 0.0, t = 0.0;
    if (mode != DSP_NORM_T) { const double d = x - col.mean; z = d / col.sigma; }
    if (mode != DSP_NORM_Z) { const double d = x - row.mean; t = d / row.sigma; }
    if (mode == DSP_NORM_Z) return (float)z;
    if (mode == DSP_NORM_T) return (float)t;
    const double both = z + t;
    return (float)(0.5 * both);
}

// narrow matrices: a thread per trial of the flat matrix; scores and out may be the same buffer (a thread reads a trial, then writes it)
__global__ __launch_bounds__(kThreads) void snorm_apply_flat_kernel(const float *scores, long total, long S, const dsp_cohort_stat *__restrict__ row_stats,
                                                                    const dsp_cohort_stat *__restrict__ col_stats, int mode, double std_floor, float *out)
{
    const long i = block_index() * kThreads + threadIdx.x;
    if (i >= total) return;
    const long r = i / S, c = i - r * S;
    Side row{0.0, 1.0}, col{0.0, 1.0};
    if (mode != DSP_NORM_Z) row = side_of(&row_stats[r], std_floor);
    if (mode != DSP_NORM_T) col = side_of(&col_stats[c], std_floor);
    out[i] = normalised(scores[i], mode, row, col);
}

// a block per kSnormApplyRows rows of 256 adjacent columns: a thread owns a column and reads its statistic once
__global__ __launch_bounds__(kThreads) void snorm_apply_tiled_kernel(const float *scores, long T, long S, long col_tiles, long blocks,
                                                                     const dsp_cohort_stat *__restrict__ row_stats, const dsp_cohort_stat *__restrict__ col_stats, int mode,
                                                                     double std_floor, float *out)
{
    const long b = block_index();
    if (b >= blocks) return;
    const long group = b / col_tiles, c = (b - group * col_tiles) * kThreads + threadIdx.x;
    if (c >= S) return;
    Side row{0.0, 1.0}, col{0.0, 1.0};
    if (mode != DSP_NORM_T) col = side_of(&col_stats[c], std_floor);
    const long r0 = group * kSnormApplyRows, r1 = r0 + kSnormApplyRows < T ? r0 + kSnormApplyRows : T;
    for (long r = r0; r < r1; ++r) {
        if (mode != DSP_NORM_Z) row = side_of(&row_stats[r], std_floor);
        out[r * S + c] = normalised(scores[r * S + c], mode, row, col);
    }
}

// Both statistics kernels may ask for more dynamic LDS than a kernel gets by default (64 KiB): the resident vector form up to 128 KiB,
// the column form 64 KiB beside 4.5 KiB of static arrays.  The limits are constants, raised once per device (the current one).
hipError_t raise_lds_limits()
{
    static std::mutex mu;
    static bool raised[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    if (raised[dev]) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(snorm_stat_columns_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSnormTileLds);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(snorm_stat_vector_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                kSnormResident * (int)sizeof(float));
    raised[dev] = e == hipSuccess;
    return e;
}

}  // namespace

hipError_t launch_cohort_stats(const float *cohort, long n_rows, long n_cols, int axis, int top_k, dsp_cohort_stat *stats, hipStream_t st)
{
    const bool per_row = axis == DSP_COHORT_PER_ROW;
    const long vectors = per_row ? n_rows : n_cols, n = per_row ? n_cols : n_rows;
    if (vectors < 1 || vectors > kSnormMaxVectors || n < 1 || n > kSnormMaxLength) return hipErrorInvalidValue;
    if (const hipError_t e = raise_lds_limits()) return e;
    if (!per_row && n_cols >= kSnormLanesAcrossColumns) {
        const long tiles = ceil_div(n_cols, kSnormTileColumns);
        snorm_stat_columns_kernel<<<grid_for(tiles), kThreads, kSnormTileLds, st>>>(cohort, n_rows, n_cols, tiles, top_k, stats);
        return hipGetLastError();
    }
    const long vec_stride = per_row ? n_cols : 1, elem_stride = per_row ? 1 : n_cols;
    if (n <= kSnormResident) {
        const size_t lds = (size_t)n * sizeof(float);
        snorm_stat_vector_kernel<true><<<grid_for(vectors), kThreads, lds, st>>>(cohort, vectors, n, vec_stride, elem_stride, top_k, stats);
    } else {
        snorm_stat_vector_kernel<false><<<grid_for(vectors), kThreads, 0, st>>>(cohort, vectors, n, vec_stride, elem_stride, top_k, stats);
    }
    return hipGetLastError();
}

hipError_t launch_score_normalize(const float *scores, long n_rows, long n_cols, const dsp_cohort_stat *row_stats, const dsp_cohort_stat *col_stats, int mode,
                                  double std_floor, float *out, hipStream_t st)
{
    if (n_rows < 1 || n_cols < 1 || n_rows > kSnormMaxVectors || n_cols > kSnormMaxVectors) return hipErrorInvalidValue;
    if (n_cols < kSnormApplyTiled) {
        const long total = n_rows * n_cols;
        snorm_apply_flat_kernel<<<grid_for(ceil_div(total, kThreads)), kThreads, 0, st>>>(scores, total, n_cols, row_stats, col_stats, mode, std_floor, out);
    } else {
        const long col_tiles = ceil_div(n_cols, kThreads), blocks = col_tiles * ceil_div(n_rows, kSnormApplyRows);
        snorm_apply_tiled_kernel<<<grid_for(blocks), kThreads, 0, st>>>(scores, n_rows, n_cols, col_tiles, blocks, row_stats, col_stats, mode, std_floor, out);
    }
    return hipGetLastError();
}

}  // namespace dsp
