// vad_kernels.hip -- voice activity detection on ragged batches for gfx950 (include/dsp_amd.h dsp_vad_*, dsp_rows_*).
//
//   vad_power_kernel     the audio, once: float64 sums of squares per sub-block of g samples into LDS, a frame's m of them added
//                        in ascending order, / frame_length -> d_power
//   vad_stats_kernel     per tile of 256 rows: the largest finite power into the clip's key by an integer atomicMax, the tile's sum
//                        over the 256-leaf halving tree and its finite count (DSP_VAD_REF_MAX and _MEAN only)
//   vad_level_kernel     per clip: reference and threshold
//   vad_decide_kernel    per tile, with the raw flags of context + pad rows on either side computed again: smoothing, hangover,
//                        flags, levels, the tile's record
//   vad_clip_kernel      per clip: its record and kept count from its tiles' records
//   rows_count_kernel    kept rows per clip from any flags
//   rows_tile_count / rows_scan / rows_copy   the selection: a stable compaction of the matrix's rows
//
// Nothing is added with float atomics and every tree is fixed by g, by 256 or by a clip's row count alone, so an output is the same
// bits whatever the batch, the clip's position in it, the grid, the stream and the workspace's previous contents.
#include <hip/hip_runtime.h>

#include "stream_load.hpp"
#include "vad_kernels.hpp"

namespace dsp {
namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kBlock = kVadTileRows;
constexpr int kWaves = kBlock / 64;
constexpr int kUnroll = 4;               // slots a lane group takes at a time in the power kernel
constexpr long kMaxGrid = 2048;          // 256 CUs x 8 blocks: the rest of the tiles by the grid's stride

// the clip of a tile: the last c with to[c] <= tile (a clip without tiles shares its offset with the next one and is passed over)
// (span_find.hpp's owner_of finds the same clip; this form stays because joining it changes the kernels' instructions, which nobody has timed)
__device__ inline long clip_of_tile(const long *to, long n_clips, long tile)
{
    long lo = 0, hi = n_clips - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (to[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a double as an ordered key: an unsigned that grows with the double; 0 is below every key
__device__ inline unsigned long long key_of(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double double_of(unsigned long long key)
{
    return __longlong_as_double((long long)((key >> 63) ? (key & 0x7fffffffffffffffull) : ~key));
}

__device__ inline double square(float x) { return (double)x * (double)x; }      // exact: 48 significant bits at most

__global__ __launch_bounds__(kBlock) void vad_power_kernel(const float *__restrict__ sig, const long *__restrict__ so, const long *__restrict__ fo,
                                                           const long *__restrict__ to, long n_clips, long n_tiles, VadGeometry geo, int frame_length,
                                                           int hop, double *__restrict__ power)
{
    __shared__ double sums[kVadSlots];
    const int g = geo.g, m = geo.m, s = geo.stride, W = geo.lanes, per_hop = hop / g;
    const int group = threadIdx.x / W, lane = threadIdx.x % W, n_groups = kBlock / W;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long c = clip_of_tile(to, n_clips, tile);
        const long n = so[c + 1] - so[c], T = fo[c + 1] - fo[c];
        const long t0 = (tile - to[c]) * kBlock;
        const int rows = (int)min((long)kBlock, T - t0);
        const float *x = sig + so[c];
        const long nb = (n + g - 1) / g;
        // 16-byte loads where every quad of every sub-block starts on a 16-byte boundary; a quad the clip's end cuts is loaded by dwords,
        // in the same order: the tree is one
        const bool vec = (g & 3) == 0 && (reinterpret_cast<size_t>(x) & 15) == 0;
        for (int r0 = 0; r0 < rows; r0 += geo.chunk_rows) {
            const int rc = min(geo.chunk_rows, rows - r0);
            const int slots = (rc - 1) * s + m;
            // slot k is sub-block b_first + k where the frames overlap or touch (stride = hop / g); where they do not, the m of row k / m
            const long b_first = ((t0 + r0) * hop - geo.lead) / g;              // (an exact division: every term is a multiple of g)
            for (int k0 = 0; k0 < slots; k0 += kUnroll * n_groups) {
                // the first quad of kUnroll slots is loaded before any is added, so that as many loads are in flight
                long base[kUnroll];
                int len[kUnroll];                                               // samples of the sub-block inside the clip, 0: none
                bool whole[kUnroll];
                f4v head[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int k = k0 + u * n_groups + group;
                    base[u] = 0;
                    len[u] = 0;
                    if (k < slots) {
                        long b = b_first + k;
                        if (s != per_hop) {
                            const int r = k / m;
                            b = b_first + (long)r * per_hop + (k - r * m);
                        }
                        if (b >= 0 && b < nb) {
                            base[u] = b * g;
                            len[u] = (int)min((long)g, n - base[u]);
                        }
                    }
                    whole[u] = vec && 4 * lane + 4 <= len[u];
                    if (whole[u]) head[u] = load_stream(reinterpret_cast<const f4v *>(x + base[u] + 4 * lane));
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int k = k0 + u * n_groups + group;
                    double acc = 0.0;
                    int e = 4 * lane;
                    if (whole[u]) {
                        acc += square(head[u].x);
                        acc += square(head[u].y);
                        acc += square(head[u].z);
                        acc += square(head[u].w);
                        e += 4 * W;
                    }
                    for (; e < len[u]; e += 4 * W) {
                        if (vec && e + 4 <= len[u]) {
                            const f4v v = load_stream(reinterpret_cast<const f4v *>(x + base[u] + e));
                            acc += square(v.x);
                            acc += square(v.y);
                            acc += square(v.z);
                            acc += square(v.w);
                        } else {
                            const int left = min(4, len[u] - e);
                            for (int i = 0; i < left; ++i) acc += square(load_stream(x + base[u] + e + i));
                        }
                    }
                    for (int off = W >> 1; off >= 1; off >>= 1) acc += __shfl_down(acc, off, W);
                    if (k < slots && lane == 0) sums[k] = acc;
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < rc) {
                const int r = threadIdx.x;
                double a = 0.0;
                for (int j = 0; j < m; ++j) a += sums[r * s + j];
                power[fo[c] + t0 + r0 + r] = a / (double)frame_length;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kBlock) void vad_stats_kernel(const double *__restrict__ power, const long *__restrict__ fo, const long *__restrict__ to,
                                                           long n_clips, long n_tiles, unsigned long long *__restrict__ ref_key, VadTile *__restrict__ tiles)
{
    __shared__ double leaf[kBlock];
    __shared__ int finite_of_wave[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long c = clip_of_tile(to, n_clips, tile);
        const long T = fo[c + 1] - fo[c], t = (tile - to[c]) * kBlock + threadIdx.x;
        double p = 0.0;
        bool fin = false;
        if (t < T) {
            p = power[fo[c] + t];
            fin = is_finite(p);
        }
        unsigned long long key = fin ? key_of(p) : 0ull;
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long other = __shfl_down(key, off, 64);
            key = key > other ? key : other;
        }
        if (lane == 0 && key) atomicMax(&ref_key[c], key);
        const unsigned long long mask = __ballot(fin);
        if (lane == 0) finite_of_wave[wave] = __popcll(mask);
        leaf[threadIdx.x] = fin ? p : 0.0;
        __syncthreads();
        for (int off = kBlock >> 1; off >= 1; off >>= 1) {
            if ((int)threadIdx.x < off) leaf[threadIdx.x] += leaf[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            int nf = 0;
            for (int w = 0; w < kWaves; ++w) nf += finite_of_wave[w];
            tiles[tile].sum = leaf[0];
            tiles[tile].n_finite = nf;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void vad_level_kernel(const long *__restrict__ to, long n_clips, const unsigned long long *__restrict__ ref_key,
                                                           const VadTile *__restrict__ tiles, VadDecision dec, double *__restrict__ level)
{
    const long c = block_index() * kBlock + threadIdx.x;
    if (c >= n_clips) return;
    double ref = 1.0;
    if (dec.reference == DSP_VAD_REF_MAX) {
        ref = ref_key[c] ? double_of(ref_key[c]) : 0.0;
    } else if (dec.reference == DSP_VAD_REF_MEAN) {
        double sum = 0.0;
        long nf = 0;
        for (long tile = to[c]; tile < to[c + 1]; ++tile) {
            sum += tiles[tile].sum;
            nf += tiles[tile].n_finite;
        }
        ref = nf ? sum / (double)nf : 0.0;
    }
    const double scaled = ref * dec.ratio;
    level[2 * c] = ref;
    level[2 * c + 1] = scaled >= dec.floor ? scaled : dec.floor;
}

// flags among entries [0, 512) of a tile's image, as 8 ballot words and their running counts
struct FlagImage {
    unsigned long long word[9];
    int before[9];
    // flags in entries [a, b]
    __device__ int count(int a, int b) const { return upto(b + 1) - upto(a); }
    __device__ int upto(int i) const { return before[i >> 6] + __popcll(word[i >> 6] & ((1ull << (i & 63)) - 1ull)); }
    __device__ void scan()
    {
        int run = 0;
        for (int w = 0; w < 8; ++w) {
            before[w] = run;
            run += __popcll(word[w]);
        }
        before[8] = run;
        word[8] = 0ull;
    }
};

__global__ __launch_bounds__(kBlock) void vad_decide_kernel(const double *__restrict__ power, const long *__restrict__ fo, const long *__restrict__ to,
                                                            long n_clips, long n_tiles, const double *__restrict__ level, VadDecision dec,
                                                            unsigned char *__restrict__ flags, float *__restrict__ level_db, VadTile *__restrict__ tiles)
{
    __shared__ FlagImage raw, smooth;
    __shared__ unsigned long long kept_word[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ctx = dec.context, pad = dec.pad, halo = ctx + pad, span = kBlock + 2 * halo;       // span <= 512
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long c = clip_of_tile(to, n_clips, tile);
        const long T = fo[c + 1] - fo[c], t0 = (tile - to[c]) * kBlock;
        const double thr = level[2 * c + 1];
        const long first_row = t0 - halo;                  // the row of entry 0
        for (int pass = 0; pass < 2; ++pass) {
            const int i = pass * kBlock + threadIdx.x;
            const long t = first_row + i;
            bool on = false;
            if (i < span && t >= 0 && t < T) {
                const double p = power[fo[c] + t];
                on = is_finite(p) && p > thr;
            }
            const unsigned long long mask = __ballot(on);
            if (lane == 0) raw.word[pass * kWaves + wave] = mask;
        }
        __syncthreads();
        if (threadIdx.x == 0) raw.scan();
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            const int i = pass * kBlock + threadIdx.x;
            const long t = first_row + i;
            bool on = false;
            if (i >= ctx && i < span - ctx && t >= 0 && t < T) {
                const long lo = max(0L, t - ctx), hi = min(T - 1, t + ctx);
                const int num = raw.count((int)(lo - first_row), (int)(hi - first_row));
                on = (double)num >= (double)(hi - lo + 1) * dec.proportion;
            }
            const unsigned long long mask = __ballot(on);
            if (lane == 0) smooth.word[pass * kWaves + wave] = mask;
        }
        __syncthreads();
        if (threadIdx.x == 0) smooth.scan();
        __syncthreads();
        const long t = t0 + threadIdx.x;
        bool keep = false;
        if (t < T) {
            const long lo = max(0L, t - pad), hi = min(T - 1, t + pad);
            keep = smooth.count((int)(lo - first_row), (int)(hi - first_row)) > 0;
            flags[fo[c] + t] = keep ? 1 : 0;
            if (level_db) level_db[fo[c] + t] = (float)(10.0 * log10(power[fo[c] + t] / thr));
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) kept_word[wave] = mask;
        __syncthreads();
        if (threadIdx.x == 0) {
            int kept = 0, first = -1, last = -1;
            for (int w = 0; w < kWaves; ++w) {
                const unsigned long long k = kept_word[w];
                if (!k) continue;
                kept += __popcll(k);
                if (first < 0) first = (int)t0 + 64 * w + (__ffsll((long long)k) - 1);
                last = (int)t0 + 64 * w + 63 - __clzll((long long)k);
            }
            const int rows = (int)min((long)kBlock, T - t0);
            tiles[tile].n_raw = raw.count(halo, halo + rows - 1);
            tiles[tile].n_kept = kept;
            tiles[tile].first = first;
            tiles[tile].last = last;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void vad_clip_kernel(const long *__restrict__ to, long n_clips, const VadTile *__restrict__ tiles,
                                                          const double *__restrict__ level, dsp_vad_clip *__restrict__ clips, long *__restrict__ counts)
{
    const long c = block_index() * kBlock + threadIdx.x;
    if (c >= n_clips) return;
    long n_raw = 0, n_kept = 0;
    int first = -1, last = -1;
    for (long tile = to[c]; tile < to[c + 1]; ++tile) {
        const VadTile r = tiles[tile];
        n_raw += r.n_raw;
        n_kept += r.n_kept;
        if (first < 0) first = r.first;
        if (r.last >= 0) last = r.last;
    }
    counts[c] = n_kept;
    if (clips) clips[c] = dsp_vad_clip{level[2 * c], level[2 * c + 1], (int)n_raw, (int)n_kept, first, last};
}

// a wavefront per clip
__global__ __launch_bounds__(kBlock) void rows_count_kernel(const unsigned char *__restrict__ flags, const long *__restrict__ fo, long n_clips,
                                                            long *__restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const long c = block_index() * kWaves + (threadIdx.x >> 6);
    if (c >= n_clips) return;
    long kept = 0;
    for (long r = fo[c] + lane; r < fo[c + 1]; r += 64) kept += flags[r] != 0;
    for (int off = 32; off >= 1; off >>= 1) kept += __shfl_down(kept, off, 64);
    if (lane == 0) counts[c] = kept;
}

__global__ __launch_bounds__(kBlock) void rows_tile_count_kernel(const unsigned char *__restrict__ flags, long n_rows, long n_tiles, int *__restrict__ sel_count)
{
    __shared__ int of_wave[kWaves];
    const long tile = block_index();
    if (tile >= n_tiles) return;
    const long r = tile * kBlock + threadIdx.x;
    const unsigned long long mask = __ballot(r < n_rows && flags[r] != 0);
    if ((threadIdx.x & 63) == 0) of_wave[threadIdx.x >> 6] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int kept = 0;
        for (int w = 0; w < kWaves; ++w) kept += of_wave[w];
        sel_count[tile] = kept;
    }
}

// one block: sel_base[tile] = the kept rows of the tiles before it
__global__ __launch_bounds__(kBlock) void rows_scan_kernel(const int *__restrict__ sel_count, long n_tiles, long *__restrict__ sel_base)
{
    __shared__ long part[kBlock];
    __shared__ long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long t0 = 0; t0 < n_tiles; t0 += kBlock) {
        const long tile = t0 + threadIdx.x;
        const long own = tile < n_tiles ? sel_count[tile] : 0;
        part[threadIdx.x] = own;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const long add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (tile < n_tiles) sel_base[tile] = carry + part[threadIdx.x] - own;
        __syncthreads();
        if (threadIdx.x == kBlock - 1) carry += part[kBlock - 1];
        __syncthreads();
    }
}

// a tile's kept rows, in order, to rows [sel_base[tile], ...) of the output: a group of `lanes` lanes (a power of two >= d) per row
__global__ __launch_bounds__(kBlock) void rows_copy_kernel(const float *__restrict__ in, int d, int lanes, const unsigned char *__restrict__ flags, long n_rows,
                                                           long n_tiles, long n_out, long row_base, const long *__restrict__ sel_base, float *__restrict__ out,
                                                           long *__restrict__ row_index)
{
    __shared__ int source[kBlock];
    __shared__ int of_wave[kWaves];
    const long tile = block_index();
    if (tile >= n_tiles) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r = tile * kBlock + threadIdx.x;
    const bool keep = r < n_rows && flags[r] != 0;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) of_wave[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, kept = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += of_wave[w];
        kept += of_wave[w];
    }
    if (keep) source[before + __popcll(mask & ((1ull << lane) - 1ull))] = threadIdx.x;
    __syncthreads();
    const long base = sel_base[tile];
    const int group = threadIdx.x / lanes, j = threadIdx.x % lanes, n_groups = kBlock / lanes;
    for (int k = group; k < kept; k += n_groups) {
        const long dst = base + k, src = tile * kBlock + source[k];
        if (dst >= n_out) break;                             // (flags that hold more than kept_offsets announced: nothing past d_out's end)
        if (j < d) out[dst * d + j] = in[src * d + j];
        if (row_index && j == 0) row_index[dst] = row_base + src;
    }
}

long persistent_grid(long tiles) { return std::min(std::max(tiles, 1L), kMaxGrid); }

}  // namespace

hipError_t launch_vad_power(const float *d_signal, const VadWorkspace &ws, long n_clips, long n_tiles, const VadGeometry &geo, int frame_length, int hop,
                            double *d_power, hipStream_t stream)
{
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(vad_power_kernel, dim3((unsigned)persistent_grid(n_tiles)), dim3(kBlock), 0, stream, d_signal, ws.so, ws.fo, ws.to, n_clips, n_tiles, geo,
                       frame_length, hop, d_power);
    return hipGetLastError();
}

hipError_t launch_vad_decide(const double *d_power, const VadWorkspace &ws, long n_clips, long n_tiles, const VadDecision &dec, unsigned char *d_flags,
                             float *d_level_db, dsp_vad_clip *d_clips, hipStream_t stream)
{
    const dim3 per_clip = grid_for(ceil_div(n_clips, kBlock)), per_tile((unsigned)persistent_grid(n_tiles));
    if (dec.reference != DSP_VAD_REF_ABSOLUTE) {
        const hipError_t e = hipMemsetAsync(ws.ref_key, 0, (size_t)n_clips * sizeof(unsigned long long), stream);
        if (e != hipSuccess) return e;
        if (n_tiles)
            hipLaunchKernelGGL(vad_stats_kernel, per_tile, dim3(kBlock), 0, stream, d_power, ws.fo, ws.to, n_clips, n_tiles, ws.ref_key, ws.tiles);
    }
    hipLaunchKernelGGL(vad_level_kernel, per_clip, dim3(kBlock), 0, stream, ws.to, n_clips, ws.ref_key, ws.tiles, dec, ws.level);
    if (n_tiles)
        hipLaunchKernelGGL(vad_decide_kernel, per_tile, dim3(kBlock), 0, stream, d_power, ws.fo, ws.to, n_clips, n_tiles, ws.level, dec, d_flags, d_level_db, ws.tiles);
    hipLaunchKernelGGL(vad_clip_kernel, per_clip, dim3(kBlock), 0, stream, ws.to, n_clips, ws.tiles, ws.level, d_clips, ws.counts);
    return hipGetLastError();
}

hipError_t launch_rows_count(const unsigned char *d_flags, const VadWorkspace &ws, long n_clips, hipStream_t stream)
{
    hipLaunchKernelGGL(rows_count_kernel, grid_for(ceil_div(n_clips, kWaves)), dim3(kBlock), 0, stream, d_flags, ws.fo, n_clips, ws.counts);
    return hipGetLastError();
}

hipError_t launch_rows_select(const float *d_in, int d, const unsigned char *d_flags, long n_rows, long n_out, long row_base, const VadWorkspace &ws,
                              float *d_out, long *d_row_index, hipStream_t stream)
{
    const long n_tiles = ceil_div(n_rows, kBlock);
    if (n_tiles == 0 || n_out == 0) return hipSuccess;
    int lanes = 1;
    while (lanes < d) lanes *= 2;
    hipLaunchKernelGGL(rows_tile_count_kernel, grid_for(n_tiles), dim3(kBlock), 0, stream, d_flags, n_rows, n_tiles, ws.sel_count);
    hipLaunchKernelGGL(rows_scan_kernel, dim3(1), dim3(kBlock), 0, stream, ws.sel_count, n_tiles, ws.sel_base);
    hipLaunchKernelGGL(rows_copy_kernel, grid_for(n_tiles), dim3(kBlock), 0, stream, d_in, d, lanes, d_flags, n_rows, n_tiles, n_out, row_base, ws.sel_base, d_out,
                       d_row_index);
    return hipGetLastError();
}

}  // namespace dsp
