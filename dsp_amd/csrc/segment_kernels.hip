// segment_kernels.hip -- segments from window scores (include/dsp_amd.h dsp_segments_device).
//
//   seg_best_*      DSP_SEG_EXCLUSIVE only: the best column of every window's row (the smallest that attains the maximum of the non-NaN
//                   entries, -1 for a row of NaN)
//   seg_mask_*      the thresholds and the hysteresis: a wavefront takes one chunk of 4096 windows and leaves the chunk's 64 state words,
//                   twice -- for state 0 and for state 1 in front of the chunk.  Below kSegLanesAcrossColumns columns the lanes run
//                   along time: the two tests of 64 windows are two __ballot masks, lane j keeps those of word j, settles its word in
//                   six doubling steps, and the 64 words' carries are settled the same way on the ballots of their last bits.  From
//                   there on the lanes run across columns: a lane builds its column's words bit by bit from loads that are coalesced
//                   across the wavefront and carries its own state from word to word.
//   seg_carry       a lane per track over its chunks (9 an hour): the chunks' last a and b bits composed in order -> the state in front of
//                   each chunk
//   seg_state       a lane per (block of 8 words, column): folds that state in -- from here on `a` is the state -- and notes the block's
//                   first and last 1
//   seg_track_scan  a lane per track over its blocks: the last 1 before each block (prefix), the first 1 after it, the first tail after
//                   it (suffix), each in place over what the blocks noted
//   seg_tails       a lane per (block, column): the block's first tail
//   seg_segments    a lane per (block, column): the segments whose head lies in the block -- once to count, and after the prefix sums
//                   of the counts once more to write recording, column, first_window and n_windows where the sums say.  Merging and
//                   dropping are local tests on rises and falls (segment_kernels.hpp), so every block of every track runs at once
//   seg_tile_*      exclusive prefix sums of the counts in (recording, column, block) order, which is the output's order (tiles of 4096
//                   counts, the tiles' sums, the units); seg_track_counts: a track's count is the difference of two of them
//   seg_stats       a wavefront per written segment, grid-stride over the device-side count: n_active, peak, peak_window and the float64
//                   sum of the active windows -- lane l adds windows first + l, first + l + 64, ... and the lanes are added in a fixed
//                   tree, so the order depends on the segment alone
// No atomics.  Every index is checked against the recording's windows before a load and against max_segments before a store.
#include <climits>
#include <cmath>

#include "segment_kernels.hpp"

namespace dsp {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kScanPerThread = kSegScanTile / kThreads;

__device__ inline long least(long x, long y) { return x < y ? x : y; }

// offsets: wo | wdo | co | bo, n + 1 longs each
struct SegOffsets {
    const long *wo, *wdo, *co, *bo;
    __device__ SegOffsets(const long *p, long n) : wo(p), wdo(p + (n + 1)), co(p + 2 * (n + 1)), bo(p + 3 * (n + 1)) {}
};

// the recording that owns `chunk` (or block, with bo): the largest r < n with co[r] <= chunk (recordings without windows own none)
// (span_find.hpp's owner_of finds the same recording; this form stays because joining it changes the kernels' instructions, which nobody has timed)
__device__ long owner_of_chunk(const long *co, long n, long chunk)
{
    long lo = 0, hi = n;
    while (hi - lo > 1) {
        const long mid = lo + (hi - lo) / 2;
        if (co[mid] <= chunk) lo = mid; else hi = mid;
    }
    return lo;
}

// (value, column) of a row's best entry so far; column INT_MAX: none
__device__ inline void best_take(float &v, int &c, float ov, int oc)
{
    if (oc != INT_MAX && (c == INT_MAX || ov > v || (ov == v && oc < c))) { v = ov; c = oc; }
}

__global__ __launch_bounds__(kThreads) void seg_best_rows_kernel(const float *__restrict__ scores, long windows, long S, int *__restrict__ best)
{
    const long w = (long)blockIdx.x * kThreads + threadIdx.x;
    if (w >= windows) return;
    float v = 0.0f;
    int c = INT_MAX;
    for (long s = 0; s < S; ++s) {
        const float x = scores[w * S + s];
        if (x == x) best_take(v, c, x, (int)s);
    }
    best[w] = c == INT_MAX ? -1 : c;
}

__global__ __launch_bounds__(kThreads) void seg_best_waves_kernel(const float *__restrict__ scores, long windows, long S, int *__restrict__ best)
{
    const long w = (long)blockIdx.x * kWaves + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (w >= windows) return;
    float v = 0.0f;
    int c = INT_MAX;
    for (long s = lane; s < S; s += 64) {
        const float x = scores[w * S + s];
        if (x == x) best_take(v, c, x, (int)s);
    }
    for (int step = 1; step < 64; step <<= 1) best_take(v, c, __shfl_xor(v, step, 64), __shfl_xor(c, step, 64));
    if (lane == 0) best[w] = c == INT_MAX ? -1 : c;
}

// e[w] of one window: NaN past the recording's end, -inf outside the row's best column under DSP_SEG_EXCLUSIVE
__device__ inline float effective(const float *__restrict__ scores, const int *__restrict__ best, long row, long S, long s)
{
    const float x = scores[row * S + s];
    return best && best[row] != (int)s ? -INFINITY : x;
}

__global__ __launch_bounds__(kThreads) void seg_mask_time_kernel(const float *__restrict__ scores, const long *__restrict__ offsets, long n, long S, long units,
                                                                 float on, float off, const int *__restrict__ best, uint64_t *__restrict__ a,
                                                                 uint64_t *__restrict__ b)
{
    const long unit = (long)blockIdx.x * kWaves + threadIdx.x / 64;          // (chunk, column)
    const int lane = threadIdx.x & 63;
    if (unit >= units) return;
    const SegOffsets o(offsets, n);
    const long chunk = unit / S, s = unit % S;
    const long r = owner_of_chunk(o.co, n, chunk), c = chunk - o.co[r];
    const long W = o.wo[r + 1] - o.wo[r], row0 = o.wo[r];
    const long words = least(kSegChunkWords, seg_words(W) - c * kSegChunkWords);
    uint64_t set = 0, keep = 0;
    for (long j = 0; j < words; ++j) {
        const long w = c * kSegChunk + j * kSegWord + lane;
        const float e = w < W ? effective(scores, best, row0 + w, S, s) : NAN;
        const uint64_t sm = __ballot(e >= on), km = __ballot(e >= off);
        if (lane == j) { set = sm; keep = km; }
    }
    uint64_t g, p, G, P;
    seg_word_scan(set, keep, g, p);
    seg_word_scan(__ballot((int)(g >> 63)), __ballot((int)(p >> 63)), G, P);   // bit j: word j's last state / all of words 0 .. j keep
    const uint64_t in0 = ((G << 1) >> lane) & 1, through = (((P << 1) | 1) >> lane) & 1;
    if (lane < words) {
        const long at = (o.wdo[r] + c * kSegChunkWords + lane) * S + s;
        a[at] = g | (p & (0 - in0));
        b[at] = p & (0 - through);
    }
}

__global__ __launch_bounds__(kThreads) void seg_mask_columns_kernel(const float *__restrict__ scores, const long *__restrict__ offsets, long n, long S,
                                                                    long groups, long units, float on, float off, const int *__restrict__ best,
                                                                    uint64_t *__restrict__ a, uint64_t *__restrict__ b)
{
    const long unit = (long)blockIdx.x * kWaves + threadIdx.x / 64;          // (chunk, group of 64 columns)
    if (unit >= units) return;
    const SegOffsets o(offsets, n);
    const long chunk = unit / groups, s = (unit % groups) * 64 + (threadIdx.x & 63);
    if (s >= S) return;
    const long r = owner_of_chunk(o.co, n, chunk), c = chunk - o.co[r];
    const long W = o.wo[r + 1] - o.wo[r], row0 = o.wo[r];
    const long words = least(kSegChunkWords, seg_words(W) - c * kSegChunkWords);
    uint64_t in0 = 0, through = 1;
    for (long j = 0; j < words; ++j) {
        const long w0 = c * kSegChunk + j * kSegWord;
        const int bits = (int)least(kSegWord, W - w0);
        uint64_t set = 0, keep = 0;
        for (int i = 0; i < bits; ++i) {
            const float e = effective(scores, best, row0 + w0 + i, S, s);
            set |= (uint64_t)(e >= on) << i;
            keep |= (uint64_t)(e >= off) << i;
        }
        uint64_t g, p;
        seg_word_scan(set, keep, g, p);
        const long at = (o.wdo[r] + c * kSegChunkWords + j) * S + s;
        const uint64_t state0 = g | (p & (0 - in0));
        a[at] = state0;
        b[at] = p & (0 - through);
        in0 = state0 >> 63;
        through &= p >> 63;
    }
}

__global__ __launch_bounds__(kThreads) void seg_carry_kernel(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, uint8_t *__restrict__ chunk_in,
                                                             const long *__restrict__ offsets, long n, long S, long tracks)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= tracks) return;
    const SegOffsets o(offsets, n);
    const long r = t / S, s = t % S;
    const long n_words = o.wdo[r + 1] - o.wdo[r], chunks = o.co[r + 1] - o.co[r];
    uint64_t in = 0;
    for (long c = 0; c < chunks; ++c) {
        chunk_in[(o.co[r] + c) * S + s] = (uint8_t)in;
        const long last = (o.wdo[r] + least(n_words, (c + 1) * kSegChunkWords) - 1) * S + s;
        in = (a[last] >> 63) | ((b[last] >> 63) & in);
    }
}

// a unit is a (block, column): block `bg` of all recordings' blocks, column s = the fastest index
struct SegUnit {
    long r, s, blk, w0, at;          // recording, column, block and its first word within the recording, index into the per-block arrays
    int n;                           // words in the block
    __device__ SegUnit(const SegOffsets &o, long n_rec, long S, long unit) : at(unit)
    {
        const long bg = unit / S;
        s = unit % S;
        r = owner_of_chunk(o.bo, n_rec, bg);
        blk = bg - o.bo[r];
        w0 = blk * kSegBlockWords;
        n = (int)least(kSegBlockWords, o.wdo[r + 1] - o.wdo[r] - w0);
    }
};

__global__ __launch_bounds__(kThreads) void seg_state_kernel(uint64_t *__restrict__ a, const uint64_t *__restrict__ b, const uint8_t *__restrict__ chunk_in,
                                                             const long *__restrict__ offsets, long n, long S, long units, int *__restrict__ last_one,
                                                             int *__restrict__ first_one)
{
    const long unit = (long)blockIdx.x * kThreads + threadIdx.x;
    if (unit >= units) return;
    const SegOffsets o(offsets, n);
    const SegUnit u(o, n, S, unit);
    const uint64_t in = chunk_in[(o.co[u.r] + u.w0 / kSegChunkWords) * S + u.s];      // (a block lies in one chunk)
    for (int j = 0; j < u.n; ++j) {
        const long at = (o.wdo[u.r] + u.w0 + j) * S + u.s;
        a[at] |= b[at] & (0 - in);
    }
    int first, last;
    seg_block_ones(SegState{a + o.wdo[u.r] * S + u.s, S}, u.w0, u.n, first, last);
    last_one[unit] = last;
    first_one[unit] = first;
}

// in place over a track's blocks: v[i] <- the last non-negative entry before i (forward) or the first one after i (backward), -1 without
__global__ __launch_bounds__(kThreads) void seg_track_scan_kernel(int *__restrict__ v, const long *__restrict__ offsets, long n, long S, long tracks, bool forward)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= tracks) return;
    const SegOffsets o(offsets, n);
    const long r = t / S, s = t % S, blocks = o.bo[r + 1] - o.bo[r];
    int running = -1;
    for (long i = 0; i < blocks; ++i) {
        const long at = (o.bo[r] + (forward ? i : blocks - 1 - i)) * S + s;
        const int mine = v[at];
        v[at] = running;
        if (mine >= 0) running = mine;
    }
}

__device__ inline long none_before(int p) { return p < 0 ? kSegNoneBefore : p; }
__device__ inline long none_after(int p) { return p < 0 ? kSegNoneAfter : p; }

__global__ __launch_bounds__(kThreads) void seg_tails_kernel(const uint64_t *__restrict__ a, const long *__restrict__ offsets, long n, long S, long units, long max_gap,
                                                             const int *__restrict__ prev_one, const int *__restrict__ next_one, int *__restrict__ first_tail)
{
    const long unit = (long)blockIdx.x * kThreads + threadIdx.x;
    if (unit >= units) return;
    const SegOffsets o(offsets, n);
    const SegUnit u(o, n, S, unit);
    first_tail[unit] = seg_block_first_tail(SegState{a + o.wdo[u.r] * S + u.s, S}, u.w0, u.n, none_before(prev_one[unit]), none_after(next_one[unit]), max_gap);
}

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void seg_segments_kernel(const uint64_t *__restrict__ a, const long *__restrict__ offsets, long n, long S, long units,
                                                                long max_gap, long min_windows, const int *__restrict__ prev_one, const int *__restrict__ next_one,
                                                                const int *__restrict__ next_tail, int *__restrict__ counts, const long *__restrict__ base,
                                                                dsp_segment *__restrict__ segments, long max_segments)
{
    const long unit = (long)blockIdx.x * kThreads + threadIdx.x;
    if (unit >= units) return;
    const SegOffsets o(offsets, n);
    const SegUnit u(o, n, S, unit);
    const SegState st{a + o.wdo[u.r] * S + u.s, S};
    const long po = none_before(prev_one[unit]), no = none_after(next_one[unit]), nt = next_tail[unit];
    const long ordered = o.bo[u.r] * S + u.s * (o.bo[u.r + 1] - o.bo[u.r]) + u.blk;      // (recording, column, block): the output's order
    if constexpr (EMIT) {
        long k = base[ordered];
        seg_block_segments(st, u.w0, u.n, po, no, nt, max_gap, min_windows, [&](long first, long windows) {
            if (k < max_segments) {
                dsp_segment &out = segments[k];
                out.recording = (int)u.r;
                out.column = (int)u.s;
                out.first_window = (int)first;
                out.n_windows = (int)windows;
            }
            ++k;
        });
    } else {
        counts[ordered] = seg_block_segments(st, u.w0, u.n, po, no, nt, max_gap, min_windows, [](long, long) {});
    }
}

__global__ __launch_bounds__(kThreads) void seg_track_counts_kernel(const long *__restrict__ base, const long *__restrict__ total, const long *__restrict__ offsets,
                                                                    long n, long S, long tracks, long units, int *__restrict__ track_counts)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= tracks) return;
    const SegOffsets o(offsets, n);
    const long r = t / S, s = t % S, blocks = o.bo[r + 1] - o.bo[r];
    const long first = o.bo[r] * S + s * blocks, next = first + blocks;
    track_counts[t] = blocks == 0 ? 0 : (int)((next < units ? base[next] : total[0]) - base[first]);
}

// exclusive prefix sum of one value per thread over the block; total = the block's sum.  lds: kThreads longs.
__device__ long block_exclusive(long v, long *lds, long &total)
{
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const long add = tid >= d ? lds[tid - d] : 0;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    total = lds[kThreads - 1];
    const long inclusive = lds[tid];
    __syncthreads();
    return inclusive - v;
}

__global__ __launch_bounds__(kThreads) void seg_tile_sum_kernel(const int *__restrict__ counts, long tracks, long *__restrict__ tile_sum)
{
    __shared__ long lds[kThreads];
    const long t0 = (long)blockIdx.x * kSegScanTile + (long)threadIdx.x * kScanPerThread;
    long mine = 0;
    for (int i = 0; i < kScanPerThread; ++i)
        if (t0 + i < tracks) mine += counts[t0 + i];
    long total;
    block_exclusive(mine, lds, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one block: the tiles' bases, and the call's total[2] = segments found, segments written
__global__ __launch_bounds__(kThreads) void seg_tile_base_kernel(const long *__restrict__ tile_sum, long tiles, long *__restrict__ tile_base, long max_segments,
                                                                 long *__restrict__ total)
{
    __shared__ long lds[kThreads];
    long running = 0;
    for (long i0 = 0; i0 < tiles; i0 += kThreads) {
        const long i = i0 + threadIdx.x;
        long sum;
        const long before = block_exclusive(i < tiles ? tile_sum[i] : 0, lds, sum);
        if (i < tiles) tile_base[i] = running + before;
        running += sum;
    }
    if (threadIdx.x == 0) {
        total[0] = running;
        total[1] = least(running, max_segments);
    }
}

__global__ __launch_bounds__(kThreads) void seg_track_base_kernel(const int *__restrict__ counts, long tracks, const long *__restrict__ tile_base,
                                                                  long *__restrict__ base)
{
    __shared__ long lds[kThreads];
    const long t0 = (long)blockIdx.x * kSegScanTile + (long)threadIdx.x * kScanPerThread;
    long mine = 0;
    for (int i = 0; i < kScanPerThread; ++i)
        if (t0 + i < tracks) mine += counts[t0 + i];
    long total;
    long at = tile_base[blockIdx.x] + block_exclusive(mine, lds, total);
    for (int i = 0; i < kScanPerThread; ++i)
        if (t0 + i < tracks) { base[t0 + i] = at; at += counts[t0 + i]; }
}

__global__ __launch_bounds__(kThreads) void seg_stats_kernel(const float *__restrict__ scores, const uint64_t *__restrict__ a,
                                                             const long *__restrict__ offsets, long n, long S,
                                                             dsp_segment *__restrict__ segments, const long *__restrict__ total)
{
    const SegOffsets o(offsets, n);
    const int lane = threadIdx.x & 63;
    const long written = total[1], stride = (long)gridDim.x * kWaves;
    for (long k = (long)blockIdx.x * kWaves + threadIdx.x / 64; k < written; k += stride) {
        const long r = segments[k].recording, s = segments[k].column, first = segments[k].first_window, windows = segments[k].n_windows;
        double sum = 0.0;
        int active = 0, peak_window = INT_MAX;
        float peak = 0.0f;
        for (long w = first + lane; w < first + windows; w += 64) {
            const long word = (o.wdo[r] + w / kSegWord) * S + s;
            const uint64_t state = a[word];
            if ((state >> (w % kSegWord)) & 1) {
                const float x = scores[(o.wo[r] + w) * S + s];
                sum += (double)x;
                ++active;
                if (peak_window == INT_MAX || x > peak) { peak = x; peak_window = (int)w; }
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {                  // lane l takes lane l + d: a fixed tree, lane 0 holds the segment
            sum += __shfl_down(sum, d, 64);
            active += __shfl_down(active, d, 64);
            best_take(peak, peak_window, __shfl_down(peak, d, 64), __shfl_down(peak_window, d, 64));
        }
        if (lane == 0) {
            dsp_segment &out = segments[k];
            out.n_active = active;
            out.peak_window = peak_window;
            out.peak = peak;
            out.mean = (float)(sum / (double)active);
        }
    }
}

unsigned blocks_for(long items, long per_block) { return (unsigned)ceil_div(items, per_block); }

}  // namespace

hipError_t launch_segments(const SegCall &q, const SegWorkspace &ws, hipStream_t st)
{
    const long S = q.columns, tracks = q.n_recordings * S;
    if (q.exclusive && q.windows > 0) {
        if (S < kSegLanesAcrossColumns)
            seg_best_rows_kernel<<<blocks_for(q.windows, kThreads), kThreads, 0, st>>>(q.scores, q.windows, S, ws.best);
        else
            seg_best_waves_kernel<<<blocks_for(q.windows, kWaves), kThreads, 0, st>>>(q.scores, q.windows, S, ws.best);
    }
    const int *best = q.exclusive ? ws.best : nullptr;
    if (q.chunks > 0) {
        if (S < kSegLanesAcrossColumns) {
            const long units = q.chunks * S;
            seg_mask_time_kernel<<<blocks_for(units, kWaves), kThreads, 0, st>>>(q.scores, q.offsets, q.n_recordings, S, units, q.on, q.off, best, ws.a, ws.b);
        } else {
            const long groups = ceil_div(S, 64), units = q.chunks * groups;
            seg_mask_columns_kernel<<<blocks_for(units, kWaves), kThreads, 0, st>>>(q.scores, q.offsets, q.n_recordings, S, groups, units, q.on, q.off, best,
                                                                                   ws.a, ws.b);
        }
    }
    const long units = q.blocks * S, tiles = ceil_div(units, kSegScanTile);
    const unsigned track_blocks = blocks_for(tracks, kThreads), unit_blocks = blocks_for(units, kThreads);
    if (units > 0) {
        seg_carry_kernel<<<track_blocks, kThreads, 0, st>>>(ws.a, ws.b, ws.chunk_in, q.offsets, q.n_recordings, S, tracks);
        seg_state_kernel<<<unit_blocks, kThreads, 0, st>>>(ws.a, ws.b, ws.chunk_in, q.offsets, q.n_recordings, S, units, ws.prev_one, ws.next_one);
        seg_track_scan_kernel<<<track_blocks, kThreads, 0, st>>>(ws.prev_one, q.offsets, q.n_recordings, S, tracks, true);
        seg_track_scan_kernel<<<track_blocks, kThreads, 0, st>>>(ws.next_one, q.offsets, q.n_recordings, S, tracks, false);
        seg_tails_kernel<<<unit_blocks, kThreads, 0, st>>>(ws.a, q.offsets, q.n_recordings, S, units, q.max_gap, ws.prev_one, ws.next_one, ws.next_tail);
        seg_track_scan_kernel<<<track_blocks, kThreads, 0, st>>>(ws.next_tail, q.offsets, q.n_recordings, S, tracks, false);
        seg_segments_kernel<false><<<unit_blocks, kThreads, 0, st>>>(ws.a, q.offsets, q.n_recordings, S, units, q.max_gap, q.min_windows, ws.prev_one, ws.next_one,
                                                                     ws.next_tail, ws.counts, nullptr, nullptr, 0);
        seg_tile_sum_kernel<<<(unsigned)tiles, kThreads, 0, st>>>(ws.counts, units, ws.tile_sum);
    }
    seg_tile_base_kernel<<<1, kThreads, 0, st>>>(ws.tile_sum, tiles, ws.tile_base, q.max_segments, q.total);
    if (units > 0) seg_track_base_kernel<<<(unsigned)tiles, kThreads, 0, st>>>(ws.counts, units, ws.tile_base, ws.base);
    if (q.track_counts)
        seg_track_counts_kernel<<<track_blocks, kThreads, 0, st>>>(ws.base, q.total, q.offsets, q.n_recordings, S, tracks, units, q.track_counts);
    if (q.segments && q.max_segments > 0 && units > 0) {
        seg_segments_kernel<true><<<unit_blocks, kThreads, 0, st>>>(ws.a, q.offsets, q.n_recordings, S, units, q.max_gap, q.min_windows, ws.prev_one, ws.next_one,
                                                                    ws.next_tail, nullptr, ws.base, q.segments, q.max_segments);
        const long waves = std::min<long>(q.max_segments, 1L << 16);
        seg_stats_kernel<<<blocks_for(waves, kWaves), kThreads, 0, st>>>(q.scores, ws.a, q.offsets, q.n_recordings, S, q.segments, q.total);
    }
    return hipGetLastError();
}

}  // namespace dsp
