// segment_kernels.hpp -- segments from window scores (include/dsp_amd.h dsp_segments_device): the layout of the
// segmenter's workspace, the per-block search for segment heads and tails that host and device share, and what capi_segments.cpp hands the kernels
// of segment_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dsp_amd.h"
#include "score_matrix.hpp"

namespace dsp {

// Time is cut into words of 64 windows (one bit per window, bit i of word j = window 64 j + i of the recording) and chunks of 64 words:
// a chunk is what one wavefront settles without looking at another.  Words and chunks are counted per recording, from its first window.
constexpr int kSegWord = 64;
constexpr int kSegChunkWords = 64;
constexpr int kSegChunk = kSegWord * kSegChunkWords;         // 4096 windows
constexpr long kSegMaxColumns = 1L << 19;
constexpr long kSegMaxTracks = 1L << 31;
// below this many columns a wavefront's lanes run along time (one column, 64 consecutive windows per load); from it on they run across
// columns (64 consecutive columns of one window per load).  Either way a load is 64 floats that lie together or S apart with S small.
constexpr long kSegLanesAcrossColumns = 32;
constexpr int kSegScanTile = 4096;                           // track counts per block of the prefix sums

__host__ __device__ inline long seg_words(long windows) { return (windows + kSegWord - 1) / kSegWord; }
__host__ __device__ inline long seg_chunks(long windows) { return (windows + kSegChunk - 1) / kSegChunk; }

// Hysteresis inside one word.  set: windows with e >= on, keep: windows with e >= off (set is a subset: off <= on).  state[i] = set[i] |
// (keep[i] & state[i - 1]) is a carry chain: g receives the state with 0 before the word, p the windows that every window from the
// word's first up to them keeps -- those that are also on when the state before the word is 1.  Six doubling steps (Kogge-Stone).
__host__ __device__ inline void seg_word_scan(uint64_t set, uint64_t keep, uint64_t &g, uint64_t &p)
{
    g = set;
    p = keep;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        g |= p & (g << d);
        p &= (p << d) | ((1ull << d) - 1);
    }
}

// The mask kernels leave two words per 64 windows, [word][column]: a = the state with 0 in front of the word's CHUNK, b = the windows
// that are on in addition when 1 is in front of it.  A chunk's last a and b bits are its transfer function; a lane per track composes
// them in order (a few steps: 9 chunks an hour) and leaves the state in front of each chunk, and the state kernel folds it in: from
// there on `a` holds the state itself.
//
// Merging, dropping and counting run per BLOCK of 8 words (512 windows), every block of every track at once.  With the position of the
// last 1 before a rise and of the first 1 after a fall, both rules are local:
//   a rise at p is a HEAD (a segment starts) when no 1 lies in [p - 1 - max_gap, p - 1]
//   a fall at q is a TAIL (a segment ends)   when no 1 lies in [q + 1, q + 1 + max_gap]
// Heads and tails alternate along a track, segment k = [head k, tail k], and it survives when tail - head + 1 >= min_windows.  What a
// block needs from outside is three positions -- the last 1 before it, the first 1 after it, the first tail after it -- which small
// per-track passes over the blocks' own first / last 1 and first tail provide (prefix, suffix, suffix).
constexpr int kSegBlockWords = 8;
constexpr int kSegBlock = kSegWord * kSegBlockWords;
__host__ __device__ inline long seg_blocks(long windows) { return (windows + kSegBlock - 1) / kSegBlock; }
constexpr long kSegNoneBefore = -(1L << 60), kSegNoneAfter = 1L << 60;      // "no 1 before / after": farther than any gap

struct SegState {
    const uint64_t *word;                                    // the track's first state word
    long stride;                                             // columns
    __host__ __device__ uint64_t at(long j) const { return word[j * stride]; }
};

// first and last 1 of words [w0, w0 + n) as window positions, -1 without one
__host__ __device__ inline void seg_block_ones(const SegState &st, long w0, int n, int &first, int &last)
{
    first = last = -1;
    for (int j = 0; j < n; ++j) {
        const uint64_t v = st.at(w0 + j);
        if (!v) continue;
        if (first < 0) first = (int)((w0 + j) * kSegWord + __builtin_ctzll(v));
        last = (int)((w0 + j) * kSegWord + 63 - __builtin_clzll(v));
    }
}

// The heads and tails of words [w0, w0 + n) of a track, in ascending order: on_head(p), on_tail(q).  prev_one: the last 1 before the
// block (kSegNoneBefore without one), next_one: the first 1 after it (kSegNoneAfter).  A run that comes in from the block before has no
// rise here, one that goes on into the next block no fall.  Words of all 0 or all 1 cost one step, others one step per run.
template <class Head, class Tail>
__host__ __device__ inline void seg_block_events(const SegState &st, long w0, int n, long prev_one, long next_one, long max_gap, Head on_head, Tail on_tail)
{
    const long begin = w0 * kSegWord, end = (w0 + n) * kSegWord - 1;        // (windows past the recording's end are 0)
    bool have = false, in_run = false;
    long last_b = prev_one, run_a = 0;                       // the run before: its end (or prev_one); the run in progress: its start
    bool last_falls = false;
    auto run = [&](long a, long b) {
        if (have && last_falls && a - last_b - 1 > max_gap) on_tail(last_b);
        const bool rises = a > begin || prev_one != begin - 1;
        if (rises && a - last_b - 1 > max_gap) on_head(a);
        have = true;
        last_b = b;
        last_falls = b < end || next_one != end + 1;
    };
    for (int j = 0; j < n; ++j) {
        uint64_t v = st.at(w0 + j);
        const long base = (w0 + j) * kSegWord;
        if (in_run) {
            if (v == ~0ull) continue;
            const int z = __builtin_ctzll(~v);               // the run ends in front of the word's first 0
            run(run_a, base + z - 1);
            in_run = false;
            v &= ~((1ull << z) - 1);
        }
        while (v) {
            const int a = __builtin_ctzll(v);
            const uint64_t rest = ~(v >> a);                  // (the shift brings in 0s: rest != 0 unless a == 0 and v is all 1)
            const int len = rest ? __builtin_ctzll(rest) : 64;
            if (a + len >= 64) { in_run = true; run_a = base + a; break; }
            run(base + a, base + a + len - 1);
            v &= ~(((1ull << len) - 1) << a);
        }
    }
    if (in_run) run(run_a, end);
    if (have && last_falls && next_one - last_b - 1 > max_gap) on_tail(last_b);
}

// the block's first tail, -1 without one
__host__ __device__ inline int seg_block_first_tail(const SegState &st, long w0, int n, long prev_one, long next_one, long max_gap)
{
    long first = -1;
    seg_block_events(st, w0, n, prev_one, next_one, max_gap, [](long) {}, [&](long q) { if (first < 0) first = q; });
    return (int)first;
}

// the segments whose head lies in the block, ascending: emit(first_window, n_windows) for those of min_windows or more -> how many.
// next_tail: the first tail after the block (there is one whenever a head of the block has no tail in it).
template <class Emit>
__host__ __device__ inline int seg_block_segments(const SegState &st, long w0, int n, long prev_one, long next_one, long next_tail, long max_gap,
                                                  long min_windows, Emit emit)
{
    int count = 0;
    long head = -1;
    auto close = [&](long q) {
        if (head >= 0 && q - head + 1 >= min_windows) { emit(head, q - head + 1); ++count; }
        head = -1;
    };
    seg_block_events(st, w0, n, prev_one, next_one, max_gap, [&](long p) { head = p; }, close);
    if (head >= 0) close(next_tail);
    return count;
}

// The workspace, laid out by seg_layout over one grow-only buffer (score_matrix.hpp Carver).  Nothing in it is read before the call
// has written it.
struct SegWorkspace {
    uint64_t *a = nullptr, *b = nullptr;                     // [words of all recordings][S]
    uint8_t *chunk_in = nullptr;                             // [chunks of all recordings][S]
    int *best = nullptr;                                     // [windows], DSP_SEG_EXCLUSIVE only: the row's best column, -1 without one
    int *prev_one = nullptr, *next_one = nullptr, *next_tail = nullptr;      // [blocks of all recordings][S], -1: none
    int *counts = nullptr;                                   // [units]: a unit is a (recording, column, block), in that order
    long *base = nullptr;                                    // [units]: the unit's first segment in the output
    long *tile_sum = nullptr, *tile_base = nullptr;          // [ceil(units / kSegScanTile)]
};
// words, chunks and blocks here are counted over all columns (those of all recordings * S); units = blocks
inline SegWorkspace seg_layout(Carver &c, long words, long chunks, long blocks, long windows, bool exclusive)
{
    const size_t tiles = (size_t)ceil_div(blocks, kSegScanTile);
    SegWorkspace w;
    w.a = c.take<uint64_t>((size_t)words);
    w.b = c.take<uint64_t>((size_t)words);
    w.chunk_in = c.take<uint8_t>((size_t)chunks);
    if (exclusive) w.best = c.take<int>((size_t)windows);
    w.prev_one = c.take<int>((size_t)blocks);
    w.next_one = c.take<int>((size_t)blocks);
    w.next_tail = c.take<int>((size_t)blocks);
    w.counts = c.take<int>((size_t)blocks);
    w.base = c.take<long>((size_t)blocks);
    w.tile_sum = c.take<long>(tiles);
    w.tile_base = c.take<long>(tiles);
    return w;
}
inline size_t seg_workspace_bytes(long words, long chunks, long blocks, long windows, bool exclusive)
{
    Carver c;
    seg_layout(c, words, chunks, blocks, windows, exclusive);
    return c.at;
}
inline SegWorkspace seg_carve(char *p, long words, long chunks, long blocks, long windows, bool exclusive)
{
    Carver c{p};
    return seg_layout(c, words, chunks, blocks, windows, exclusive);
}

// What one call needs on the device.  d_offsets: four arrays of n_recordings + 1 longs one behind the other -- window, word, chunk and
// block offsets of the recordings (prefix sums, per column).  Everything is enqueued on `stream`; nothing waits for it.
struct SegCall {
    const float *scores;
    const long *offsets;
    long n_recordings, columns, windows, words, chunks, blocks;      // totals over the recordings, per column
    float on, off;
    long min_windows, max_gap;
    bool exclusive;
    dsp_segment *segments;
    long max_segments;                                       // 0 with segments == nullptr
    int *track_counts;                                       // may be nullptr
    long *total;
};
hipError_t launch_segments(const SegCall &call, const SegWorkspace &ws, hipStream_t stream);

}  // namespace dsp
