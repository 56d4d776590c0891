// vad_kernels.hpp -- voice activity detection on ragged batches (include/dsp_amd.h dsp_vad_*, dsp_rows_*): the
// geometry that the frame length, the hop and the framing fix, the workspace's layout and the launchers of vad_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <numeric>

#include "score_matrix.hpp"

namespace dsp {

constexpr int kVadTileRows = 256;         // rows of a clip per tile = threads per block: one row per thread in the decision
constexpr int kVadMaxSubBlocks = 64;      // m: sub-blocks per frame
constexpr int kVadMaxFrame = 4096;
constexpr int kVadMaxContext = 64;        // context_frames and pad_frames, each
constexpr int kVadSlots = 2048;           // sub-block sums a block keeps in LDS at a time (16 KiB)
constexpr int kVadMaxDim = 64;            // columns of a matrix whose rows are selected

// What frame_length, hop_length and the framing fix.  Frame t of a clip is sub-blocks [b0(t), b0(t) + m) of g samples, b0(t) =
// (t hop - lead) / g; a block keeps the sums of a chunk of rows in LDS, row r of the chunk at slots [r stride, r stride + m).
struct VadGeometry {
    int g = 0, m = 0;
    int lead = 0;            // samples of frame 0 before the clip
    int lanes = 0;           // lanes that share one sub-block: the least power of two >= ceil(g / 4), at most 64
    int stride = 0;          // min(hop / g, m): overlapping frames share slots, disjoint ones skip the samples between them
    int chunk_rows = 0;      // rows per chunk: (chunk_rows - 1) stride + m <= kVadSlots, at most kVadTileRows
};

// the geometry, or false and why
inline bool vad_geometry(int frame_length, int hop, int framing, VadGeometry &geo, std::string &why)
{
    if (hop < 1) { why = "hop_length must be >= 1"; return false; }
    if (frame_length < 1 || frame_length > kVadMaxFrame) { why = "frame_length must be 1 .. 4096"; return false; }
    if (framing != DSP_FRAMING_COMPLETE && framing != DSP_FRAMING_STREAM && framing != DSP_FRAMING_CENTER) { why = "framing must be a DSP_FRAMING_* value"; return false; }
    if (framing == DSP_FRAMING_CENTER && (frame_length & 1)) { why = "DSP_FRAMING_CENTER needs an even frame_length"; return false; }
    if (framing == DSP_FRAMING_STREAM && hop > frame_length) { why = "DSP_FRAMING_STREAM needs hop_length <= frame_length"; return false; }
    geo.lead = framing == DSP_FRAMING_COMPLETE ? 0 : framing == DSP_FRAMING_STREAM ? frame_length - hop : frame_length / 2;
    geo.g = std::gcd(hop, frame_length);
    if (geo.lead) geo.g = std::gcd(geo.g, geo.lead);
    geo.m = frame_length / geo.g;
    if (geo.m > kVadMaxSubBlocks) {
        why = "frame_length / gcd(hop_length, frame_length, lead) must be <= 64 sub-blocks per frame, got " + std::to_string(geo.m);
        return false;
    }
    const int quads = (geo.g + 3) / 4;
    geo.lanes = 1;
    while (geo.lanes < quads && geo.lanes < 64) geo.lanes *= 2;
    geo.stride = (int)std::min<long>(hop / geo.g, geo.m);
    geo.chunk_rows = std::min(kVadTileRows, (kVadSlots - geo.m) / geo.stride + 1);
    return true;
}

inline long vad_tiles(long rows) { return ceil_div(rows, kVadTileRows); }

// what the decision leaves per tile of a clip for the clip's record
struct VadTile {
    double sum;                       // of the tile's finite powers, over the 256-leaf halving tree (DSP_VAD_REF_MEAN)
    int n_finite, n_raw, n_kept;
    int first, last;                  // kept rows of the clip, -1: none in this tile
    int reserved;
};
static_assert(sizeof(VadTile) == 32, "VadTile is 32 bytes");

// The caller's workspace, in this order; `power` last, so that the entries that keep no power need less.
struct VadWorkspace {
    long *so, *fo, *to;               // [n + 1] each, back to back: sample, row and tile offsets, from 0
    unsigned long long *ref_key;      // [n]: the ordered key of the largest finite power, 0: none
    double *level;                    // [n][2]: reference, threshold
    long *counts;                     // [n]: kept rows
    VadTile *tiles;                   // [n + rows / 256 + 1]
    int *sel_count;                   // [rows / 256 + 1]: kept rows per tile of the whole matrix
    long *sel_base;                   // the same, scanned
    double *power;                    // [rows]: dsp_vad_run_ragged_device
};

inline VadWorkspace vad_layout(Carver &cv, long n, long rows, bool with_power)
{
    VadWorkspace w{};
    const size_t n1 = (size_t)n + 1, tiles = (size_t)n + (size_t)(rows / kVadTileRows) + 1, sel = (size_t)(rows / kVadTileRows) + 1;
    w.so = cv.take<long>(3 * n1);      // one block: one copy brings all three
    w.fo = w.so + n1;
    w.to = w.fo + n1;
    w.ref_key = cv.take<unsigned long long>(n1);
    w.level = cv.take<double>(2 * n1);
    w.counts = cv.take<long>(n1);
    w.tiles = cv.take<VadTile>(tiles);
    w.sel_count = cv.take<int>(sel);
    w.sel_base = cv.take<long>(sel);
    if (with_power) w.power = cv.take<double>((size_t)rows + 1);
    return w;
}
inline size_t vad_workspace_bytes(long n, long rows, bool with_power)
{
    Carver cv;
    vad_layout(cv, n, rows, with_power);
    return cv.at;
}
inline VadWorkspace vad_carve(void *base, long n, long rows, bool with_power)
{
    Carver cv{static_cast<char *>(base)};
    return vad_layout(cv, n, rows, with_power);
}

// one call's decision: the config's numbers the kernels read
struct VadDecision {
    int reference;
    double ratio, floor, proportion;
    int context, pad;
};

// d_signal + offsets[0], d_power + frame_offsets[0]: the offsets in the workspace count from 0
hipError_t launch_vad_power(const float *d_signal, const VadWorkspace &ws, long n_clips, long n_tiles, const VadGeometry &geo, int frame_length, int hop,
                            double *d_power, hipStream_t stream);
// the reference level and threshold per clip, flags, levels, tile records, then the clips' records and kept counts (ws.counts)
hipError_t launch_vad_decide(const double *d_power, const VadWorkspace &ws, long n_clips, long n_tiles, const VadDecision &dec, unsigned char *d_flags,
                             float *d_level_db, dsp_vad_clip *d_clips, hipStream_t stream);
// ws.counts[c] = the non-zero flags of clip c
hipError_t launch_rows_count(const unsigned char *d_flags, const VadWorkspace &ws, long n_clips, hipStream_t stream);
// rows [0, n_rows) of d_in and d_flags: the kept ones to d_out[0 .. n_out) in order, d_row_index[k] = row_base + the row (may be NULL)
hipError_t launch_rows_select(const float *d_in, int d, const unsigned char *d_flags, long n_rows, long n_out, long row_base, const VadWorkspace &ws,
                              float *d_out, long *d_row_index, hipStream_t stream);

}  // namespace dsp
