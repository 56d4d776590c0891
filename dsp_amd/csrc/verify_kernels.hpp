// verify_kernels.hpp -- float log-sum-exp scoring of every clip of a ragged matrix against a UBM and S enrolled speakers (include/dsp_amd.h
// dsp_speaker_verif*) and of every sliding window of long recordings (dsp_speaker_float_scan_device): what
// the host code of capi_verify.cpp hands the kernels of verify_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include "enroll_kernels.hpp"
#include "gmm_model.hpp"

namespace dsp {

// A block takes one chunk of kVerifyChunkRows rows of one clip -- a row per lane, a tile of kVerifyTileRows rows per wave -- and one tile
// of kVerifySpeakerTile speakers; the block of speaker tile 0 also takes the UBM, in front of its speakers.
constexpr int kVerifyChunkRows = 256;
constexpr int kVerifyTileRows = 64;
constexpr int kVerifySpeakerTile = 16;
constexpr int kVerifyTilesPerChunk = kVerifyChunkRows / kVerifyTileRows;
constexpr long kVerifyMaxSpeakers = 1L << 19;        // speaker tiles are the grid's y
static_assert(kVerifyChunkRows == kEnrollChunkRows, "the clips' spans count chunks as the enroller's do");
static_assert(kVerifyMaxSpeakers / kVerifySpeakerTile <= 65535, "speaker tiles fit the grid's y");

// Partials: float64 [chunk][tile of the chunk][model], model 0 the UBM and model 1 + s speaker s -- the sum of ll over the tile's rows.
// Tile t of a clip is tile t % 4 of its chunk t / 4, so a clip's tiles lie one behind the other from its first chunk.
inline size_t verify_partial_doubles(long chunks, long n_speakers) { return (size_t)chunks * kVerifyTilesPerChunk * (size_t)(n_speakers + 1); }

// ll sums of every (tile, model) of the clips d_spans[n_clips] (units = chunks, total_chunks > 0) into d_partials, then one block per
// clip: the tiles added in ascending order in float64 and the outputs written at clip index 0 .. n_clips - 1 of each pointer.  d_means:
// [n_speakers][k][d], n_speakers in 1 .. kVerifyMaxSpeakers.  Any output may be NULL.
hipError_t launch_verify(const float *d_feats, const RowSpan *d_spans, long n_clips, long total_chunks, const GmmModel &ubm, const float *d_means,
                         long n_speakers, double *d_partials, float *d_llr, float *d_ll_ubm, float *d_ll_target, int *d_best, float *d_best_llr,
                         hipStream_t stream);

// The window scan (dsp_speaker_float_scan_device), one run of consecutive windows.  A piece is what the run holds of one
// recording: some of its windows, hop_frames apart, and the rows from the first of them to the end of the last.  Both arrays have a
// RowSpan per piece with the same row0, the first row of the piece's first window in d_feats:
//   d_pieces   unit0 = the piece's first chunk of kVerifyChunkRows rows in the run, n = its rows
//   d_wins     unit0 = the piece's first window in the run,                         n = the rows of each of its windows
// Workspace: float32 d_ws[1 + n_speakers][pitch], model 0 the UBM and model 1 + s speaker s, the ll of row `base` + i of d_feats at i;
// every row of every piece lies in [base, base + pitch).  The outputs are written at window index 0 .. windows - 1 of each pointer.
inline size_t verify_scan_floats(long pitch, long n_speakers) { return (size_t)pitch * (size_t)(n_speakers + 1); }
hipError_t launch_verify_scan(const float *d_feats, const RowSpan *d_pieces, const RowSpan *d_wins, long n_pieces, long chunks, long windows, int window_frames,
                              int hop_frames, long base, long pitch, const GmmModel &ubm, const float *d_means, long n_speakers, float *d_ws, float *d_llr,
                              float *d_ll_ubm, float *d_ll_target, int *d_best, float *d_best_llr, hipStream_t stream);

}  // namespace dsp
