// enroll_kernels.hpp -- sliding CMVN of a ragged MFCC matrix and MAP enrolment of speakers against a float UBM (include/dsp_amd.h dsp_cmvn_*,
// dsp_speaker_enroll*): what the host code of capi_enroll.cpp hands the kernels of enroll_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "gmm_model.hpp"

namespace dsp {

// one recording (CMVN) or speaker (enrolment) of a batch: its first row in the matrix, its row count, and the first of its units -- tiles
// of kCmvnTileRows rows, chunks of kEnrollChunkRows rows -- in the launch's numbering (the host counts: nothing is divided per block)
struct RowSpan {
    long row0;
    long unit0;
    long n;
};
static_assert(sizeof(RowSpan) == 24, "three 8-byte words");

// CMVN: a block normalises kCmvnTileRows consecutive rows of one recording from an LDS image of those rows and `half` rows each side.
// The widest image, window 2048 at d = kGmmMaxD = 16, is (64 + 2048) * 16 * 4 = 135 168 bytes of rows plus 16 for the source's alignment shift:
// 135 184 of the CU's 160 KiB.
constexpr int kCmvnTileRows = 64;
constexpr int kCmvnMaxWindow = 2048;

// Enrolment: a speaker's rows are cut into chunks of kEnrollChunkRows -- chunk c = rows [c C, min(n, (c + 1) C)), a function of the
// speaker's own row count alone.  Chunk partials: [k][d + 1] floats (N_k, F_k[0..d)) and the chunk's sum of ll behind them.
constexpr int kEnrollChunkRows = 256;
inline size_t enroll_partial_floats(int k, int d) { return (size_t)k * (d + 1) + 1; }

// on the current device, once before the first launch_cmvn there (dsp_cmvn_create): lets the kernel ask for LDS images above 64 KiB
hipError_t prepare_cmvn();

// y rows of recordings d_spans[n_rec] (units = tiles), total_tiles > 0; window in 2 .. kCmvnMaxWindow, d in 1 .. 16
hipError_t launch_cmvn(const float *d_in, const RowSpan *d_spans, long n_rec, long total_tiles, int d, int window, float *d_out, hipStream_t stream);

// statistics of every chunk into d_partials[total_chunks][enroll_partial_floats], then one block per speaker: chunks summed in ascending
// order in float64, the MAP update, Q6, the saturation count and the ll mean.  map_fixed: alpha_k = param, else alpha_k = N'_k / (N'_k + param).
// Any output may be NULL.
hipError_t launch_enroll(const float *d_feats, const RowSpan *d_spans, long n_speakers, long total_chunks, const GmmModel &ubm, float *d_partials,
                         int map_fixed, float param, float *d_means, int8_t *d_means_q6, float *d_counts, float *d_ll_mean, int *d_saturated,
                         hipStream_t stream);

}  // namespace dsp
