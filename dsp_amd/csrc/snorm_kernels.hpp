// snorm_kernels.hpp -- cohort normalisation of speaker scores on the GPU (include/dsp_amd.h dsp_cohort_stats_device,
// dsp_score_normalize_device): the limits the C ABI checks, the constants that pick a kernel form, and what
// capi_snorm.cpp hands the kernels of snorm_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/dsp_amd.h"
#include "score_matrix.hpp"

namespace dsp {

constexpr long kSnormMaxLength = 1L << 22;                   // values of one cohort vector (the reduced axis)
constexpr long kSnormMaxVectors = 1L << 30;                  // records of one call; rows and columns of a score matrix
constexpr int kSnormMaxTopK = 1 << 22;
// the tree of the float64 sums: chunks of kSnormChunk leaves from index 0, the adjacent pairwise tree inside a chunk (1, 2, 4 ... 2048
// apart, absent leaves +0.0), the chunks added in ascending order
constexpr int kSnormChunk = 4096;
// vector form (a block per vector, its lanes along the vector): vectors up to this many values stay in LDS after the first read
// (128 KiB of the CU's 160 KiB); longer ones are read again by every pass
constexpr int kSnormResident = 32 * 1024;
// per column, from this many columns on a block owns kSnormTileColumns adjacent columns and its lanes run across them (every load a
// coalesced row segment); below it every column is a vector of the vector form, its rows spread over the block's lanes
constexpr long kSnormLanesAcrossColumns = 32;
constexpr int kSnormTileColumns = 64;
constexpr int kSnormTileLds = 256 * kSnormTileColumns * 4;   // the per-column histograms of one digit pass: [256 bins][64 columns]
// apply: below this many columns a thread takes consecutive trials of the flat matrix; from it on a block takes kSnormApplyRows rows of
// 256 adjacent columns, a thread one column whose statistic it reads once
constexpr long kSnormApplyTiled = 64;
constexpr int kSnormApplyRows = 16;

// Everything is enqueued on `stream`; nothing waits for it.  The shapes are those the C ABI has checked (>= 1 vector of 1 .. 2^22
// values; >= 1 row and column of scores).
hipError_t launch_cohort_stats(const float *cohort, long n_rows, long n_cols, int axis, int top_k, dsp_cohort_stat *stats, hipStream_t stream);
hipError_t launch_score_normalize(const float *scores, long n_rows, long n_cols, const dsp_cohort_stat *row_stats, const dsp_cohort_stat *col_stats, int mode,
                                  double std_floor, float *out, hipStream_t stream);

}  // namespace dsp
