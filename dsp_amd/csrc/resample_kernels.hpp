// resample_kernels.hpp -- the rational-ratio polyphase FIR resampler (include/dsp_amd.h dsp_resample_*): what the host code
// of capi_resample.cpp hands the kernels of resample_kernels.hip.
#pragma once

#include <hip/hip_runtime_api.h>

namespace dsp {

// one recording of a batch: where it starts in the input (samples per channel) and in the output, its lengths, and the first of its
// tiles in the launch's tile numbering (the host counts; the kernels divide nothing per recording)
struct ResampleSpan {
    long in_off;
    long out_off;
    long tile0;
    long n_out;
    int n;
    int pad_;
};
static_assert(sizeof(ResampleSpan) == 40, "five aligned 8-byte words");

constexpr int kResampleOutputsPerLane = 4;     // outputs k, k + up, k + 2 up, k + 3 up share one polyphase branch: one tap read per four FMAs

// the geometry of one ratio: a function of (up, down) alone, so that no output bit can depend on the batch or the entry point
struct ResampleShape {
    int up, down, half;
    int taps;      // T = ceil((2 half + 1) / up): taps of one polyphase branch
    int row;       // T rounded up to a multiple of 4: floats per branch in the device table (reversed: ascending input sample), zero filled
    int tile;      // consecutive outputs of one recording per block = kResampleOutputsPerLane * up * groups
    int items;     // tile / kResampleOutputsPerLane: lane work items per block
    int span;      // input samples a tile reads (the taps' zero fill included)
    int staged;    // 1: the span is staged in LDS; 0 (a branch too long for it): read from global memory
    int lds_bytes;
};

// in_kind: 0 float samples, 1 / 2 / 3 int16 mono / stereo channel 0 / stereo average (capi_util.hpp pcm16_kind).  Tiles
// [0, total_tiles) of d_spans[n_rec]; d_taps[up][row].  up == down == 1 copies (decodes) without a filter.
hipError_t launch_resample(const void *d_in, int in_kind, const ResampleSpan *d_spans, long n_rec, long total_tiles, const ResampleShape &s,
                           const float *d_taps, float *d_out, hipStream_t stream);

// ---- live streams (include/dsp_amd.h dsp_stream_resample*) ----
// One stream of a push (or of a finish) that emits outputs: k0 .. k0 + n_out - 1 of the stream, written at out_off.  The samples they read
// come from two places: [c0, n0) from the stream's carry, carry_off sample frames into the carry buffer, and [n0, n1) from the chunk,
// chunk_off sample frames into the chunk buffer.  Samples before c0 are read by no output of the span; samples from n1 on have not
// arrived (or, in a finish, never will): both are zeros.
struct StreamResampleSpan {
    long k0;
    long out_off;
    long tile0;
    long n_out;
    long c0, n0, n1;
    long carry_off;
    long chunk_off;
};
static_assert(sizeof(StreamResampleSpan) == 72, "nine aligned 8-byte words");

// Tiles [0, total_tiles) of d_spans[n_spans], every span with n_out >= 1; a staged shape that is not the copy (s.staged, up or down > 1).
// d_carry and d_chunks in the stream's own format (in_kind as above); the kernel only reads them.
hipError_t launch_resample_stream(const void *d_carry, const void *d_chunks, int in_kind, const StreamResampleSpan *d_spans, long n_spans,
                                  long total_tiles, const ResampleShape &s, const float *d_taps, float *d_out, hipStream_t stream);

}  // namespace dsp
