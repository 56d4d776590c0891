// augment_kernels.hpp -- augmentation of raw training clips on the GPU (include/dsp_amd.h dsp_augment_*, dsp_stft_*, dsp_istft_*; DESIGN.md
// 3.23): what the host hands the kernels of augment_kernels.hip, and the library's normal draw (one definition for the host helper
// dsp_augment_normal and for finish_kernel).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "stoptrain_kernels.hpp"

namespace dsp {

constexpr int kAugFft = 2048, kAugHop = 512, kAugBins = 1025, kAugPad = 1024;
constexpr int kAugMaxSamples = 1 << 24;            // a clip holds fewer samples than this: every index inside a clip fits an int
constexpr int kAugPvocBlock = 128;                 // lanes per block of pvoc_kernel: ceil(1025 / 128) = 9 blocks per clip
constexpr int kAugPvocBlocksPerClip = (kAugBins + kAugPvocBlock - 1) / kAugPvocBlock;
constexpr int kAugTile = 1024;                     // output samples per block of the gather and of finish_kernel (256 lanes x 4)

// The tables of the transform, computed in float64 and rounded once (capi_augment.cpp).  All (cos, sin) pairs are exp(-2 pi i x).
struct AugTables {
    float win_half[kAugFft];          // 0.5 x the periodic Hann window (the forward untangle's 1 / 2, exact)
    float win[kAugFft];               // the window itself: the inverse's synthesis window
    float win_sq[kAugFft];            // win[i]^2 rounded to float32: the terms of the overlap-add's normalisation
    float w1024[2][1024];             // W1024^i
    float w2048[2][512];              // W2048^k, k < 512
};

// One clip (or one op) of a launch.  Table [n + 1]: entry n is the sentinel that holds the totals (frame0, tile0).
struct AugSpan {
    long in_off;                      // stft: first sample of the clip in the input; finish: first sample of the source
    long frame0;                      // first row of the spectrum this launch reads (stft: writes); istft: also of the frame workspace
    long out_off;                     // pvoc: first row of the spectrum written; gather / finish: first output sample
    long tile0;                       // gather / finish: the first block of this entry
    double rate;                      // pvoc
    unsigned long long key;           // finish: the stream of the draws
    int n;                            // stft: samples of the clip; gather: length; finish: samples of the source
    int frames;                       // rows read (stft: written)
    int frames_out;                   // pvoc: rows written
    int n_out;                        // finish: samples written
    float sigma;                      // finish
    int src;                          // finish: which source buffer in_off counts in (0: the caller's input, 1 / 2: the handle's workspaces)
};
static_assert(sizeof(AugSpan) == 72, "AugSpan travels as bytes");

// ---- the library's normal draw: Box-Muller on one 64-bit draw per pair of samples ----------------------------------------------------
// d = stop_train_draw(seed, key, j): u1 = ((d >> 40) + 1) 2^-24 in (0, 1], u2 = ((d >> 16) & 0xFFFFFF) 2^-24 in [0, 1);
// samples 2 j and 2 j + 1 are sqrt(-2 ln u1) cos(2 pi u2) and sqrt(-2 ln u1) sin(2 pi u2).
__host__ __device__ inline void augment_uniforms(uint64_t seed, uint64_t key, uint64_t j, uint32_t &a, uint32_t &b)
{
    const uint64_t d = stop_train_draw(seed, key, j);
    a = (uint32_t)(d >> 40) + 1u;                  // 1 .. 2^24
    b = (uint32_t)(d >> 16) & 0xFFFFFFu;           // 0 .. 2^24 - 1
}

hipError_t launch_stft2048(const float *in, const AugSpan *spans, long n_clips, long n_frames, int reflect, const AugTables *tables, float2 *spec,
                           hipStream_t stream);
hipError_t launch_pvoc(const float2 *spec, const AugSpan *spans, long n_clips, float2 *spec_out, hipStream_t stream);
hipError_t launch_istft2048(const float2 *spec, const AugSpan *spans, long n_clips, long n_frames, long n_tiles, const AugTables *tables, float *frames,
                            float *out, hipStream_t stream);
hipError_t launch_augment_finish(const float *const src[3], const AugSpan *spans, long n_ops, long n_tiles, unsigned long long seed, float *out, hipStream_t stream);

}  // namespace dsp
