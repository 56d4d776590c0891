// augment_kernels.hip -- augmentation of raw training clips (cepstrum/train.py:25-36, 52-56: time stretch, pitch shift, additive noise)
// for a ragged batch in HBM, and the complex STFT / inverse STFT it is made of (include/dsp_amd.h dsp_augment_*).
// n_fft 2048, hop 512, periodic Hann, 1025 bins.  The algorithm is librosa's (stft / phase_vocoder / istft), restated from its published
// form: librosa is not a pinned dependency of the reference, and parity with its own numbers is UNPINNED.
//
//   stft2048_kernel    one frame per 64-lane wavefront: the centred frame is read with the reflect / zero padding as index arithmetic,
//                      windowed, packed z[n] = x[2n] + i x[2n+1] and transformed as a 1024-point complex Stockham autosort in three
//                      passes (16 x 16 x 4) through a padded per-wave LDS image, then untangled to bins 0 .. 1024
//   pvoc_kernel        one lane per (clip, bin), bins across lanes: the lane walks the output frames in order with the phase
//                      accumulator in float64, (|D|, angle) of columns i and i + 1 in registers
//   istft2048_kernel   one frame per wavefront: bins 0 .. 1024 -> the packed spectrum -> the same transform, conjugated -> the frame times
//                      the window into a workspace; istft_gather_kernel then sums every output sample's (at most four) frames and
//                      squared window values in ascending frame order and divides (a gather: no atomics, the same bits every time)
//   finish_kernel      out = (source or 0 past its end) + sigma x the library's normal draw: the tail of every operation
//
// The radix-16 butterfly is a copy of mfcc2048_kernel.hip's: that kernel is tuned on its own and is not touched from here.  Shared with
// the MFCC kernels: c32, cmul, cmul_mi, radix4 and wave_lds_sync of mfcc_device.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "augment_kernels.hpp"
#include "mfcc_device.hpp"

namespace dsp {

namespace {

constexpr int A_WAVE_BYTES = 1092 * 8;             // 1025 x float2 image, one float2 of padding every 16
constexpr int A_W1024 = 4 * A_WAVE_BYTES;          // block-shared: W1024^i, i < 1024
constexpr int A_W2048 = A_W1024 + 1024 * 8;        // block-shared: W2048^k, k < 512
constexpr int A_TW1 = A_W2048 + 512 * 8;           // block-shared: pass 1's twiddles W_256^(t k) at [t - 1][k]
constexpr int A_BLOCK_BYTES = A_TW1 + 15 * 16 * 8;
static_assert(A_WAVE_BYTES % 16 == 0 && A_BLOCK_BYTES % 16 == 0, "keep the carve 16-byte aligned");
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kPiD = 3.14159265358979323846;

__device__ __forceinline__ constexpr int ZI(int i) { return i + (i >> 4); }
__device__ __forceinline__ constexpr int r16_out(int p) { return (p >> 2) + 4 * (p & 3); }

// forward 16-point DFT in place as 4 x 4: position p = 4 q1 + q2 ends up holding X[q1 + 4 q2] = X[r16_out(p)]
__device__ __forceinline__ void radix16(c32 (&v)[16])
{
#pragma unroll
    for (int t2 = 0; t2 < 4; ++t2) {
        c32 u[4] = {v[t2], v[4 + t2], v[8 + t2], v[12 + t2]};
        radix4(u);
#pragma unroll
        for (int q1 = 0; q1 < 4; ++q1) v[4 * q1 + t2] = u[q1];
    }
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    constexpr c32 W1 = {C1, -S1}, W2 = {R2, -R2}, W3 = {S1, -C1}, W6 = {-R2, -R2}, W9 = {-C1, S1};
    v[4 * 1 + 1] = cmul(v[4 * 1 + 1], W1); v[4 * 1 + 2] = cmul(v[4 * 1 + 2], W2); v[4 * 1 + 3] = cmul(v[4 * 1 + 3], W3);
    v[4 * 2 + 1] = cmul(v[4 * 2 + 1], W2); v[4 * 2 + 2] = cmul_mi(v[4 * 2 + 2]);   v[4 * 2 + 3] = cmul(v[4 * 2 + 3], W6);
    v[4 * 3 + 1] = cmul(v[4 * 3 + 1], W3); v[4 * 3 + 2] = cmul(v[4 * 3 + 2], W6); v[4 * 3 + 3] = cmul(v[4 * 3 + 3], W9);
#pragma unroll
    for (int q1 = 0; q1 < 4; ++q1) {
        c32 u[4] = {v[4 * q1], v[4 * q1 + 1], v[4 * q1 + 2], v[4 * q1 + 3]};
        radix4(u);
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) v[4 * q1 + q2] = u[q2];
    }
}

// the block-shared twiddle tables (every lane of the block; a __syncthreads() follows at the caller)
__device__ __forceinline__ void stage_twiddles(char *smem, const AugTables *G)
{
    float2 *w1024 = reinterpret_cast<float2 *>(smem + A_W1024);
    float2 *w2048 = reinterpret_cast<float2 *>(smem + A_W2048);
    float2 *tw1 = reinterpret_cast<float2 *>(smem + A_TW1);
    for (int i = threadIdx.x; i < 1024; i += 256) w1024[i] = make_float2(G->w1024[0][i], G->w1024[1][i]);
    for (int i = threadIdx.x; i < 512; i += 256) w2048[i] = make_float2(G->w2048[0][i], G->w2048[1][i]);
    if (threadIdx.x < 240) { const int i = 4 * (threadIdx.x / 16 + 1) * (threadIdx.x % 16); tw1[threadIdx.x] = make_float2(G->w1024[0][i], G->w1024[1][i]); }
}

// 1024-point forward complex DFT of v[a] = z[lane + 64 a] by one wavefront: Stockham autosort 16 x 16 x 4 through the wave's padded LDS
// image; the result lies in zbuf in natural order (Z[k] at ZI(k)).  The image is padded by one float2 every 16: the stride-16 stores of
// the radix-16 passes would otherwise all land in one bank pair.
__device__ __forceinline__ void fft1024_wave(c32 (&v)[16], float2 *zbuf, const float2 *tw1, const float2 *w1024, int lane)
{
    radix16(v);                                                   // pass 0: R = 16, Ns = 1, no twiddles
#pragma unroll
    for (int p = 0; p < 16; ++p) zbuf[ZI(16 * lane + r16_out(p))] = make_float2(v[p].x, v[p].y);
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 16; ++t) {                                // pass 1: R = 16, Ns = 16, twiddles W_256^(t k), k = lane % 16
        const float2 x = zbuf[ZI(lane + 64 * t)];
        v[t] = {x.x, x.y};
    }
    wave_lds_sync();
    const int k = lane & 15;
#pragma unroll
    for (int t = 1; t < 16; ++t) {
        const float2 w = tw1[16 * (t - 1) + k];
        v[t] = cmul(v[t], c32{w.x, w.y});
    }
    radix16(v);
    const int base = 16 * (lane - k) + k;
#pragma unroll
    for (int p = 0; p < 16; ++p) zbuf[ZI(base + 16 * r16_out(p))] = make_float2(v[p].x, v[p].y);
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 4; ++m)                                   // pass 2: R = 4, Ns = 256: four butterflies per lane, natural order out
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float2 x = zbuf[ZI(lane + 64 * m + 256 * t)];
            v[m + 4 * t] = {x.x, x.y};
        }
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int j = lane + 64 * m;
        c32 u[4] = {v[m], v[m + 4], v[m + 8], v[m + 12]};
#pragma unroll
        for (int t = 1; t < 4; ++t) {
            const float2 w = w1024[(t * j) & 1023];
            u[t] = cmul(u[t], c32{w.x, w.y});
        }
        radix4(u);
#pragma unroll
        for (int q = 0; q < 4; ++q) zbuf[ZI(j + 256 * q)] = make_float2(u[q].x, u[q].y);
    }
    wave_lds_sync();
}

// the entry of a span table whose rows / tiles hold `g`: the largest c with first(c) <= g (entry n is the sentinel with the total)
// (span_find.hpp's owner_of finds the same entry in long; this int form stays because joining it changes the kernels' instructions, which nobody has timed)
template <class First>
__device__ __forceinline__ int span_of(long g, int n, First first)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first(mid) <= g) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

// ---- STFT ---------------------------------------------------------------------------------------------------------------------------
// frame t of a clip of n samples = samples [512 t - 1024, 512 t + 1024) of the clip; outside [0, n): REFLECT np.pad(mode="reflect")
// (n >= 1025: one reflection reaches), else zeros.  D[g][k], k = 0 .. 1024, interleaved (re, im), row g = frame0(clip) + t.
template <bool REFLECT>
__global__ __launch_bounds__(256) void stft2048_kernel(const float *__restrict__ in, const AugSpan *__restrict__ spans, int n_clips, long n_frames,
                                                       const AugTables *__restrict__ G, float2 *__restrict__ spec)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *zbuf = reinterpret_cast<float2 *>(smem + wib * A_WAVE_BYTES);
    const float2 *w1024 = reinterpret_cast<const float2 *>(smem + A_W1024);
    const float2 *w2048 = reinterpret_cast<const float2 *>(smem + A_W2048);
    const float2 *tw1 = reinterpret_cast<const float2 *>(smem + A_TW1);
    stage_twiddles(smem, G);
    __syncthreads();

    for (long g = (long)blockIdx.x * 4 + wib; g < n_frames; g += (long)gridDim.x * 4) {
        const int c = span_of(g, n_clips, [&](int i) { return spans[i].frame0; });
        const int n = spans[c].n;
        const int base = kAugHop * (int)(g - spans[c].frame0) - kAugPad;      // first sample of the frame inside its clip
        const float *x = in + spans[c].in_off;
        const bool interior = base >= 0 && base + kAugFft <= n;
        const bool pairs = interior && ((reinterpret_cast<uintptr_t>(x + base) & 7) == 0);
        c32 v[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            const int i = 2 * (lane + 64 * a);
            float x0, x1;
            if (pairs) {
                const float2 p = *reinterpret_cast<const float2 *>(x + base + i);
                x0 = p.x; x1 = p.y;
            } else {
                int j0 = base + i, j1 = base + i + 1;
                if (REFLECT) {
                    j0 = j0 < 0 ? -j0 : (j0 >= n ? 2 * (n - 1) - j0 : j0);
                    j1 = j1 < 0 ? -j1 : (j1 >= n ? 2 * (n - 1) - j1 : j1);
                    x0 = x[j0]; x1 = x[j1];
                } else {
                    x0 = j0 >= 0 && j0 < n ? x[j0] : 0.0f;
                    x1 = j1 >= 0 && j1 < n ? x[j1] : 0.0f;
                }
            }
            const float2 w = *reinterpret_cast<const float2 *>(&G->win_half[i]);
            v[a] = {x0 * w.x, x1 * w.y};
        }
        fft1024_wave(v, zbuf, tw1, w1024, lane);
        if (lane == 0) zbuf[ZI(1024)] = zbuf[ZI(0)];         // Z[1024] = Z[0] for the pairing below
        wave_lds_sync();
        // untangle: X[k] = E - i W2048^k O, X[1024 - k] = conj(E) - i conj(W2048^k O), E = Z[k] + conj(Z[1024 - k]), O = Z[k] - conj(Z[1024 - k])
        float2 *row = spec + g * kAugBins;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = lane + 64 * t;
            const float2 a = zbuf[ZI(k)], b = zbuf[ZI(1024 - k)], w = w2048[k];
            const c32 E = {a.x + b.x, a.y - b.y};
            const c32 O = {a.x - b.x, a.y + b.y};
            const c32 Tw = cmul(O, c32{w.x, w.y});
            row[k] = make_float2(E.x + Tw.y, E.y - Tw.x);
            row[1024 - k] = make_float2(E.x - Tw.y, -(E.y + Tw.x));
        }
        if (lane == 0) {
            const float2 zm = zbuf[ZI(512)];
            row[512] = make_float2(2.0f * zm.x, -2.0f * zm.y);
        }
        wave_lds_sync();
    }
}

// ---- phase vocoder ------------------------------------------------------------------------------------------------------------------
// Output frame t of a clip reads columns i = floor(t rate) and i + 1 of its D (columns >= T read as zero):
//   S[t][k] = ((1 - a) |D[i][k]| + a |D[i+1][k]|) exp(j acc_t[k]),  acc_0 = angle(D[0][k]),
//   acc_{t+1} = acc_t + phi_k + wrap(angle(D[i+1][k]) - angle(D[i][k]) - phi_k),  phi_k = pi 512 k / 1024, wrap(d) = d - 2 pi rint(d / 2 pi)
// acc in float64, in frame order (phi_k reaches 1600 rad per step: a float32 accumulator loses the phase within a hundred frames); the
// argument of sin / cos is acc reduced by 2 pi rint(acc / 2 pi) in double, rounded to float32.  angle(0) = 0.
namespace {
struct Polar { float mag, ang; };
__device__ __forceinline__ Polar polar_of(const float2 *col0, int col, int T)
{
    if (col >= T) return {0.0f, 0.0f};
    const float2 z = col0[(long)col * kAugBins];
    return {hypotf(z.x, z.y), (z.x == 0.0f && z.y == 0.0f) ? 0.0f : atan2f(z.y, z.x)};
}
}  // namespace

__global__ __launch_bounds__(kAugPvocBlock) void pvoc_kernel(const float2 *__restrict__ spec, const AugSpan *__restrict__ spans, float2 *__restrict__ out)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x / kAugPvocBlocksPerClip;
    const int k = (blockIdx.x % kAugPvocBlocksPerClip) * kAugPvocBlock + threadIdx.x;
    if (k >= kAugBins) return;
    const int T = spans[c].frames, T_out = spans[c].frames_out;
    const double rate = spans[c].rate;
    const float2 *D = spec + spans[c].frame0 * kAugBins + k;
    float2 *S = out + spans[c].out_off * kAugBins + k;
    const double phi = kPiD * 512.0 * (double)k / 1024.0;
    int ci = 0;                                                   // the column c0 holds; c1 holds ci + 1
    Polar c0 = polar_of(D, 0, T), c1 = polar_of(D, 1, T);
    double acc = (double)c0.ang;
    for (int t = 0; t < T_out; ++t) {
        const double s = (double)t * rate;
        const double fl = floor(s);
        const int i = (int)fl;
        const float al = (float)(s - fl);
        if (i != ci) {                                            // (the same in every lane of the block: one clip, one t)
            if (i == ci + 1) { c0 = c1; c1 = polar_of(D, i + 1, T); }
            else { c0 = polar_of(D, i, T); c1 = polar_of(D, i + 1, T); }
            ci = i;
        }
        const float mag = (1.0f - al) * c0.mag + al * c1.mag;
        const float ph = (float)(acc - kTwoPi * rint(acc / kTwoPi));
        float sn, cs;
        sincosf(ph, &sn, &cs);
        S[(long)t * kAugBins] = make_float2(mag * cs, mag * sn);
        double d = (double)c1.ang - (double)c0.ang - phi;
        d = d - kTwoPi * rint(d / kTwoPi);
        acc = acc + phi + d;
    }
}

// ---- inverse STFT -------------------------------------------------------------------------------------------------------------------
// Frame g: x = irfft(S[g]) (the 1 / 2048 included, Im of bins 0 and 1024 ignored) times the window -> frames[g][0 .. 2048).
// With z[n] = x[2n] + i x[2n+1] and Z its 1024-point DFT: conj(Z[k]) = P - i Q, conj(Z[1024 - k]) = conj(P) - i conj(Q),
// P = conj(X[k]) + X[1024 - k], Q = (conj(X[k]) - X[1024 - k]) W2048^k (both carry the factor 2 of the pairing); z = conj(DFT(conj(Z))) / 1024.
__global__ __launch_bounds__(256) void istft2048_kernel(const float2 *__restrict__ spec, long n_frames, const AugTables *__restrict__ G, float *__restrict__ frames)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *zbuf = reinterpret_cast<float2 *>(smem + wib * A_WAVE_BYTES);
    const float2 *w1024 = reinterpret_cast<const float2 *>(smem + A_W1024);
    const float2 *w2048 = reinterpret_cast<const float2 *>(smem + A_W2048);
    const float2 *tw1 = reinterpret_cast<const float2 *>(smem + A_TW1);
    stage_twiddles(smem, G);
    __syncthreads();

    constexpr float kScale = 1.0f / 2048.0f;                       // a power of two: exact wherever it is applied
    for (long g = (long)blockIdx.x * 4 + wib; g < n_frames; g += (long)gridDim.x * 4) {
        const float2 *row = spec + g * kAugBins;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = lane + 64 * t;
            float2 a = row[k], b = row[1024 - k];
            if (k == 0) { a.y = 0.0f; b.y = 0.0f; }
            const float2 w = w2048[k];
            const c32 P = {(a.x + b.x) * kScale, (b.y - a.y) * kScale};
            const c32 Q = cmul(c32{(a.x - b.x) * kScale, (-a.y - b.y) * kScale}, c32{w.x, w.y});
            zbuf[ZI(k)] = make_float2(P.x + Q.y, P.y - Q.x);
            zbuf[ZI(1024 - k)] = make_float2(P.x - Q.y, -P.y - Q.x);      // (k = 0 lands in the image's spare slot 1024, which nothing reads)
        }
        if (lane == 0) {
            const float2 m = row[512];
            zbuf[ZI(512)] = make_float2(2.0f * m.x * kScale, 2.0f * m.y * kScale);
        }
        wave_lds_sync();
        c32 v[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            const float2 z = zbuf[ZI(lane + 64 * a)];
            v[a] = {z.x, z.y};
        }
        wave_lds_sync();
        fft1024_wave(v, zbuf, tw1, w1024, lane);
        float *dst = frames + g * kAugFft;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            const int i = 2 * (lane + 64 * a);
            const float2 y = zbuf[ZI(lane + 64 * a)];
            const float2 w = *reinterpret_cast<const float2 *>(&G->win[i]);
            *reinterpret_cast<float2 *>(dst + i) = make_float2(y.x * w.x, -y.y * w.y);
        }
        wave_lds_sync();
    }
}

// out[s], s < length, of a clip with T frames: p = s + 1024; sum over t = max(0, p / 512 - 3) .. min(T - 1, p / 512), ascending, of
// frames[t][p - 512 t], divided by the sum in the same order of win[p - 512 t]^2 where that exceeds float32's smallest normal.  Samples
// no frame reaches are zeros: the zero fill to `length`.  256 lanes x 4 consecutive samples per block (they share p / 512).
__global__ __launch_bounds__(256) void istft_gather_kernel(const float *__restrict__ frames, const AugSpan *__restrict__ spans, int n_clips,
                                                           const AugTables *__restrict__ G, float *__restrict__ out)
{
#pragma clang fp contract(off)
    const int c = span_of((long)blockIdx.x, n_clips, [&](int i) { return spans[i].tile0; });
    const int length = spans[c].n, T = spans[c].frames;
    const int s0 = (int)((long)blockIdx.x - spans[c].tile0) * kAugTile + 4 * (int)threadIdx.x;
    if (s0 >= length) return;
    const int p = s0 + kAugPad, q = p >> 9;
    const int t_lo = q - 3 > 0 ? q - 3 : 0, t_hi = q < T - 1 ? q : T - 1;
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wss[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float *fr = frames + spans[c].frame0 * kAugFft;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int o = p - kAugHop * t;                              // a multiple of 4 in [0, 2048)
        const float4 f = *reinterpret_cast<const float4 *>(fr + (long)t * kAugFft + o);
        const float4 w = *reinterpret_cast<const float4 *>(&G->win_sq[o]);
        y[0] += f.x; y[1] += f.y; y[2] += f.z; y[3] += f.w;
        wss[0] += w.x; wss[1] += w.y; wss[2] += w.z; wss[3] += w.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (wss[e] > FLT_MIN) y[e] = y[e] / wss[e];
    float *dst = out + spans[c].out_off + s0;
    if (s0 + 4 <= length && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4 *>(dst) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (s0 + e < length) dst[e] = y[e];
    }
}

// ---- the tail of every operation ----------------------------------------------------------------------------------------------------
// out[i] = (i < n ? src[i] : 0) + sigma normal(seed, key, i), i < n_out; sigma == 0: the source's bits (no draw, no addition)
__global__ __launch_bounds__(256) void finish_kernel(const float *__restrict__ src0, const float *__restrict__ src1, const float *__restrict__ src2,
                                                     const AugSpan *__restrict__ spans, int n_ops, unsigned long long seed, float *__restrict__ out)
{
#pragma clang fp contract(off)
    const int c = span_of((long)blockIdx.x, n_ops, [&](int i) { return spans[i].tile0; });
    const int n = spans[c].n, n_out = spans[c].n_out;
    const int s0 = (int)((long)blockIdx.x - spans[c].tile0) * kAugTile + 4 * (int)threadIdx.x;
    if (s0 >= n_out) return;
    const int kind = spans[c].src;
    const float *src = (kind == 0 ? src0 : kind == 1 ? src1 : src2) + spans[c].in_off + s0;
    float v[4];
    if (s0 + 4 <= n && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const float4 f = *reinterpret_cast<const float4 *>(src);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s0 + e < n ? src[e] : 0.0f;
    }
    const float sigma = spans[c].sigma;
    if (sigma > 0.0f) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {                               // samples 2 j and 2 j + 1 share draw j
            uint32_t a, b;
            augment_uniforms(seed, spans[c].key, (uint64_t)(s0 >> 1) + h, a, b);
            const float r = sqrtf(-2.0f * logf((float)a * 0x1p-24f));
            float sn, cs;
            sincosf(6.2831855f * ((float)b * 0x1p-24f), &sn, &cs);
            v[2 * h] = v[2 * h] + sigma * (r * cs);
            v[2 * h + 1] = v[2 * h + 1] + sigma * (r * sn);
        }
    }
    float *dst = out + spans[c].out_off + s0;
    if (s0 + 4 <= n_out && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (s0 + e < n_out) dst[e] = v[e];
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
namespace {
int frame_blocks(long n_frames) { return (int)std::min<long>((n_frames + 3) / 4, 256L * 3); }      // 48 KB of LDS per block: three blocks per CU
}

hipError_t launch_stft2048(const float *in, const AugSpan *spans, long n_clips, long n_frames, int reflect, const AugTables *tables, float2 *spec,
                           hipStream_t stream)
{
    if (n_frames <= 0) return hipSuccess;
    const dim3 g(frame_blocks(n_frames)), b(256);
    if (reflect) hipLaunchKernelGGL(stft2048_kernel<true>, g, b, A_BLOCK_BYTES, stream, in, spans, (int)n_clips, n_frames, tables, spec);
    else hipLaunchKernelGGL(stft2048_kernel<false>, g, b, A_BLOCK_BYTES, stream, in, spans, (int)n_clips, n_frames, tables, spec);
    return hipGetLastError();
}

hipError_t launch_pvoc(const float2 *spec, const AugSpan *spans, long n_clips, float2 *spec_out, hipStream_t stream)
{
    if (n_clips <= 0) return hipSuccess;
    hipLaunchKernelGGL(pvoc_kernel, dim3((unsigned)(n_clips * kAugPvocBlocksPerClip)), dim3(kAugPvocBlock), 0, stream, spec, spans, spec_out);
    return hipGetLastError();
}

hipError_t launch_istft2048(const float2 *spec, const AugSpan *spans, long n_clips, long n_frames, long n_tiles, const AugTables *tables, float *frames,
                            float *out, hipStream_t stream)
{
    if (n_frames > 0) {
        hipLaunchKernelGGL(istft2048_kernel, dim3(frame_blocks(n_frames)), dim3(256), A_BLOCK_BYTES, stream, spec, n_frames, tables, frames);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(istft_gather_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, frames, spans, (int)n_clips, tables, out);
    return hipGetLastError();
}

hipError_t launch_augment_finish(const float *const src[3], const AugSpan *spans, long n_ops, long n_tiles, unsigned long long seed, float *out,
                                 hipStream_t stream)
{
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, src[0], src[1], src[2], spans, (int)n_ops, seed, out);
    return hipGetLastError();
}

}  // namespace dsp
