// mfcc400_kernel.hip -- the MFCC chain at n_fft = 400: the rows the speaker GMMs are trained and scored on,
// librosa.feature.mfcc(y, sr = 16000, n_mfcc = 13, n_fft = 400, hop_length = 160) of 2fa/audio/speaker/gmm_utils.py:52-58
// (dsp_mfcc_speaker_config).  Same chain as the other kernels, one 64-lane wavefront per frame, four per block:
//
//   load      5 x global_load_dwordx2 on lanes j < 40: z[j + 40 t] = x[2n] + i x[2n+1], x window / 2.  DSP_FRAMING_CENTER: the frame
//             starts n_fft / 2 samples before t hop; positions outside the clip read as 0 and are NOT loaded (in a ragged buffer the
//             neighbouring clip lies there)
//   FFT       400-point real FFT as a 200-point complex Stockham autosort, 200 = 5 x 5 x 8: two radix-5 passes on lanes j < 40, one
//             radix-8 pass on lanes j < 25, through an unpadded 201 x float2 per-wave LDS image (tools/lds_banks_400.py: 90 LDS cycles
//             per frame, 10 of them conflicts, all on pass 1's stores); every twiddle is a per-lane table entry held in registers
//   untangle  bins k = l + 64 t < 100 with 200 - k, bin 100 alone; power spectrum P[0..200] to LDS (over the image)
//   mel       lanes m and m + 64 walk filter m's run of non-zero weights in ascending bins (weights from a block-shared LDS copy);
//             an empty filter (HTK scale at 128 filters has four) yields 0, i.e. the amin floor
//   log       per-frame reference = max, or librosa's power_to_db(ref = 1) with the clip-wide top_db floor in two passes
//             (capi.cpp two_pass_floor), as mfcc2048_kernel.hip
//   DCT-II    two lanes per coefficient (<= 32 coefficients), halves of the log-mel vector each, rows from a block-shared LDS copy
//
// A row depends on its own 400 samples (and, under DSP_LOG_GLOBAL_REF1, on its clip's floor): not on the grid, the chunk or its
// neighbours.  This is the plain form: 24 (FFT passes 0, 1) and 39 (pass 2) lanes idle; a register-resident or two-frame form is
// not built.
#include <hip/hip_runtime.h>

#include "mfcc_device.hpp"
#include "tables.hpp"

namespace dsp {

namespace {

constexpr int R_ZBUF = 0;                          // 201 x float2 image (Z[200] = Z[0]), natural index; later P[0..200]
constexpr int R_LMEL = 208 * 8;                    // 128 log-mel values
constexpr int R_WAVE_BYTES = R_LMEL + 128 * 4;
static_assert(R_WAVE_BYTES % 16 == 0, "keep the carve 16-byte aligned");
constexpr int R_MELW = 4 * R_WAVE_BYTES;           // block-shared: the filterbank's non-zero weights, filter after filter
constexpr int R_DCT = R_MELW + k400MaxWeights * 4; // block-shared: dct_t[i][lane], i < ceil(n_mels / 2); 256 B per row, added by the launcher

// forward 5-point DFT in place: v[q] = sum_t v[t] exp(-2 pi i q t / 5)
__device__ __forceinline__ void radix5(c32 (&v)[8])
{
    constexpr float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f;       // cos(2 pi / 5), cos(4 pi / 5)
    constexpr float S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;        // sin(2 pi / 5), sin(4 pi / 5)
    const c32 a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]);
    const c32 b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
    const c32 m1 = {v[0].x + C1 * a1.x + C2 * a2.x, v[0].y + C1 * a1.y + C2 * a2.y};
    const c32 m2 = {v[0].x + C2 * a1.x + C1 * a2.x, v[0].y + C2 * a1.y + C1 * a2.y};
    const c32 n1 = {S1 * b1.x + S2 * b2.x, S1 * b1.y + S2 * b2.y};
    const c32 n2 = {S2 * b1.x - S1 * b2.x, S2 * b1.y - S1 * b2.y};
    v[0] = {v[0].x + a1.x + a2.x, v[0].y + a1.y + a2.y};
    v[1] = cadd(m1, cmul_mi(n1));
    v[4] = csub(m1, cmul_mi(n1));
    v[2] = cadd(m2, cmul_mi(n2));
    v[3] = csub(m2, cmul_mi(n2));
}

// forward 8-point DFT in place, natural order in and out (two radix-4 butterflies and W8)
__device__ __forceinline__ void radix8(c32 (&v)[8])
{
    c32 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
    radix4(e);
    radix4(o);
    constexpr float R2 = 0.70710678118654752f;
    const c32 t1 = {(o[1].x + o[1].y) * R2, (o[1].y - o[1].x) * R2};        // W8^1 = (1 - i) / sqrt 2
    const c32 t2 = cmul_mi(o[2]);                                            // W8^2 = -i
    const c32 t3 = {(o[3].y - o[3].x) * R2, -(o[3].x + o[3].y) * R2};       // W8^3 = (-1 - i) / sqrt 2
    v[0] = cadd(e[0], o[0]); v[4] = csub(e[0], o[0]);
    v[1] = cadd(e[1], t1);   v[5] = csub(e[1], t1);
    v[2] = cadd(e[2], t2);   v[6] = csub(e[2], t2);
    v[3] = cadd(e[3], t3);   v[7] = csub(e[3], t3);
}

}  // namespace

// CLIPS: frames overlap inside clips of one length (WaveCursor); RAGGED (CLIPS): clips of different lengths, frame g of the batch to
// out[g], clip, t and samples from args.spans (RaggedCursor)
template <bool CLIPS, bool RAGGED>
__global__ __launch_bounds__(256) void mfcc400_kernel(const Mfcc512Args args, const Tables400 *__restrict__ T)
{
    static_assert(!RAGGED || CLIPS, "ragged batches: clip mode");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *wl = smem + wib * R_WAVE_BYTES;
    float2 *zbuf = reinterpret_cast<float2 *>(wl + R_ZBUF);
    float *pbuf = reinterpret_cast<float *>(wl + R_ZBUF);
    float *lmel = reinterpret_cast<float *>(wl + R_LMEL);
    float *melw = reinterpret_cast<float *>(smem + R_MELW);
    float *dct_t = reinterpret_cast<float *>(smem + R_DCT);
    const int n_mels = args.n_mels, n_mfcc = args.n_mfcc;
    const int half = (n_mels + 1) / 2;                   // log-mels per DCT lane
    for (int i = threadIdx.x; i < T->n_weights; i += 256) melw[i] = T->mel_w[i];
    for (int i = threadIdx.x; i < half * 64; i += 256) dct_t[i] = (&T->dct_t[0][0])[i];
    __syncthreads();

    // this lane's constants, in registers across the frame loop
    const int j5 = lane < 40 ? lane : 39, j8 = lane < 25 ? lane : 24;       // idle lanes read what a live lane reads and store nothing
    const bool on5 = lane < 40, on8 = lane < 25;
    float win[10];
    c32 tw1[4], tw2[7], twu[2];
#pragma unroll
    for (int a = 0; a < 10; ++a) win[a] = T->win[a][lane];
#pragma unroll
    for (int q = 0; q < 4; ++q) tw1[q] = {T->tw1[2 * q][lane], T->tw1[2 * q + 1][lane]};
#pragma unroll
    for (int q = 0; q < 7; ++q) tw2[q] = {T->tw2[2 * q][lane], T->tw2[2 * q + 1][lane]};
#pragma unroll
    for (int t = 0; t < 2; ++t) twu[t] = {T->twu[2 * t][lane], T->twu[2 * t + 1][lane]};
    int mel_lo[2], mel_len[2], mel_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = lane + 64 * i;
        mel_lo[i] = m < n_mels ? T->mel_lo[m] : 0;
        mel_len[i] = m < n_mels ? T->mel_len[m] : 0;
        mel_off[i] = m < n_mels ? T->mel_off[m] : 0;
    }

    const long wave = (long)blockIdx.x * 4 + wib;
    const long n_waves = (long)gridDim.x * 4;
    const unsigned amin_u = __float_as_uint(args.amin);
    const float neg_top_db = -args.top_db;

    std::conditional_t<RAGGED, RaggedCursor, WaveCursor<CLIPS>> cur;
    if constexpr (RAGGED) cur.init(wave, n_waves, args.chunk, args.n_frames, args.hop, args.spans, args.n_clips);
    else cur.init(wave, n_waves, args.chunk, args.n_frames, args.frames_per_clip, CLIPS ? args.hop : k400Fft, args.clip_stride);

    while (cur.valid()) {
        const long f = cur.f, clip_f = cur.clip;
        (void)clip_f;
        // ---- load + window: v[t] = z[lane + 40 t] ---------------------------------------------------------------------------
        // samples [lo_i, hi_i) of the frame exist; the rest reads as zero.  Complete and independent frames: [0, 400).
        long src = cur.off;
        int lo_i = 0, hi_i = k400Fft;
        if constexpr (CLIPS) {
            if (args.center_framing) {
                const int start = cur.t * args.hop - k400Fft / 2;        // first sample of the frame inside its clip (even; < 0: padding)
                src -= k400Fft / 2;                                       // cur.off = clip_off + t * hop
                lo_i = start < 0 ? -start : 0;
                int n_clip = args.samples_per_clip;                       // ragged batches: the clip's own length
                if constexpr (RAGGED) n_clip = cur.n_samples;
                hi_i = min(k400Fft, n_clip - start);
            }
        }
        c32 v[8];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int i = 2 * (lane + 40 * t);
            const float *p = static_cast<const float *>(args.in) + src + i;
            float x0 = 0.0f, x1 = 0.0f;
            if (on5 && i >= lo_i && i + 1 < hi_i) {                      // lo_i is even: a pair never straddles it
                const f2v x = CLIPS ? *reinterpret_cast<const f2v *>(p) : __builtin_nontemporal_load(reinterpret_cast<const f2v *>(p));
                x0 = x.x; x1 = x.y;                                      // (clips re-read samples: cacheable)
            } else if (on5 && i >= lo_i && i < hi_i) {
                x0 = *p;
            }
            v[t] = {x0 * win[2 * t], x1 * win[2 * t + 1]};
        }
        cur.next();

        // ---- 200-point complex FFT: Stockham autosort as 5 x 5 x 8, three passes through the wave's LDS image -------------------
        // pass with Ns points done, radix R, butterfly j < 200 / R: k = j % Ns, inputs x[j + (200 / R) t] W_{R Ns}^(t k), outputs
        // y[(j - k) R + k + q Ns]
        // pass 0: R = 5, Ns = 1: butterfly j = lane takes the 5 points this lane loaded, no twiddles
        radix5(v);
        if (on5) {
#pragma unroll
            for (int q = 0; q < 5; ++q) zbuf[5 * lane + q] = make_float2(v[q].x, v[q].y);
        }
        wave_lds_sync();
        // pass 1: R = 5, Ns = 5: k = lane % 5, twiddles W25^(t k)
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const float2 x = zbuf[j5 + 40 * t];
            v[t] = {x.x, x.y};
        }
        wave_lds_sync();
#pragma unroll
        for (int t = 1; t < 5; ++t) v[t] = cmul(v[t], tw1[t - 1]);
        radix5(v);
        if (on5) {
            const int k = lane % 5;
            const int base = 5 * (lane - k) + k;
#pragma unroll
            for (int q = 0; q < 5; ++q) zbuf[base + 5 * q] = make_float2(v[q].x, v[q].y);
        }
        wave_lds_sync();
        // pass 2: R = 8, Ns = 25: k = j = lane, twiddles W200^(t k), outputs y[k + 25 q]: natural order
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float2 x = zbuf[j8 + 25 * t];
            v[t] = {x.x, x.y};
        }
        wave_lds_sync();
#pragma unroll
        for (int t = 1; t < 8; ++t) v[t] = cmul(v[t], tw2[t - 1]);
        radix8(v);
        if (on8) {
#pragma unroll
            for (int q = 0; q < 8; ++q) zbuf[lane + 25 * q] = make_float2(v[q].x, v[q].y);
            if (lane == 0) zbuf[200] = make_float2(v[0].x, v[0].y);      // Z[200] = Z[0] for the pairing below
        }
        wave_lds_sync();

        // ---- untangle: bins k = l + 64 t < 100 with 200 - k; bin 100 alone ------------------------------------------------------
        float P[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = lane + 64 * t < 100 ? lane + 64 * t : 0;
            const float2 a = zbuf[k], b = zbuf[200 - k];
            const c32 E = {a.x + b.x, a.y - b.y};
            const c32 O = {a.x - b.x, a.y + b.y};
            const c32 Tw = cmul(O, twu[t]);
            const float xr = E.x + Tw.y, xi = E.y - Tw.x;
            const float mr = E.x - Tw.y, mi = E.y + Tw.x;
            P[2 * t] = xr * xr + xi * xi;
            P[2 * t + 1] = mr * mr + mi * mi;
        }
        const float2 zm = zbuf[100];
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = lane + 64 * t;
            if (k < 100) {
                pbuf[k] = P[2 * t];
                pbuf[200 - k] = P[2 * t + 1];
            }
        }
        if (lane == 0) pbuf[100] = 4.0f * (zm.x * zm.x + zm.y * zm.y);
        wave_lds_sync();

        // ---- mel: lane m (and m + 64) walks filter m's run of weights in ascending bins ---------------------------------------
        float e[2] = {0.0f, 0.0f};
        float emax = 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i == 1 && n_mels <= 64) break;
            const float *w = melw + mel_off[i], *pw = pbuf + mel_lo[i];
            float acc = 0.0f;
            for (int k = 0; k < mel_len[i]; ++k) acc = fmaf(w[k], pw[k], acc);
            e[i] = acc;
            emax = fmaxf(emax, acc);
        }
        // ---- 10 log10 -----------------------------------------------------------------------------------------------------------
        const float ref = __uint_as_float(max(__float_as_uint(wave_max_nonneg(emax)), amin_u));
        if (args.log_mode != 0) {
            // librosa power_to_db(ref = 1.0, top_db below the CLIP's maximum): same two passes as the 512- and 2048-point kernels
            const float k10 = 3.01029995663981195f;
            const float top_db_val = k10 * __builtin_amdgcn_logf(ref);          // this frame's maximum in dB
            if (args.frame_max != nullptr) {                                    // pass 1: only the frame maximum
                if (lane == 0) args.frame_max[f] = top_db_val;
                wave_lds_sync();
                continue;
            }
            const float floor_db = args.clip_floor ? args.clip_floor[clip_f] : top_db_val + neg_top_db;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float ec = __uint_as_float(max(__float_as_uint(e[i]), amin_u));
                const float db = fmaxf(k10 * __builtin_amdgcn_logf(ec), floor_db);
                lmel[lane + 64 * i] = (lane + 64 * i < n_mels) ? db : 0.0f;
            }
        } else {
            // per-frame reference (mfcc.c:169-206), one log of the ratio
            const float inv = __builtin_amdgcn_rcpf(ref);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float ec = __uint_as_float(max(__float_as_uint(e[i]), amin_u));
                float db = 3.01029995663981195f * __builtin_amdgcn_logf(ec * inv);
                db = __builtin_amdgcn_fmed3f(db, neg_top_db, 0.0f);
                lmel[lane + 64 * i] = (lane + 64 * i < n_mels) ? db : 0.0f;          // 128 slots: the DCT may read up to 2 half <= n_mels + 1
            }
        }
        wave_lds_sync();

        // ---- DCT-II: lane 2 c + h dots log-mels [h half, h half + half) with its column of the LDS copy of dct_t -------------
        {
            const int c = lane >> 1, h = lane & 1;
            const float *lm = lmel + h * half;
            float acc = 0.0f;
#pragma unroll 4
            for (int m = 0; m < half; ++m) acc = fmaf(dct_t[m * 64 + lane], lm[m], acc);     // rows past n_mels / n_mfcc hold 0
            acc += dpp<DPP_QUAD_1032>(acc);
            if (h == 0 && c < n_mfcc) args.out[f * n_mfcc + c] = acc;
        }
        wave_lds_sync();
    }
}

static size_t lds_bytes_400(int n_mels) { return (size_t)R_DCT + (size_t)((n_mels + 1) / 2) * 256; }

hipError_t launch_mfcc400(const Mfcc512Args &args, const Tables400 *tables, int blocks, hipStream_t stream)
{
    const bool clips = args.frames_per_clip > 0 || args.spans;
    if (args.in_kind != 0 || args.frame_len != k400Fft || args.n_mels < 1 || args.n_mels > k400MaxMels || args.n_mfcc < 1 ||
        args.n_mfcc > k400MaxMfcc || (args.log_mode != 0 && args.log_mode != 1) || args.spectrum != 0 || args.stream_framing != 0)
        return hipErrorInvalidConfiguration;
    if (args.center_framing && (!clips || (args.samples_per_clip <= 0 && !args.spans))) return hipErrorInvalidConfiguration;      // (ragged: lengths in the spans)
    const dim3 g(blocks), b(256);
    const size_t lds = lds_bytes_400(args.n_mels);
    if (args.spans) {
        if (args.n_clips <= 0) return hipErrorInvalidConfiguration;
        hipLaunchKernelGGL((mfcc400_kernel<true, true>), g, b, lds, stream, args, tables);
    } else if (clips) {
        hipLaunchKernelGGL((mfcc400_kernel<true, false>), g, b, lds, stream, args, tables);
    } else {
        hipLaunchKernelGGL((mfcc400_kernel<false, false>), g, b, lds, stream, args, tables);
    }
    return hipGetLastError();
}

int mfcc400_blocks_per_cu(int n_mels)
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mfcc400_kernel<true, false>, 256, lds_bytes_400(n_mels));
    return e == hipSuccess && n > 0 ? n : 2;
}

}  // namespace dsp
