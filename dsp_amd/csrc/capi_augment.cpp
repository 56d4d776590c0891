// capi_augment.cpp -- the C ABI of the clip augmenter (include/dsp_amd.h dsp_augment_*, dsp_stft_*, dsp_istft_*, dsp_time_stretch_*;
// DESIGN.md 3.23): the host rules (frame counts, stretched lengths, the pitch ratio, the draws of the policy), the tables, and the
// entries that put a ragged batch of clips through augment_kernels.hip.  The time stretch IS the STFT entry, the vocoder and the
// inverse STFT entry, one after the other on the handle's workspaces: the pieces tested alone are the pieces that run.
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <utility>

#include "augment_kernels.hpp"
#include "capi_util.hpp"

using dsp::capi_fail;

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kRateMin = 0.125, kRateMax = 8.0;
constexpr int kMaxSteps = 12, kMaxTermCap = 1024;
constexpr unsigned long long kPolicyStream = 0xA000000000000000ull;

int check_rate(double rate)
{
    if (!(std::isfinite(rate) && rate >= kRateMin && rate <= kRateMax)) return capi_fail(DSP_EINVAL, "rate must be finite and in [1/8, 8]");
    return DSP_OK;
}

long stretch_frames(long frames, double rate) { return (long)std::ceil((double)frames / rate); }
long stretch_length(long n, double rate) { return std::max(1L, (long)std::nearbyint((double)n / rate)); }      // (round to nearest, ties to even)

int pitch_ratio(int n_steps, int bins_per_octave, int max_term, int &up, int &down)
{
    if (bins_per_octave < 1) return capi_fail(DSP_EINVAL, "bins_per_octave must be >= 1");
    if (max_term < 1 || max_term > kMaxTermCap) return capi_fail(DSP_EINVAL, "max_term must be 1 .. 1024 (the resampler's cap)");
    const double f = std::pow(2.0, -(double)n_steps / (double)bins_per_octave);
    if (!(f >= kRateMin && f <= kRateMax)) return capi_fail(DSP_EINVAL, "2^(-n_steps / bins_per_octave) must lie in [1/8, 8]");
    double best = INFINITY;
    up = down = 1;
    for (int d = 1; d <= max_term; ++d) {
        const double x = f * d;
        for (long u = (long)std::floor(x); u <= (long)std::floor(x) + 1; ++u) {
            if (u < 1 || u > max_term) continue;
            const double err = std::fabs((double)u / (double)d - f);
            if (err < best) { best = err; up = (int)u; down = d; }      // strictly better only: ties keep the smaller denominator
        }
    }
    return DSP_OK;
}

// what can be said of an op without a handle: its kind and parameters, its clip's index and length (pad_mode < 0: the padding is not known)
int check_op(const dsp_augment_op &op, long j, long n, const long *offsets, int pad_mode, long &len)
{
    const std::string who = "op " + std::to_string(j) + ": ";
    if (op.kind != DSP_AUGMENT_STRETCH && op.kind != DSP_AUGMENT_PITCH && op.kind != DSP_AUGMENT_NOISE)
        return capi_fail(DSP_EINVAL, who + "kind must be DSP_AUGMENT_STRETCH, _PITCH or _NOISE");
    if (op.clip < 0 || op.clip >= n) return capi_fail(DSP_EINVAL, who + "clip " + std::to_string(op.clip) + " is not one of the " + std::to_string(n) + " clips");
    if (!(op.sigma >= 0.0f) || !std::isfinite(op.sigma)) return capi_fail(DSP_EINVAL, who + "sigma must be finite and >= 0");
    len = dsp::ragged_clip_length(offsets, op.clip);
    if (len < 0) return (int)len;
    if (len >= dsp::kAugMaxSamples) return capi_fail(DSP_EINVAL, who + "a clip must be shorter than 2^24 samples");
    if (op.kind == DSP_AUGMENT_NOISE) return DSP_OK;
    if (op.kind == DSP_AUGMENT_STRETCH) {
        if (check_rate(op.rate)) return capi_fail(DSP_EINVAL, who + "rate must be finite and in [1/8, 8]");
    } else if (op.n_steps < -kMaxSteps || op.n_steps > kMaxSteps) {
        return capi_fail(DSP_EINVAL, who + "n_steps must be -12 .. 12");
    }
    if (len < 1) return capi_fail(DSP_EINVAL, who + "a clip to stretch holds at least one sample");
    if (pad_mode == DSP_PAD_REFLECT && len <= dsp::kAugPad) return capi_fail(DSP_EINVAL, who + "reflect padding needs a clip of at least 1025 samples");
    return DSP_OK;
}

int check_clip(long c, long len, int pad_mode)
{
    if (len < 1) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + " holds no sample");
    if (pad_mode == DSP_PAD_REFLECT && len <= dsp::kAugPad) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + ": reflect padding needs at least 1025 samples");
    if (len >= dsp::kAugMaxSamples) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + ": a clip must be shorter than 2^24 samples");
    return DSP_OK;
}

long tiles_of(long samples) { return (samples + dsp::kAugTile - 1) / dsp::kAugTile; }

}  // namespace

struct dsp_augmenter : dsp::Handle {
    int pad_mode = DSP_PAD_REFLECT, max_term = 256;
    dsp::DeviceBuf<dsp::AugTables> tables;
    dsp::DeviceBuf<float> spec, spec_out;      // D and S of a stretch, (re, im) pairs
    dsp::DeviceBuf<float> frames;              // the inverse transform's windowed frames, [rows][2048]
    dsp::DeviceBuf<float> ws_a, ws_b;          // an augment call's stretched clips, and the pitch ops' resampled ones
    dsp::SpanRing ring;
    std::map<std::pair<int, int>, std::unique_ptr<dsp_resampler, dsp::DestroyWith<dsp_resampler_destroy>>> resamplers;      // one per (up, down), owned
};

namespace {

// a span table (entry m: the sentinel) into a leased slot, uploaded
int upload_spans(dsp_augmenter *aug, const std::vector<dsp::AugSpan> &spans, dsp::SpanRing::Lease &slot, hipStream_t st)
{
    const size_t bytes = spans.size() * sizeof(dsp::AugSpan);
    DSP_CAPI_HIP(aug->ring.acquire(bytes, slot));
    std::memcpy(slot.h(), spans.data(), bytes);
    DSP_CAPI_HIP(slot.upload(bytes, st));
    return DSP_OK;
}

// clip c = lens[c] samples at d_in + starts[c] (checked by the caller) -> rows [fo[c], fo[c + 1]) of d_spec
int stft_run(dsp_augmenter *aug, const float *d_in, long m, const long *starts, const long *lens, float *d_spec, std::vector<long> &fo, hipStream_t st)
{
    std::vector<dsp::AugSpan> spans((size_t)m + 1);
    fo.assign((size_t)m + 1, 0);
    for (long c = 0; c < m; ++c) {
        dsp::AugSpan &s = spans[(size_t)c];
        s = dsp::AugSpan{};
        s.in_off = starts[c];
        s.frame0 = fo[(size_t)c];
        s.n = (int)lens[c];
        s.frames = (int)(1 + lens[c] / dsp::kAugHop);
        fo[(size_t)c + 1] = fo[(size_t)c] + s.frames;
    }
    spans[(size_t)m] = dsp::AugSpan{};
    spans[(size_t)m].frame0 = fo[(size_t)m];
    dsp::SpanRing::Lease slot;
    if (const int rc = upload_spans(aug, spans, slot, st)) return rc;
    DSP_CAPI_HIP(dsp::launch_stft2048(d_in, static_cast<const dsp::AugSpan *>(slot.d()), m, fo[(size_t)m], aug->pad_mode == DSP_PAD_REFLECT, aug->tables,
                                      reinterpret_cast<float2 *>(d_spec), st));
    return DSP_OK;
}

// rows [fo[c], fo[c + 1]) of d_spec stretched by rates[c] -> rows [so[c], so[c + 1]) of d_spec_out
int pvoc_run(dsp_augmenter *aug, const float *d_spec, long m, const std::vector<long> &fo, const double *rates, float *d_spec_out, const std::vector<long> &so,
             hipStream_t st)
{
    std::vector<dsp::AugSpan> spans((size_t)m + 1);
    for (long c = 0; c < m; ++c) {
        dsp::AugSpan &s = spans[(size_t)c];
        s = dsp::AugSpan{};
        s.frame0 = fo[(size_t)c];
        s.out_off = so[(size_t)c];
        s.rate = rates[c];
        s.frames = (int)(fo[(size_t)c + 1] - fo[(size_t)c]);
        s.frames_out = (int)(so[(size_t)c + 1] - so[(size_t)c]);
    }
    spans[(size_t)m] = dsp::AugSpan{};
    dsp::SpanRing::Lease slot;
    if (const int rc = upload_spans(aug, spans, slot, st)) return rc;
    DSP_CAPI_HIP(dsp::launch_pvoc(reinterpret_cast<const float2 *>(d_spec), static_cast<const dsp::AugSpan *>(slot.d()), m, reinterpret_cast<float2 *>(d_spec_out), st));
    return DSP_OK;
}

// rows [fo[c], fo[c + 1]) of d_spec -> lengths[c] samples at d_out + out_off[c] (all checked by the caller)
int istft_run(dsp_augmenter *aug, const float *d_spec, long m, const long *fo, const long *lengths, float *d_out, const long *out_off, hipStream_t st)
{
    const long rows0 = fo[0], rows = fo[m] - fo[0];
    std::vector<dsp::AugSpan> spans((size_t)m + 1);
    long tiles = 0;
    for (long c = 0; c < m; ++c) {
        dsp::AugSpan &s = spans[(size_t)c];
        s = dsp::AugSpan{};
        s.frame0 = fo[c] - rows0;
        s.out_off = out_off[c];
        s.tile0 = tiles;
        s.n = (int)lengths[c];
        s.frames = (int)(fo[c + 1] - fo[c]);
        tiles += tiles_of(lengths[c]);
    }
    spans[(size_t)m] = dsp::AugSpan{};
    spans[(size_t)m].frame0 = rows;
    spans[(size_t)m].tile0 = tiles;
    if (tiles == 0) return DSP_OK;
    if (rows > 0 && aug->frames.reserve((size_t)rows * dsp::kAugFft * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (the inverse STFT's frames)");
    dsp::SpanRing::Lease slot;
    if (const int rc = upload_spans(aug, spans, slot, st)) return rc;
    DSP_CAPI_HIP(dsp::launch_istft2048(reinterpret_cast<const float2 *>(d_spec) + rows0 * dsp::kAugBins, static_cast<const dsp::AugSpan *>(slot.d()), m, rows, tiles,
                                       aug->tables, aug->frames, d_out, st));
    return DSP_OK;
}

int stretch_run(dsp_augmenter *aug, const float *d_in, long m, const long *starts, const long *lens, const double *rates, float *d_out, const long *out_off,
                hipStream_t st);

}  // namespace

extern "C" {

long dsp_stft_frames(long n)
{
    if (n < 0) return capi_fail(DSP_EINVAL, "n < 0");
    return 1 + n / dsp::kAugHop;
}

long dsp_stretch_frames(long n_frames, double rate)
{
    if (n_frames < 0) return capi_fail(DSP_EINVAL, "n_frames < 0");
    if (const int rc = check_rate(rate)) return rc;
    return stretch_frames(n_frames, rate);
}

long dsp_stretch_length(long n, double rate)
{
    if (n < 0) return capi_fail(DSP_EINVAL, "n < 0");
    if (const int rc = check_rate(rate)) return rc;
    return stretch_length(n, rate);
}

int dsp_pitch_ratio(int n_steps, int bins_per_octave, int max_term, int *up, int *down)
{
    int u, d;
    if (const int rc = pitch_ratio(n_steps, bins_per_octave, max_term, u, d)) return rc;
    if (up) *up = u;
    if (down) *down = d;
    return DSP_OK;
}

double dsp_augment_normal(unsigned long long seed, unsigned long long key, unsigned long long i)
{
    uint32_t a, b;
    dsp::augment_uniforms(seed, key, i >> 1, a, b);
    const double r = std::sqrt(-2.0 * std::log((double)a * 0x1p-24)), t = 2.0 * kPi * ((double)b * 0x1p-24);
    return (i & 1) ? r * std::sin(t) : r * std::cos(t);
}

long dsp_augment_out_offsets(const long *offsets, long n, const dsp_augment_op *ops, long m, long *out_offsets)
{
    if (n < 0 || m < 0) return capi_fail(DSP_EINVAL, "n < 0 or m < 0");
    if (!out_offsets || (m > 0 && (!ops || !offsets))) return capi_fail(DSP_EINVAL, "offsets, ops and out_offsets must not be NULL");
    out_offsets[0] = 0;
    for (long j = 0; j < m; ++j) {
        long len;
        if (const int rc = check_op(ops[j], j, n, offsets, -1, len)) return rc;
        out_offsets[j + 1] = out_offsets[j] + (ops[j].kind == DSP_AUGMENT_STRETCH ? stretch_length(len, ops[j].rate) : len);
    }
    return out_offsets[m];
}

long dsp_augment_draw(unsigned long long seed, const int *labels, long n, double prob, dsp_augment_op *ops, long cap)
{
    if (n < 0 || (n > 0 && !labels)) return capi_fail(DSP_EINVAL, "n < 0 or labels NULL");
    if (!(prob >= 0.0 && prob <= 1.0)) return capi_fail(DSP_EINVAL, "prob must be in [0, 1]");
    if (ops && cap < 0) return capi_fail(DSP_EINVAL, "cap < 0");
    long count = 0;
    for (long r = 0; r < n; ++r) {
        if (labels[r] != 1 || !(dsp::stop_train_uniform(seed, kPolicyStream + 0, (uint64_t)r) < prob)) continue;
        if (ops) {
            if (count >= cap) return capi_fail(DSP_EINVAL, "the policy draws more ops than `cap`");
            dsp_augment_op op{};
            op.clip = r;
            op.key = (unsigned long long)r;
            op.kind = std::min(2, (int)std::floor(3.0 * dsp::stop_train_uniform(seed, kPolicyStream + 1, (uint64_t)r)));
            op.rate = 1.0;
            if (op.kind == DSP_AUGMENT_STRETCH) op.rate = 0.8 + 0.4 * dsp::stop_train_uniform(seed, kPolicyStream + 2, (uint64_t)r);
            else if (op.kind == DSP_AUGMENT_PITCH) op.n_steps = std::min(4, (int)std::floor(5.0 * dsp::stop_train_uniform(seed, kPolicyStream + 3, (uint64_t)r))) - 2;
            else op.sigma = 0.005f;
            ops[count] = op;
        }
        ++count;
    }
    return count;
}

int dsp_augmenter_create(int device, int pad_mode, int max_term, dsp_augmenter **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (pad_mode != DSP_PAD_REFLECT && pad_mode != DSP_PAD_ZERO) return capi_fail(DSP_EINVAL, "pad_mode must be DSP_PAD_REFLECT or DSP_PAD_ZERO");
    if (max_term < 1 || max_term > kMaxTermCap) return capi_fail(DSP_EINVAL, "max_term must be 1 .. 1024 (the resampler's cap)");
    if (const int rc = dsp::check_device(device)) return rc;
    auto t = std::make_unique<dsp::AugTables>();
    for (int i = 0; i < dsp::kAugFft; ++i) {
        const float w = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * (double)i / (double)dsp::kAugFft));
        t->win[i] = w;
        t->win_half[i] = 0.5f * w;
        t->win_sq[i] = (float)((double)w * (double)w);
    }
    for (int i = 0; i < 1024; ++i) {      // exp(-2 pi i x), evaluated in float64
        t->w1024[0][i] = (float)std::cos(-2.0 * kPi * ((double)i / 1024.0));
        t->w1024[1][i] = (float)std::sin(-2.0 * kPi * ((double)i / 1024.0));
    }
    for (int k = 0; k < 512; ++k) {
        t->w2048[0][k] = (float)std::cos(-2.0 * kPi * ((double)k / 2048.0));
        t->w2048[1][k] = (float)std::sin(-2.0 * kPi * ((double)k / 2048.0));
    }
    return dsp::create_on_device(device, out, [&](dsp_augmenter &aug) -> int {
        aug.pad_mode = pad_mode;
        aug.max_term = max_term;
        if (dsp::upload(aug.tables, *t) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc / upload of the tables");
        return DSP_OK;
    });
}

void dsp_augmenter_destroy(dsp_augmenter *aug) { dsp::destroy(aug); }

int dsp_stft_ragged_device(dsp_augmenter *aug, const float *d_in, long n, const long *offsets, float *d_spec, long *frame_offsets_out, void *stream)
{
    if (!aug || n < 0) return capi_fail(DSP_EINVAL, "bad argument (augmenter NULL or n < 0)");
    if (n == 0) return DSP_OK;
    if (!offsets || !d_in || !d_spec) return capi_fail(DSP_EINVAL, "offsets, input and output must not be NULL");
    std::vector<long> starts((size_t)n), lens((size_t)n), fo;
    for (long c = 0; c < n; ++c) {
        const long len = dsp::ragged_clip_length(offsets, c);
        if (len < 0) return (int)len;
        if (const int rc = check_clip(c, len, aug->pad_mode)) return rc;
        starts[(size_t)c] = offsets[c];
        lens[(size_t)c] = len;
    }
    DSP_ON_DEVICE(aug->device);
    if (const int rc = stft_run(aug, d_in, n, starts.data(), lens.data(), d_spec, fo, (hipStream_t)stream)) return rc;
    if (frame_offsets_out) std::memcpy(frame_offsets_out, fo.data(), (size_t)(n + 1) * sizeof(long));
    return DSP_OK;
}

int dsp_istft_ragged_device(dsp_augmenter *aug, const float *d_spec, long n, const long *frame_offsets, const long *lengths, float *d_out,
                            const long *out_offsets, void *stream)
{
    if (!aug || n < 0) return capi_fail(DSP_EINVAL, "bad argument (augmenter NULL or n < 0)");
    if (n == 0) return DSP_OK;
    if (!frame_offsets || !lengths || !out_offsets || !d_spec || !d_out)
        return capi_fail(DSP_EINVAL, "frame_offsets, lengths, out_offsets, input and output must not be NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n, "clip")) return rc;
    for (long c = 0; c < n; ++c) {
        if (lengths[c] < 0 || lengths[c] >= dsp::kAugMaxSamples) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + ": length must be 0 .. 2^24 - 1");
        if (frame_offsets[c + 1] - frame_offsets[c] > dsp::kAugMaxSamples / dsp::kAugHop)
            return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + ": more frames than a clip of 2^24 samples has");
        if (out_offsets[c] < 0) return capi_fail(DSP_EINVAL, "out_offsets must be non-negative");
    }
    DSP_ON_DEVICE(aug->device);
    return istft_run(aug, d_spec, n, frame_offsets, lengths, d_out, out_offsets, (hipStream_t)stream);
}

int dsp_time_stretch_ragged_device(dsp_augmenter *aug, const float *d_in, long n, const long *offsets, const double *rates, float *d_out, void *stream)
{
    if (!aug || n < 0) return capi_fail(DSP_EINVAL, "bad argument (augmenter NULL or n < 0)");
    if (n == 0) return DSP_OK;
    if (!offsets || !rates || !d_in || !d_out) return capi_fail(DSP_EINVAL, "offsets, rates, input and output must not be NULL");
    std::vector<long> starts((size_t)n), lens((size_t)n), oo((size_t)n + 1, 0);
    for (long c = 0; c < n; ++c) {
        const long len = dsp::ragged_clip_length(offsets, c);
        if (len < 0) return (int)len;
        if (const int rc = check_clip(c, len, aug->pad_mode)) return rc;
        if (check_rate(rates[c])) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + ": rate must be finite and in [1/8, 8]");
        starts[(size_t)c] = offsets[c];
        lens[(size_t)c] = len;
        oo[(size_t)c + 1] = oo[(size_t)c] + stretch_length(len, rates[c]);
    }
    DSP_ON_DEVICE(aug->device);
    return stretch_run(aug, d_in, n, starts.data(), lens.data(), rates, d_out, oo.data(), (hipStream_t)stream);
}

}  // extern "C"

namespace {

// the time stretch: the three entries above on the handle's workspaces
int stretch_run(dsp_augmenter *aug, const float *d_in, long m, const long *starts, const long *lens, const double *rates, float *d_out, const long *out_off,
                hipStream_t st)
{
    std::vector<long> fo, so((size_t)m + 1, 0), lengths((size_t)m);
    long rows = 0;
    for (long c = 0; c < m; ++c) {
        const long T = 1 + lens[c] / dsp::kAugHop;
        rows += T;
        so[(size_t)c + 1] = so[(size_t)c] + stretch_frames(T, rates[c]);
        lengths[(size_t)c] = stretch_length(lens[c], rates[c]);
    }
    const size_t row_bytes = (size_t)dsp::kAugBins * 2 * sizeof(float);
    if (aug->spec.reserve((size_t)rows * row_bytes) != hipSuccess || aug->spec_out.reserve((size_t)so[(size_t)m] * row_bytes) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc (the spectra of a time stretch)");
    if (const int rc = stft_run(aug, d_in, m, starts, lens, aug->spec, fo, st)) return rc;
    if (const int rc = pvoc_run(aug, aug->spec, m, fo, rates, aug->spec_out, so, st)) return rc;
    return istft_run(aug, aug->spec_out, m, so.data(), lengths.data(), d_out, out_off, st);
}

}  // namespace

extern "C" int dsp_augment_ragged_device(dsp_augmenter *aug, const float *d_in, long n, const long *offsets, const dsp_augment_op *ops, long m,
                                         unsigned long long seed, float *d_out, void *stream)
{
    if (!aug || n < 0 || m < 0) return capi_fail(DSP_EINVAL, "bad argument (augmenter NULL, n < 0 or m < 0)");
    if (m == 0) return DSP_OK;
    if (!offsets || !ops || !d_in || !d_out) return capi_fail(DSP_EINVAL, "offsets, ops, input and output must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    // ---- validate; the ops' output offsets
    std::vector<long> len((size_t)m), oo((size_t)m + 1, 0);
    struct Ratio { int up = 1, down = 1; };
    std::vector<Ratio> ratio((size_t)m);
    for (long j = 0; j < m; ++j) {
        if (const int rc = check_op(ops[j], j, n, offsets, aug->pad_mode, len[(size_t)j])) return rc;
        if (ops[j].kind == DSP_AUGMENT_PITCH)
            if (const int rc = pitch_ratio(ops[j].n_steps, 12, aug->max_term, ratio[(size_t)j].up, ratio[(size_t)j].down)) return rc;
        oo[(size_t)j + 1] = oo[(size_t)j] + (ops[j].kind == DSP_AUGMENT_STRETCH ? stretch_length(len[(size_t)j], ops[j].rate) : len[(size_t)j]);
    }
    // ---- the ops that stretch, in the order they lie in workspace A: the stretch ops, then the pitch ops ratio by ratio
    std::vector<long> order;
    for (long j = 0; j < m; ++j)
        if (ops[j].kind == DSP_AUGMENT_STRETCH) order.push_back(j);
    const size_t n_stretch = order.size();
    std::map<std::pair<int, int>, std::vector<long>> groups;
    for (long j = 0; j < m; ++j)
        if (ops[j].kind == DSP_AUGMENT_PITCH) groups[{ratio[(size_t)j].up, ratio[(size_t)j].down}].push_back(j);
    for (auto &kv : groups) order.insert(order.end(), kv.second.begin(), kv.second.end());
    const long k = (long)order.size();
    std::vector<long> starts((size_t)k), lens((size_t)k), ao((size_t)k + 1, 0), a_of((size_t)m, -1), b_of((size_t)m, -1), b_len((size_t)m, 0);
    std::vector<double> rates((size_t)k);
    for (long i = 0; i < k; ++i) {
        const long j = order[(size_t)i];
        starts[(size_t)i] = offsets[ops[j].clip];
        lens[(size_t)i] = len[(size_t)j];
        rates[(size_t)i] = ops[j].kind == DSP_AUGMENT_STRETCH ? ops[j].rate : (double)ratio[(size_t)j].up / (double)ratio[(size_t)j].down;
        ao[(size_t)i + 1] = ao[(size_t)i] + stretch_length(lens[(size_t)i], rates[(size_t)i]);
        a_of[(size_t)j] = ao[(size_t)i];
    }
    DSP_ON_DEVICE(aug->device);
    if (k > 0) {
        if (aug->ws_a.reserve((size_t)ao[(size_t)k] * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (the stretched clips)");
        if (const int rc = stretch_run(aug, d_in, k, starts.data(), lens.data(), rates.data(), aug->ws_a, ao.data(), st)) return rc;
    }
    // ---- the pitch ops: each ratio's run of workspace A through that ratio's resampler into workspace B
    struct Run { dsp_resampler *rs; long first, count, b0; std::vector<long> bo; };
    std::vector<Run> runs;
    long b_total = 0, first = (long)n_stretch;
    for (auto &kv : groups) {
        const long count = (long)kv.second.size();
        const int up = kv.first.first, down = kv.first.second;
        if (up != down) {
            auto &owner = aug->resamplers[kv.first];
            if (!owner) {
                dsp_resampler *made = nullptr;
                if (const int rc = dsp_resampler_create(aug->device, down, up, &made)) { aug->resamplers.erase(kv.first); return rc; }
                owner.reset(made);
            }
            Run run{owner.get(), first, count, b_total, std::vector<long>((size_t)count + 1)};
            const long total = dsp_resample_offsets(down, up, ao.data() + first, count, run.bo.data());
            if (total < 0) return (int)total;
            for (long i = 0; i < count; ++i) {
                b_of[(size_t)kv.second[(size_t)i]] = b_total + run.bo[(size_t)i];
                b_len[(size_t)kv.second[(size_t)i]] = run.bo[(size_t)i + 1] - run.bo[(size_t)i];
            }
            b_total += total;
            runs.push_back(std::move(run));
        }
        first += count;
    }
    if (b_total > 0 && aug->ws_b.reserve((size_t)b_total * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (the resampled clips)");
    for (const Run &run : runs)
        if (const int rc = dsp_resample_ragged_device(run.rs, aug->ws_a, run.count, ao.data() + run.first, aug->ws_b.get() + run.b0, stream)) return rc;
    // ---- the tail: source (or zeros past its end) + sigma x the draws, op by op at its output offset
    std::vector<dsp::AugSpan> spans((size_t)m + 1);
    long tiles = 0;
    for (long j = 0; j < m; ++j) {
        dsp::AugSpan &s = spans[(size_t)j];
        s = dsp::AugSpan{};
        const long n_out = oo[(size_t)j + 1] - oo[(size_t)j];
        if (ops[j].kind == DSP_AUGMENT_NOISE) { s.src = 0; s.in_off = offsets[ops[j].clip]; s.n = (int)len[(size_t)j]; }
        else if (b_of[(size_t)j] >= 0) { s.src = 2; s.in_off = b_of[(size_t)j]; s.n = (int)std::min(b_len[(size_t)j], n_out); }
        else { s.src = 1; s.in_off = a_of[(size_t)j]; s.n = (int)n_out; }      // (a stretch, or a pitch shift by 0 steps: rate 1, no resampling)
        s.out_off = oo[(size_t)j];
        s.tile0 = tiles;
        s.n_out = (int)n_out;
        s.sigma = ops[j].sigma;
        s.key = ops[j].key;
        tiles += tiles_of(n_out);
    }
    spans[(size_t)m] = dsp::AugSpan{};
    spans[(size_t)m].tile0 = tiles;
    if (tiles == 0) return DSP_OK;
    dsp::SpanRing::Lease slot;
    if (const int rc = upload_spans(aug, spans, slot, st)) return rc;
    const float *const src[3] = {d_in, aug->ws_a, aug->ws_b};
    DSP_CAPI_HIP(dsp::launch_augment_finish(src, static_cast<const dsp::AugSpan *>(slot.d()), m, tiles, seed, d_out, st));
    return DSP_OK;
}
