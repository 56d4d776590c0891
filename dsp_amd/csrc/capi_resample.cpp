// capi_resample.cpp -- the C ABI of the polyphase FIR resampler (include/dsp_amd.h dsp_resample_*): the ratio, the
// Kaiser-windowed sinc taps in float64 (scipy.signal.resample_poly's defaults), the output offsets, and the entries that put a ragged or
// uniform batch of recordings through resample_kernels.hip.
#include <cmath>
#include <cstdint>
#include <memory>
#include <numeric>

#include "capi_util.hpp"
#include "resample_kernels.hpp"

using dsp::capi_fail;

namespace {

constexpr int kMaxFactor = 1024;
constexpr double kBeta = 5.0;
constexpr double kPi = 3.14159265358979323846;

// I0(x) for 0 <= x <= 5: the power series sum_k ((x / 2)^2k / (k!)^2), every term positive -- converged to the last bit within 30 terms
double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

struct Ratio { int up, down, half; };

int reduce(int rate_in, int rate_out, Ratio &r)
{
    if (rate_in < 1 || rate_out < 1) return capi_fail(DSP_EINVAL, "rate_in and rate_out must be >= 1");
    const int g = std::gcd(rate_in, rate_out);
    r.up = rate_out / g;
    r.down = rate_in / g;
    if (r.up > kMaxFactor || r.down > kMaxFactor)
        return capi_fail(DSP_EINVAL, "resampling " + std::to_string(rate_in) + " -> " + std::to_string(rate_out) + " reduces to " + std::to_string(r.up) + " / " +
                                         std::to_string(r.down) + ": up and down must each be <= 1024");
    r.half = 10 * std::max(r.up, r.down);
    return DSP_OK;
}

// h[n] = up v[n] / sum v,  v[n] = sinc((n - half) / m) / m * I0(beta sqrt(1 - ((n - half) / half)^2)) / I0(beta)
std::vector<double> make_taps(const Ratio &r)
{
    const int m = std::max(r.up, r.down), len = 2 * r.half + 1;
    std::vector<double> h((size_t)len);
    const double cutoff = 1.0 / m, i0b = bessel_i0(kBeta);
    long double sum = 0.0L;                                       // (8 821 terms of both signs at 44.1 kHz: a double sum loses a digit)
    for (int n = 0; n < len; ++n) {
        const double d = (double)(n - r.half), t = kPi * (cutoff * d);
        const double sinc = n == r.half ? 1.0 : std::sin(t) / t;
        const double u = d / (double)r.half, arg = 1.0 - u * u;
        h[(size_t)n] = cutoff * sinc * (bessel_i0(kBeta * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b);
        sum += h[(size_t)n];
    }
    const double total = (double)sum;
    for (double &v : h) v = v / total * (double)r.up;
    return h;
}

// ceil(n up / down), n >= 0 (n <= INT_MAX and up <= 1024: no overflow, checked all the same)
int out_length(long n, const Ratio &r, long &out)
{
    long prod;
    if (__builtin_mul_overflow(n, (long)r.up, &prod) || __builtin_add_overflow(prod, (long)(r.down - 1), &prod)) return capi_fail(DSP_EINVAL, "n * up overflows");
    out = prod / r.down;
    return DSP_OK;
}

// The geometry of a ratio (resample_kernels.hpp ResampleShape): `groups` lane groups of `up` work items each, chosen for the fullest
// 256-lane passes and the smallest share of re-read filter history within the LDS budget.  A function of (up, down) only.
dsp::ResampleShape make_shape(const Ratio &r)
{
    constexpr int R = dsp::kResampleOutputsPerLane, kLdsBudget = 40 * 1024, kMaxTile = 4096;
    dsp::ResampleShape s{};
    s.up = r.up; s.down = r.down; s.half = r.half;
    s.taps = (2 * r.half + r.up) / r.up;
    s.row = (s.taps + 3) & ~3;
    auto span_of = [&](int tile) { return (int)(((long)(tile - 1) * r.down + r.up - 1) / r.up) + s.row; };
    auto bytes_of = [&](int tile) { return (tile + span_of(tile) + 16) * 4; };
    int best = 0;
    double best_score = -1.0;
    for (int groups = 1; groups <= kMaxTile; ++groups) {
        const int tile = R * r.up * groups;
        if (tile > kMaxTile && groups > 1) break;
        if (bytes_of(tile) > kLdsBudget) break;
        const int items = r.up * groups, passes = (items + 255) / 256;
        const double fill = (double)items / (256.0 * passes), fresh = 1.0 - (double)s.row / span_of(tile);
        if (fill * fresh > best_score) { best_score = fill * fresh; best = groups; }
    }
    s.staged = best > 0;
    if (!s.staged) best = std::max(1, 1024 / (R * r.up));          // a branch longer than the LDS budget: samples from global memory
    s.tile = R * r.up * best;
    s.items = r.up * best;
    s.span = span_of(s.tile);
    s.lds_bytes = s.staged ? bytes_of(s.tile) : s.tile * 4;
    return s;
}

}  // namespace

struct dsp_resampler {
    int device = 0;
    Ratio ratio{};
    dsp::ResampleShape shape{};
    dsp::DeviceBuf<float> taps;      // [up][row]: branch p reversed, so that ascending index = ascending input sample
    dsp::SpanRing spans;
};

namespace {

// recording c: len(c) samples at in_off(c) of the input -> ceil(len(c) up / down) floats at out_off(c) of the output
template <class InOff, class Len, class OutOff>
int run(dsp_resampler *r, const void *d_in, int in_kind, long n_rec, InOff in_off, Len len, OutOff out_off, float *d_out, void *stream)
{
    const dsp::ResampleShape &s = r->shape;
    DSP_ON_DEVICE(r->device);
    dsp::SpanRing::Lease slot;
    const size_t bytes = (size_t)n_rec * sizeof(dsp::ResampleSpan);
    DSP_CAPI_HIP(r->spans.acquire(bytes, slot));
    dsp::ResampleSpan *h = static_cast<dsp::ResampleSpan *>(slot.h());
    long tiles = 0;
    for (long c = 0; c < n_rec; ++c) {
        long n_out;
        if (const int rc = out_length(len(c), r->ratio, n_out)) return rc;
        h[c] = dsp::ResampleSpan{in_off(c), out_off(c), tiles, n_out, (int)len(c), 0};
        tiles += (n_out + s.tile - 1) / s.tile;
    }
    if (tiles == 0) return DSP_OK;
    DSP_CAPI_HIP(slot.upload(bytes, (hipStream_t)stream));
    DSP_CAPI_HIP(dsp::launch_resample(d_in, in_kind, static_cast<const dsp::ResampleSpan *>(slot.d()), n_rec, tiles, s, r->taps, d_out, (hipStream_t)stream));
    return DSP_OK;
}

int run_ragged(dsp_resampler *r, const void *d_in, int in_kind, long n, const long *offsets, float *d_out, void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!r || n < 0 || (n > 0 && (!offsets || !d_in || !d_out))) return capi_fail(DSP_EINVAL, "bad argument (resampler, offsets, input and output must not be NULL)");
    if (n == 0) return DSP_OK;
    std::vector<long> out_offsets((size_t)n + 1);
    const long total = dsp_resample_offsets(r->ratio.down, r->ratio.up, offsets, n, out_offsets.data());
    if (total < 0) return (int)total;
    return run(r, d_in, in_kind, n, [&](long c) { return offsets[c]; }, [&](long c) { return offsets[c + 1] - offsets[c]; },
               [&](long c) { return out_offsets[(size_t)c]; }, d_out, stream);
}

int run_clips(dsp_resampler *r, const void *d_in, int in_kind, long n_clips, int samples, long stride, float *d_out, long out_stride, void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!r || n_clips < 0 || samples < 0) return capi_fail(DSP_EINVAL, "bad argument (resampler NULL, n_clips < 0 or samples < 0)");
    long n_out;
    if (const int rc = out_length(samples, r->ratio, n_out)) return rc;
    if (n_out > INT_MAX) return capi_fail(DSP_EINVAL, "a clip's output must be shorter than 2^31 samples");
    if (n_clips > 1 && (stride < samples || out_stride < n_out)) return capi_fail(DSP_EINVAL, "stride < samples or out_stride < the output length of a clip");
    if (n_clips == 0 || n_out == 0) return (int)n_out;
    if (!d_in || !d_out) return capi_fail(DSP_EINVAL, "input and output must not be NULL");
    const int rc = run(r, d_in, in_kind, n_clips, [&](long c) { return c * stride; }, [&](long) { return (long)samples; },
                       [&](long c) { return c * out_stride; }, d_out, stream);
    return rc < 0 ? rc : (int)n_out;
}

}  // namespace

extern "C" {

int dsp_resample_ratio(int rate_in, int rate_out, int *up, int *down, int *half_len)
{
    Ratio r;
    if (const int rc = reduce(rate_in, rate_out, r)) return rc;
    if (up) *up = r.up;
    if (down) *down = r.down;
    if (half_len) *half_len = r.half;
    return DSP_OK;
}

int dsp_resample_taps(int rate_in, int rate_out, double *h, int n)
{
    Ratio r;
    if (const int rc = reduce(rate_in, rate_out, r)) return rc;
    const int len = 2 * r.half + 1;
    if (!h) return len;
    if (n < len) return capi_fail(DSP_EINVAL, "h holds " + std::to_string(n) + " doubles, the filter has " + std::to_string(len) + " taps");
    const std::vector<double> taps = make_taps(r);
    std::memcpy(h, taps.data(), (size_t)len * sizeof(double));
    return len;
}

long dsp_resample_offsets(int rate_in, int rate_out, const long *offsets, long n, long *out_offsets)
{
    Ratio r;
    if (const int rc = reduce(rate_in, rate_out, r)) return rc;
    if (n < 0) return capi_fail(DSP_EINVAL, "n < 0");
    if (!out_offsets || (n > 0 && !offsets)) return capi_fail(DSP_EINVAL, "offsets and out_offsets must not be NULL");
    out_offsets[0] = 0;
    for (long c = 0; c < n; ++c) {
        const long len = dsp::ragged_clip_length(offsets, c);
        if (len < 0) return len;
        long n_out;
        if (const int rc = out_length(len, r, n_out)) return rc;
        if (__builtin_add_overflow(out_offsets[c], n_out, &out_offsets[c + 1])) return capi_fail(DSP_EINVAL, "the output offsets overflow");
    }
    return out_offsets[n];
}

int dsp_resampler_create(int device, int rate_in, int rate_out, dsp_resampler **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    Ratio ratio;
    if (const int rc = reduce(rate_in, rate_out, ratio)) return rc;
    if (const int rc = dsp::check_device(device)) return rc;
    auto r = std::make_unique<dsp_resampler>();
    r->device = device;
    r->ratio = ratio;
    r->shape = make_shape(ratio);
    const dsp::ResampleShape &s = r->shape;
    // rounded once to float32; branch p = taps p, p + up, ... reversed and zero filled to `row`
    const std::vector<double> h = make_taps(ratio);
    std::vector<float> table((size_t)s.up * s.row, 0.0f);
    for (int p = 0; p < s.up; ++p)
        for (int jj = 0; jj < s.taps; ++jj) {
            const long idx = p + (long)(s.taps - 1 - jj) * s.up;
            if (idx <= 2L * s.half) table[(size_t)p * s.row + jj] = (float)h[(size_t)idx];
        }
    DSP_ON_DEVICE(device);
    if (r->taps.alloc(table.size() * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the taps");
    DSP_CAPI_HIP(hipMemcpy(r->taps, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = r.release();
    return DSP_OK;
}

void dsp_resampler_destroy(dsp_resampler *r)
{
    if (!r) return;
    dsp::DeviceScope scope(r->device);
    r->spans.release();
    delete r;
}

int dsp_resample_ragged_device(dsp_resampler *r, const float *d_in, long n, const long *offsets, float *d_out, void *stream)
{
    return run_ragged(r, d_in, 0, n, offsets, d_out, stream);
}

int dsp_resample_ragged_pcm16_device(dsp_resampler *r, const int16_t *d_pcm, long n, const long *offsets, int channels, int stereo_mode,
                                     float *d_out, void *stream)
{
    return run_ragged(r, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n, offsets, d_out, stream);
}

int dsp_resample_clips_device(dsp_resampler *r, const float *d_in, long n_clips, int samples, long stride, float *d_out, long out_stride, void *stream)
{
    return run_clips(r, d_in, 0, n_clips, samples, stride, d_out, out_stride, stream);
}

int dsp_resample_clips_pcm16_device(dsp_resampler *r, const int16_t *d_pcm, long n_clips, int samples, long stride, int channels, int stereo_mode,
                                    float *d_out, long out_stride, void *stream)
{
    return run_clips(r, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, samples, stride, d_out, out_stride, stream);
}

int dsp_resample_host(int rate_in, int rate_out, const float *in, long n, float *out)
{
    Ratio ratio;
    if (const int rc = reduce(rate_in, rate_out, ratio)) return rc;
    if (n < 0 || n > INT_MAX) return capi_fail(DSP_EINVAL, "a recording holds 0 .. 2^31 - 1 samples");
    if (n == 0) return DSP_OK;
    if (!in || !out) return capi_fail(DSP_EINVAL, "in and out must not be NULL");
    long n_out;
    if (const int rc = out_length(n, ratio, n_out)) return rc;
    dsp_resampler *r = nullptr;
    if (const int rc = dsp_resampler_create(0, rate_in, rate_out, &r)) return rc;
    std::unique_ptr<dsp_resampler, void (*)(dsp_resampler *)> owner(r, dsp_resampler_destroy);
    dsp::DeviceBuf<float> d_in, d_out;
    if (d_in.alloc((size_t)n * 4) != hipSuccess || d_out.alloc((size_t)n_out * 4) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc");
    DSP_CAPI_HIP(hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice));
    const long offsets[2] = {0, n};
    if (const int rc = dsp_resample_ragged_device(r, d_in, 1, offsets, d_out, nullptr)) return rc;
    DSP_CAPI_HIP(hipMemcpy(out, d_out, (size_t)n_out * 4, hipMemcpyDeviceToHost));      // (the null stream: ordered behind the kernel)
    return DSP_OK;
}

}  // extern "C"
