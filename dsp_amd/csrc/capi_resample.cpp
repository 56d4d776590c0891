// capi_resample.cpp -- the C ABI of the polyphase FIR resampler (include/dsp_amd.h dsp_resample_*): the ratio, the
// Kaiser-windowed sinc taps in float64 (scipy.signal.resample_poly's defaults), the output offsets, and the entries that put a ragged or
// uniform batch of recordings through resample_kernels.hip; behind them the streaming resampler (dsp_stream_resample*),
// which emits the same outputs from feeds that arrive in chunks.
#include <cmath>
#include <cstdint>
#include <memory>
#include <numeric>

#include "capi_util.hpp"
#include "resample_kernels.hpp"
#include "stream_kernels.hpp"
#include "stream_resample.hpp"

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

// the device table [up][row] on the current device: the taps rounded once to float32; branch p = taps p, p + up, ... reversed and zero
// filled to `row`
int upload_taps(const Ratio &ratio, const dsp::ResampleShape &s, dsp::DeviceBuf<float> &taps)
{
    const std::vector<double> h = make_taps(ratio);
    std::vector<float> table((size_t)s.up * s.row, 0.0f);
    for (int p = 0; p < s.up; ++p)
        for (int jj = 0; jj < s.taps; ++jj) {
            const long idx = p + (long)(s.taps - 1 - jj) * s.up;
            if (idx <= 2L * s.half) table[(size_t)p * s.row + jj] = (float)h[(size_t)idx];
        }
    if (taps.alloc(table.size() * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the taps");
    DSP_CAPI_HIP(hipMemcpy(taps, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    return DSP_OK;
}

}  // namespace

struct dsp_resampler : dsp::Handle {
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

int dsp_resample_geometry(int rate_in, int rate_out, int *fields, int n)
{
    Ratio r;
    if (const int rc = reduce(rate_in, rate_out, r)) return rc;
    const dsp::ResampleShape s = make_shape(r);
    const int v[] = {s.up, s.down, s.half, s.taps, s.row, s.tile, s.items, s.span, s.staged, s.lds_bytes};
    constexpr int count = (int)(sizeof(v) / sizeof(v[0]));
    if (!fields) return count;
    if (n < count) return capi_fail(DSP_EINVAL, "fields holds " + std::to_string(n) + " ints, the geometry has " + std::to_string(count) + " fields");
    std::memcpy(fields, v, sizeof(v));
    return count;
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
    return dsp::create_on_device(device, out, [&](dsp_resampler &r) {
        r.ratio = ratio;
        r.shape = make_shape(ratio);
        return upload_taps(ratio, r.shape, r.taps);
    });
}

void dsp_resampler_destroy(dsp_resampler *r) { dsp::destroy(r); }

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

// ---- live streams: the same outputs from a feed that arrives in chunks (include/dsp_amd.h dsp_stream_resample*) ----
// A stream's state is ONE host counter, the sample frames received (N): outputs emitted = K(N), first carried sample = c(N).  The carry
// buffer holds samples [c(N), N) of every stream in the caller's own format and nothing else, so a reset is a store to the counter.
namespace {

constexpr long kMaxReceived = LONG_MAX / 4096;      // N up + half and K(N) down + half stay far inside a long (up, down <= 1024)

struct StreamRatio {
    Ratio r{};
    int taps = 1;                                   // T
    bool copy() const { return r.up == 1 && r.down == 1; }
    long emitted(long n) const                      // K(N)
    {
        if (copy()) return n;
        const long a = n * r.up - 1 - r.half;
        return a >= 0 ? a / r.down + 1 : 0;
    }
    long carry_start(long n) const                  // c(N) = max(0, i_max(K(N)) - (T - 1))
    {
        if (copy()) return n;
        return std::max(0L, (emitted(n) * r.down + r.half) / r.up - (long)(taps - 1));
    }
    long whole(long n) const { return (n * r.up + r.down - 1) / r.down; }      // ceil(N up / down)
};

StreamRatio stream_ratio(const Ratio &r)
{
    StreamRatio s;
    s.r = r;
    s.taps = (2 * r.half + r.up) / r.up;
    return s;
}

// oo[n + 1] = prefix sums of K(received + chunk) - K(received); the total, or < 0
long plan_stream_push(const StreamRatio &sr, const long *received, const long *co, long n, long *oo)
{
    oo[0] = 0;
    for (long s = 0; s < n; ++s) {
        const long len = co[s + 1] - co[s], n0 = received ? received[s] : 0;
        if (co[s] < 0 || len < 0)
            return capi_fail(DSP_EINVAL, "chunk_offsets must be non-negative and non-decreasing (stream " + std::to_string(s) + ")");
        if (n0 < 0) return capi_fail(DSP_EINVAL, "received must be non-negative (stream " + std::to_string(s) + ")");
        if (len > INT32_MAX) return capi_fail(DSP_EINVAL, "a chunk must be shorter than 2^31 sample frames (stream " + std::to_string(s) + ")");
        if (n0 > kMaxReceived - len) return capi_fail(DSP_EINVAL, "the sample counter of stream " + std::to_string(s) + " would overflow");
        oo[s + 1] = oo[s] + (sr.emitted(n0 + len) - sr.emitted(n0));
    }
    return oo[n];
}

long round_up16(long x) { return (x + 15) / 16 * 16; }

}  // namespace

struct dsp_stream_resampler : dsp::Handle {
    int rate_in = 0, rate_out = 0, in_kind = 0;
    StreamRatio sr;
    dsp::ResampleShape shape{};
    long n_streams = 0;
    long es = 4;                          // bytes per sample frame: 4 float, 2 mono int16, 4 stereo int16
    long half_stride = 0;                 // bytes of one half of a stream's carry slot (T - 1 sample frames, rounded up to 16)
    std::vector<long> received;           // THE state
    // which half of its slot a stream's carry lies in: a push that keeps part of the old carry and moves it forward writes the new
    // carry into the other half, so that no run of the copy launch reads what another writes
    std::vector<char> side, next_side;
    bool broken = false;
    dsp::DeviceBuf<float> taps;
    dsp::DeviceBuf<char> d_carry;         // [n_streams][2][half_stride]
    std::vector<long> oo;
    std::vector<dsp::StreamResampleSpan> spans;
    std::vector<dsp::ResampleSpan> copy_spans;
    std::vector<dsp::CopyRun> runs;
    dsp::SpanRing ring;                   // a push's span table and run table on their way to the GPU
    std::mutex mu;
};

namespace dsp {

StreamResamplerInfo stream_resampler_info(const dsp_stream_resampler *rs) { return StreamResamplerInfo{rs->device, rs->rate_out, rs->n_streams}; }

long stream_resampler_plan(dsp_stream_resampler *rs, const long *chunk_offsets, long *out_offsets)
{
    std::lock_guard<std::mutex> lock(rs->mu);
    return plan_stream_push(rs->sr, rs->received.data(), chunk_offsets, rs->n_streams, out_offsets);
}

bool stream_resampler_broken(dsp_stream_resampler *rs)
{
    std::lock_guard<std::mutex> lock(rs->mu);
    return rs->broken;
}

}  // namespace dsp

namespace {

// the table of spans (and of copy runs behind it) into a leased slot, uploaded; d_spans / d_runs: where they lie on the GPU
template <class Span>
int upload_tables(dsp_stream_resampler *rs, const std::vector<Span> &spans, dsp::SpanRing::Lease &slot, const Span *&d_spans, const dsp::CopyRun *&d_runs,
                  hipStream_t st)
{
    static_assert(sizeof(Span) % 8 == 0, "the run table behind the spans stays 8-byte aligned");
    const size_t sb = spans.size() * sizeof(Span), rb = rs->runs.size() * sizeof(dsp::CopyRun);
    DSP_CAPI_HIP(rs->ring.acquire(sb + rb, slot));
    if (sb) std::memcpy(slot.h(), spans.data(), sb);
    if (rb) std::memcpy(static_cast<char *>(slot.h()) + sb, rs->runs.data(), rb);
    DSP_CAPI_HIP(slot.upload(sb + rb, st));
    d_spans = static_cast<const Span *>(slot.d());
    d_runs = reinterpret_cast<const dsp::CopyRun *>(static_cast<const char *>(slot.d()) + sb);
    return DSP_OK;
}

}  // namespace

extern "C" {

long dsp_stream_resample_plan(int rate_in, int rate_out, const long *received, const long *chunk_offsets, long n_streams, long *out_offsets)
{
    Ratio r;
    if (const int rc = reduce(rate_in, rate_out, r)) return rc;
    if (n_streams < 0) return capi_fail(DSP_EINVAL, "n_streams < 0");
    if (!out_offsets || (n_streams > 0 && !chunk_offsets)) return capi_fail(DSP_EINVAL, "chunk_offsets and out_offsets must not be NULL");
    return plan_stream_push(stream_ratio(r), received, chunk_offsets, n_streams, out_offsets);
}

int dsp_stream_resampler_create(int device, int rate_in, int rate_out, long n_streams, int channels, int stereo_mode, int pcm16, dsp_stream_resampler **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    int kind = 0;
    if (pcm16) {
        if ((kind = dsp::pcm16_kind(channels, stereo_mode)) < 0) return kind;
    } else if (channels != 1) {
        return capi_fail(DSP_EINVAL, "float samples are mono: channels must be 1");
    }
    Ratio ratio;
    if (const int rc = reduce(rate_in, rate_out, ratio)) return rc;
    const dsp::ResampleShape shape = make_shape(ratio);
    if (!shape.staged)
        return capi_fail(DSP_EINVAL, "resampling " + std::to_string(rate_in) + " -> " + std::to_string(rate_out) + " has " + std::to_string(shape.taps) +
                                         " taps per output: a stream would carry more samples than a block stages (not a live-feed ratio)");
    if (n_streams < 0 || n_streams >= (1L << 31)) return capi_fail(DSP_EINVAL, "n_streams must be in [0, 2^31)");
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_stream_resampler &rs) -> int {
        rs.rate_in = rate_in;
        rs.rate_out = rate_out;
        rs.in_kind = kind;
        rs.sr = stream_ratio(ratio);
        rs.shape = shape;
        rs.n_streams = n_streams;
        rs.es = kind == 1 ? 2 : 4;
        rs.half_stride = rs.sr.copy() ? 0 : round_up16((long)(shape.taps - 1) * rs.es);
        rs.received.assign((size_t)n_streams, 0);
        rs.side.assign((size_t)n_streams, 0);
        rs.next_side.assign((size_t)n_streams, 0);
        rs.oo.assign((size_t)n_streams + 1, 0);
        if (!rs.sr.copy())
            if (const int rc = upload_taps(ratio, shape, rs.taps)) return rc;
        if (n_streams > 0 && rs.half_stride > 0 && rs.d_carry.alloc((size_t)n_streams * 2 * (size_t)rs.half_stride) != hipSuccess)
            return capi_fail(DSP_ENOMEM, "hipMalloc (the streams' carried samples)");
        return DSP_OK;
    });
}

void dsp_stream_resampler_destroy(dsp_stream_resampler *rs) { dsp::destroy(rs); }

int dsp_stream_resampler_reset(dsp_stream_resampler *rs, const long *streams, long n, void *stream)
{
    (void)stream;      // nothing to enqueue: what a stream carries is defined by its counter
    if (!rs) return capi_fail(DSP_EINVAL, "resampler is NULL");
    std::lock_guard<std::mutex> lock(rs->mu);
    if (!streams) {
        std::fill(rs->received.begin(), rs->received.end(), 0L);
        rs->broken = false;
        return DSP_OK;
    }
    if (n < 0) return capi_fail(DSP_EINVAL, "n < 0");
    for (long i = 0; i < n; ++i)
        if (streams[i] < 0 || streams[i] >= rs->n_streams) return capi_fail(DSP_EINVAL, "no stream " + std::to_string(streams[i]) + " in this resampler");
    for (long i = 0; i < n; ++i) rs->received[(size_t)streams[i]] = 0;
    return DSP_OK;
}

int dsp_stream_resampler_counts(dsp_stream_resampler *rs, long *samples_in, long *samples_out)
{
    if (!rs) return capi_fail(DSP_EINVAL, "resampler is NULL");
    std::lock_guard<std::mutex> lock(rs->mu);
    for (long i = 0; i < rs->n_streams; ++i) {
        if (samples_in) samples_in[i] = rs->received[(size_t)i];
        if (samples_out) samples_out[i] = rs->sr.emitted(rs->received[(size_t)i]);
    }
    return DSP_OK;
}

int dsp_stream_resample_push_device(dsp_stream_resampler *rs, const void *d_chunks, const long *chunk_offsets, float *d_out, long *out_offsets, void *stream)
{
    if (!rs) return capi_fail(DSP_EINVAL, "resampler is NULL");
    std::lock_guard<std::mutex> lock(rs->mu);
    if (rs->broken)
        return capi_fail(DSP_EHIP, "an earlier push failed on the GPU half way: dsp_stream_resampler_reset(resampler, NULL, ...) starts every stream afresh");
    const long n = rs->n_streams, es = rs->es;
    const StreamRatio &sr = rs->sr;
    const dsp::ResampleShape &s = rs->shape;
    long *oo = rs->oo.data();
    // ---- validate and plan: nothing below this block changes the object before the last launch is enqueued
    if (n > 0 && !chunk_offsets) return capi_fail(DSP_EINVAL, "chunk_offsets is NULL");
    const long total = n > 0 ? plan_stream_push(sr, rs->received.data(), chunk_offsets, n, oo) : (oo[0] = 0);
    if (total < 0) return (int)total;
    if (n > 0 && chunk_offsets[n] > chunk_offsets[0]) {
        if (!d_chunks) return capi_fail(DSP_EINVAL, "d_chunks is NULL");
        if (reinterpret_cast<uintptr_t>(d_chunks) % (rs->in_kind == 0 ? 4u : 2u)) return capi_fail(DSP_EINVAL, "d_chunks must be aligned to one sample");
    }
    if (total > 0 && (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4)) return capi_fail(DSP_EINVAL, "d_out must not be NULL (and aligned to a float)");
    hipStream_t st = (hipStream_t)stream;
    rs->runs.clear();
    if (sr.copy()) {      // K(N) = N, nothing carried: the one-shot's copy over the chunks
        rs->copy_spans.clear();
        long tiles = 0;
        for (long c = 0; c < n; ++c) {
            const long len = chunk_offsets[c + 1] - chunk_offsets[c];
            if (len == 0) continue;
            rs->copy_spans.push_back(dsp::ResampleSpan{chunk_offsets[c], oo[c], tiles, len, (int)len, 0});
            tiles += (len + s.tile - 1) / s.tile;
        }
        if (tiles > 0) {
            DSP_ON_DEVICE(rs->device);
            dsp::SpanRing::Lease slot;
            const dsp::ResampleSpan *d_spans;
            const dsp::CopyRun *d_runs;
            if (const int rc = upload_tables(rs, rs->copy_spans, slot, d_spans, d_runs, st)) return rc;
            DSP_CAPI_HIP(dsp::launch_resample(d_chunks, rs->in_kind, d_spans, (long)rs->copy_spans.size(), tiles, s, nullptr, d_out, st));
        }
    } else {
        rs->spans.clear();
        long tiles = 0;
        for (long c = 0; c < n; ++c) {
            const long len = chunk_offsets[c + 1] - chunk_offsets[c], n0 = rs->received[(size_t)c], n1 = n0 + len;
            const long k0 = sr.emitted(n0), k1 = sr.emitted(n1), c0 = sr.carry_start(n0), c1 = sr.carry_start(n1);
            const int cur = rs->side[(size_t)c];
            const long here = (2 * c + cur) * rs->half_stride, there = (2 * c + 1 - cur) * rs->half_stride;      // bytes into d_carry
            rs->next_side[(size_t)c] = (char)cur;
            if (c0 > n0 || c1 > n1 || c1 < c0 || (n1 - c1) * es > rs->half_stride)
                return capi_fail(DSP_EINVAL, "internal: the carry of stream " + std::to_string(c) + " would not fit its slot");
            if (k1 > k0) {
                rs->spans.push_back(dsp::StreamResampleSpan{k0, oo[c], tiles, k1 - k0, c0, n0, n1, here / es, chunk_offsets[c]});
                tiles += (k1 - k0 + s.tile - 1) / s.tile;
            }
            if (len == 0) continue;
            if (c1 >= n0) {              // the new carry lies in the chunk
                dsp::add_copy_runs(rs->runs, (chunk_offsets[c] + (c1 - n0)) * es, here, (n1 - c1) * es, 1);
            } else if (c1 == c0) {       // nothing leaves the carry: the chunk goes behind it
                dsp::add_copy_runs(rs->runs, chunk_offsets[c] * es, here + (n0 - c0) * es, len * es, 1);
            } else {                     // the carry's tail moves to the front of the other half, the chunk behind it
                dsp::add_copy_runs(rs->runs, here + (c1 - c0) * es, there, (n0 - c1) * es, 0);
                dsp::add_copy_runs(rs->runs, chunk_offsets[c] * es, there + (n0 - c1) * es, len * es, 1);
                rs->next_side[(size_t)c] = (char)(1 - cur);
            }
        }
        if (tiles > 0 || !rs->runs.empty()) {
            DSP_ON_DEVICE(rs->device);
            dsp::SpanRing::Lease slot;
            const dsp::StreamResampleSpan *d_spans;
            const dsp::CopyRun *d_runs;
            if (const int rc = upload_tables(rs, rs->spans, slot, d_spans, d_runs, st)) return rc;
            // ---- the launches: the filter only reads the carry, the copy behind it writes the new one
            if (tiles > 0)
                DSP_CAPI_HIP(dsp::launch_resample_stream(rs->d_carry, d_chunks, rs->in_kind, d_spans, (long)rs->spans.size(), tiles, s, rs->taps, d_out, st));
            // interleaved stereo at an odd int16 is copied in int16 units
            const int granule = es == 2 || reinterpret_cast<uintptr_t>(d_chunks) % 4 ? 2 : 4;
            const hipError_t e = dsp::launch_stream_copy(d_runs, (long)rs->runs.size(), rs->d_carry, d_chunks, rs->d_carry, granule, st);
            if (e != hipSuccess) {
                rs->broken = tiles > 0;      // (behind the first launch: the caller's output is written, the carry is not)
                return capi_fail(DSP_EHIP, std::string("launch_stream_copy: ") + hipGetErrorString(e));
            }
        }
        rs->side.swap(rs->next_side);
    }
    // ---- commit
    for (long c = 0; c < n; ++c) rs->received[(size_t)c] += chunk_offsets[c + 1] - chunk_offsets[c];
    if (out_offsets) std::memcpy(out_offsets, oo, (size_t)(n + 1) * sizeof(long));
    return DSP_OK;
}

int dsp_stream_resample_finish_device(dsp_stream_resampler *rs, const long *streams, long n, float *d_out, long *out_offsets, void *stream)
{
    if (!rs) return capi_fail(DSP_EINVAL, "resampler is NULL");
    std::lock_guard<std::mutex> lock(rs->mu);
    if (rs->broken)
        return capi_fail(DSP_EHIP, "an earlier push failed on the GPU half way: dsp_stream_resampler_reset(resampler, NULL, ...) starts every stream afresh");
    if (n < 0) return capi_fail(DSP_EINVAL, "n < 0");
    if (n > 0 && !streams) return capi_fail(DSP_EINVAL, "streams is NULL");
    const StreamRatio &sr = rs->sr;
    const dsp::ResampleShape &s = rs->shape;
    for (long i = 0; i < n; ++i)
        if (streams[i] < 0 || streams[i] >= rs->n_streams) return capi_fail(DSP_EINVAL, "no stream " + std::to_string(streams[i]) + " in this resampler");
    rs->spans.clear();
    std::vector<long> oo((size_t)n + 1, 0);
    std::vector<char> named((size_t)rs->n_streams, 0);
    long tiles = 0;
    for (long i = 0; i < n; ++i) {
        const long c = streams[i], n0 = rs->received[(size_t)c], k0 = sr.emitted(n0), k1 = sr.whole(n0);
        if (named[(size_t)c]) return capi_fail(DSP_EINVAL, "stream " + std::to_string(c) + " is named twice");
        named[(size_t)c] = 1;
        oo[(size_t)i + 1] = oo[(size_t)i] + (k1 - k0);
        if (k1 > k0) {
            const long here = (2 * c + rs->side[(size_t)c]) * rs->half_stride;
            rs->spans.push_back(dsp::StreamResampleSpan{k0, oo[(size_t)i], tiles, k1 - k0, sr.carry_start(n0), n0, n0, here / rs->es, 0});
            tiles += (k1 - k0 + s.tile - 1) / s.tile;
        }
    }
    if (tiles > 0) {
        if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4) return capi_fail(DSP_EINVAL, "d_out must not be NULL (and aligned to a float)");
        DSP_ON_DEVICE(rs->device);
        hipStream_t st = (hipStream_t)stream;
        rs->runs.clear();
        dsp::SpanRing::Lease slot;
        const dsp::StreamResampleSpan *d_spans;
        const dsp::CopyRun *d_runs;
        if (const int rc = upload_tables(rs, rs->spans, slot, d_spans, d_runs, st)) return rc;
        DSP_CAPI_HIP(dsp::launch_resample_stream(rs->d_carry, rs->d_carry, rs->in_kind, d_spans, (long)rs->spans.size(), tiles, s, rs->taps, d_out, st));
    }
    for (long i = 0; i < n; ++i) rs->received[(size_t)streams[i]] = 0;
    if (out_offsets) std::memcpy(out_offsets, oo.data(), (size_t)(n + 1) * sizeof(long));
    return DSP_OK;
}

}  // extern "C"
