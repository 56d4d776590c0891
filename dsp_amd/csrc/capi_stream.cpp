// capi_stream.cpp -- C ABI of stream sessions (include/dsp_amd.h "LIVE STREAMS"): N live streams on one GPU, each push hands over the
// next chunk of every stream and gets the MFCC rows and the window scores that became complete with it.  The MFCC kernel and the
// window scans are the ones dsp_mfcc_clips_ragged_device and dsp_scanner_run_device run; what is new is the state between two pushes:
// per stream the samples behind its last row's hop (< frame_length of them) and the rows behind its last window's hop (< window_frames),
// and the gather (stream_kernels.hip) that puts them in front of the new chunk / the new rows.
//
// A stream's state is a function of ONE host counter, the samples it has received: rows = R(received), windows = W(rows), carried
// samples = received - rows hop_length, carried rows = rows - windows hop_frames.  The device buffers hold what those numbers say and
// nothing else, so a reset is a store to the counter.
//
// Feeds at another rate: dsp_stream_session_attach_resampler puts a streaming resampler (capi_resample.cpp, stream_resample.hpp) in
// front.  A push then resamples the caller's chunks into d_resampled and runs the same push on the result.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "mfcc_plan.hpp"
#include "stream_kernels.hpp"
#include "stream_resample.hpp"

using dsp::capi_fail;
using dsp::CopyRun;

namespace {

// the formulas of include/dsp_amd.h: rows after n samples, windows after e rows (wf = 0: a session without models has no windows)
struct StreamRule {
    long fl = 0, h = 0, wf = 0, hf = 1;
    long rows(long n) const { return n >= fl ? 1 + (n - fl) / h : 0; }
    long windows(long e) const { return wf > 0 && e >= wf ? 1 + (e - wf) / hf : 0; }
};

int stream_rule(const dsp_mfcc_config *mfcc, const dsp_scan_config *scan, StreamRule &r)
{
    if (!mfcc) return capi_fail(DSP_EINVAL, "mfcc config is NULL");
    const long none = 0;
    long fo = 0;
    if (const long rc = dsp_mfcc_ragged_frame_offsets(mfcc, &none, 0, INT_MAX, &fo); rc < 0) return (int)rc;      // an invalid config, with its reason
    if (mfcc->framing != DSP_FRAMING_COMPLETE) return capi_fail(DSP_EINVAL, "streams are cut into complete frames: DSP_FRAMING_COMPLETE");
    if (mfcc->hop_length > mfcc->frame_length)
        return capi_fail(DSP_EINVAL, "hop_length > frame_length: a stream would have to skip input between rows");
    r.fl = mfcc->frame_length;
    r.h = mfcc->hop_length;
    r.wf = 0;
    r.hf = 1;
    if (scan) {
        if (const int rc = dsp::scan_args(scan, 0)) return rc;
        if (scan->hop_frames > scan->window_frames)
            return capi_fail(DSP_EINVAL, "hop_frames > window_frames: a stream would have to skip rows between windows");
        r.wf = scan->window_frames;
        r.hf = scan->hop_frames;
    }
    return DSP_OK;
}

// what a push emits: ro / wo [n + 1] = prefix sums of the new rows / new windows (wo may be NULL); the new rows in total, or < 0
long plan_push(const StreamRule &r, const long *received, const long *co, long n, long *ro, long *wo)
{
    ro[0] = 0;
    if (wo) wo[0] = 0;
    for (long s = 0; s < n; ++s) {
        const long len = co[s + 1] - co[s], n0 = received ? received[s] : 0;
        if (co[s] < 0 || len < 0)
            return capi_fail(DSP_EINVAL, "chunk_offsets must be non-negative and non-decreasing (stream " + std::to_string(s) + ")");
        if (n0 < 0) return capi_fail(DSP_EINVAL, "received must be non-negative (stream " + std::to_string(s) + ")");
        if (len > INT32_MAX - r.fl) return capi_fail(DSP_EINVAL, "a chunk must be shorter than 2^31 - frame_length samples (stream " + std::to_string(s) + ")");
        if (n0 > LONG_MAX - len) return capi_fail(DSP_EINVAL, "the sample counter of stream " + std::to_string(s) + " would overflow");
        const long e0 = r.rows(n0), e1 = r.rows(n0 + len);
        ro[s + 1] = ro[s] + (e1 - e0);
        if (wo) wo[s + 1] = wo[s] + (r.windows(e1) - r.windows(e0));
    }
    return ro[n];
}

long round_up(long x, long to) { return (x + to - 1) / to * to; }

}  // namespace

struct dsp_stream_session : dsp::Handle {      // device: the plan's
    dsp_mfcc_plan *plan = nullptr;
    dsp_stop_model *stop = nullptr;
    dsp_speaker_model *spk = nullptr;
    dsp_scan_config scfg{};
    StreamRule rule;
    bool scans = false;                   // a model was given: windows exist
    int in_kind = 0;
    long n_streams = 0;
    long es = 4;                          // bytes per sample frame: 4 float, 2 mono int16, 4 stereo int16
    long carry_stride = 0, row_stride = 0;      // bytes per stream in d_carry / d_rowcarry (multiples of 16)
    std::vector<long> received;           // THE state: samples per stream so far
    bool broken = false;                  // a HIP call failed behind a push's first launch: the carries are not what `received` says
    // per stream: the last received - rows hop_length sample frames, in the input's own format / the last rows - windows hop_frames rows
    dsp::DeviceBuf<char> d_carry, d_rowcarry;
    // per push, grow-only: the stitched spans (each at a 16-byte boundary), the new rows when the caller takes none, the scans' matrix
    dsp::DeviceBuf<char> d_stage, d_new, d_scanmat;
    std::vector<long> ro, wo, fo, starts, lengths;     // the host planner's tables (allocated once)
    std::vector<CopyRun> runs[4];         // stitch, sample tails, scan matrix, row tails
    dsp::SpanRing ring;                   // the four run tables of a push on their way to the GPU
    // a resampler in front (dsp_stream_session_attach_resampler; borrowed): pushes arrive at its rate_in and in its format
    dsp_stream_resampler *rs = nullptr;
    bool pushed = false;                  // a push was accepted: too late to attach
    dsp::DeviceBuf<char> d_resampled;     // per push, grow-only: the chunks at the models' rate, back to back
    std::vector<long> roo;                // their offsets
    mutable std::mutex mu;
};

extern "C" {

long dsp_stream_push_plan(const dsp_mfcc_config *mfcc, const dsp_scan_config *scan, const long *received, const long *chunk_offsets,
                          long n_streams, long *row_offsets, long *window_offsets)
{
    StreamRule r;
    if (const int rc = stream_rule(mfcc, scan, r)) return rc;
    if (n_streams < 0) return capi_fail(DSP_EINVAL, "n_streams < 0");
    if (!chunk_offsets || !row_offsets) return capi_fail(DSP_EINVAL, "chunk_offsets and row_offsets must not be NULL");
    return plan_push(r, received, chunk_offsets, n_streams, row_offsets, window_offsets);
}

int dsp_stream_session_create(dsp_mfcc_plan *plan, dsp_stop_model *stop, dsp_speaker_model *speaker, const dsp_scan_config *scan,
                              long n_streams, int channels, int stereo_mode, int pcm16, dsp_stream_session **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (!plan) return capi_fail(DSP_EINVAL, "plan is NULL");
    if (n_streams < 0 || n_streams >= (1L << 31)) return capi_fail(DSP_EINVAL, "n_streams must be in [0, 2^31)");
    const bool scans = stop || speaker;
    if (scans)
        if (const int rc = dsp::scan_args(scan, 0)) return rc;
    int kind = 0;
    if (pcm16) {
        if ((kind = dsp::pcm16_kind(channels, stereo_mode)) < 0) return kind;
    } else if (channels != 1) {
        return capi_fail(DSP_EINVAL, "float samples are mono: channels must be 1");
    }
    if (const int rc = dsp::scan_front_check(plan, kind, stop, speaker, scan)) return rc;      // the plan's kernel takes this input, as a ragged batch
    const dsp_mfcc_config &pcfg = plan->cfg;
    StreamRule rule;
    if (const int rc = stream_rule(&pcfg, scans ? scan : nullptr, rule)) return rc;
    return dsp::create_on_device(plan->device, out, [&](dsp_stream_session &s) -> int {
        s.plan = plan;
        s.stop = stop;
        s.spk = speaker;
        s.scans = scans;
        if (scans) s.scfg = *scan;
        s.rule = rule;
        s.in_kind = kind;
        s.n_streams = n_streams;
        s.es = kind == 1 ? 2 : 4;
        s.carry_stride = round_up((rule.fl - 1) * s.es, 16);
        s.row_stride = scans ? round_up((rule.wf - 1) * (long)pcfg.n_mfcc * 4, 16) : 0;
        s.received.assign((size_t)n_streams, 0);
        for (std::vector<long> *v : {&s.ro, &s.wo, &s.fo, &s.starts, &s.lengths}) v->assign((size_t)n_streams + 1, 0);
        if (n_streams > 0 && s.carry_stride > 0 && s.d_carry.alloc((size_t)n_streams * s.carry_stride) != hipSuccess)
            return capi_fail(DSP_ENOMEM, "hipMalloc (the streams' carried samples)");
        if (n_streams > 0 && s.row_stride > 0 && s.d_rowcarry.alloc((size_t)n_streams * s.row_stride) != hipSuccess)
            return capi_fail(DSP_ENOMEM, "hipMalloc (the streams' carried rows)");
        return DSP_OK;
    });
}

void dsp_stream_session_destroy(dsp_stream_session *s) { dsp::destroy(s); }

int dsp_stream_session_reset(dsp_stream_session *s, const long *streams, long n, void *stream)
{
    (void)stream;      // nothing to enqueue: what a stream carries is defined by its counter, and later pushes are ordered behind earlier ones
    if (!s) return capi_fail(DSP_EINVAL, "session is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    if (!streams) {
        if (s->rs)
            if (const int rc = dsp_stream_resampler_reset(s->rs, nullptr, 0, stream)) return rc;
        std::fill(s->received.begin(), s->received.end(), 0L);
        s->broken = false;
        return DSP_OK;
    }
    if (n < 0) return capi_fail(DSP_EINVAL, "n < 0");
    for (long i = 0; i < n; ++i)
        if (streams[i] < 0 || streams[i] >= s->n_streams) return capi_fail(DSP_EINVAL, "no stream " + std::to_string(streams[i]) + " in this session");
    if (s->rs)
        if (const int rc = dsp_stream_resampler_reset(s->rs, streams, n, stream)) return rc;
    for (long i = 0; i < n; ++i) s->received[(size_t)streams[i]] = 0;
    return DSP_OK;
}

int dsp_stream_session_counts(const dsp_stream_session *s, long *samples, long *rows, long *windows)
{
    if (!s) return capi_fail(DSP_EINVAL, "session is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    for (long i = 0; i < s->n_streams; ++i) {
        const long n = s->received[(size_t)i], e = s->rule.rows(n);
        if (samples) samples[i] = n;
        if (rows) rows[i] = e;
        if (windows) windows[i] = s->rule.windows(e);
    }
    return DSP_OK;
}

// behind the first launch of a push a failure leaves the carries half written
#define DSP_STREAM_HIP(call)                                                                                                      \
    do {                                                                                                                          \
        hipError_t e_ = (call);                                                                                                   \
        if (e_ != hipSuccess) {                                                                                                   \
            s->broken = true;                                                                                                     \
            return capi_fail(DSP_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));                                        \
        }                                                                                                                         \
    } while (0)

int dsp_stream_push_device(dsp_stream_session *s, const void *d_pushed, const long *pushed_offsets, float *d_mfcc, float *d_prob,
                           int64_t *d_llr_mean, int *d_labels, long *row_offsets, long *window_offsets, void *stream)
{
    if (!s) return capi_fail(DSP_EINVAL, "session is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->broken)
        return capi_fail(DSP_EHIP, "an earlier push failed on the GPU half way: dsp_stream_session_reset(session, NULL, ...) starts every stream afresh");
    const long n = s->n_streams;
    const StreamRule &r = s->rule;
    long *ro = s->ro.data(), *wo = s->wo.data(), *fo = s->fo.data();
    // ---- validate and plan: nothing below this block changes the session before the last launch is enqueued
    if (n > 0 && !pushed_offsets) return capi_fail(DSP_EINVAL, "chunk_offsets is NULL");
    // d_chunks / chunk_offsets: the chunks at the models' rate -- the caller's, or what the resampler in front will make of them
    const void *d_chunks = d_pushed;
    const long *chunk_offsets = pushed_offsets;
    if (s->rs) {
        const long total = dsp::stream_resampler_plan(s->rs, pushed_offsets, s->roo.data());
        if (total < 0) return (int)total;
        DSP_ON_DEVICE(s->device);
        if (s->d_resampled.reserve((size_t)total * 4 + 16) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (resampled chunks)");
        d_chunks = s->d_resampled.get();
        chunk_offsets = s->roo.data();
    }
    // the resampler's push: behind every check of this one, in front of its first launch.  Refused, it has changed nothing.
    auto resample = [&]() -> int {
        if (!s->rs) return DSP_OK;
        const int rc = dsp_stream_resample_push_device(s->rs, d_pushed, pushed_offsets, reinterpret_cast<float *>(s->d_resampled.get()), nullptr, stream);
        if (rc < 0 && dsp::stream_resampler_broken(s->rs)) s->broken = true;
        return rc;
    };
    const long total_rows = n > 0 ? plan_push(r, s->received.data(), chunk_offsets, n, ro, wo) : (ro[0] = wo[0] = 0);
    if (total_rows < 0) return (int)total_rows;
    const long total_win = wo[n];
    if (n > 0 && chunk_offsets[n] > chunk_offsets[0]) {
        if (!d_chunks) return capi_fail(DSP_EINVAL, "d_chunks is NULL");
        if (reinterpret_cast<uintptr_t>(d_chunks) % (uintptr_t)s->es) return capi_fail(DSP_EINVAL, "d_chunks must be aligned to one sample frame");
    }
    if (total_win > 0 && s->stop && !d_prob) return capi_fail(DSP_EINVAL, "the session has a stop model: d_prob must not be NULL");
    if (total_win > 0 && s->spk && !d_llr_mean) return capi_fail(DSP_EINVAL, "the session has a speaker model: d_llr_mean must not be NULL");
    const long es = s->es, align = 16 / es, rb = (long)s->plan->cfg.n_mfcc * 4;
    for (auto &v : s->runs) v.clear();
    long pos = 0, n_spans = 0, n_scan = 0, scan_win = 0;
    fo[0] = 0;
    for (long st = 0; st < n; ++st) {
        const long len = chunk_offsets[st + 1] - chunk_offsets[st], n0 = s->received[(size_t)st], n1 = n0 + len;
        const long e0 = r.rows(n0), e1 = r.rows(n1), nr = e1 - e0, c0 = n0 - e0 * r.h;
        if (nr > 0) {      // [carried | chunk] at a 16-byte boundary of the staging buffer, one MFCC span; its tail is the new carry
            s->starts[(size_t)n_spans] = pos;
            s->lengths[(size_t)n_spans] = c0 + len;
            ++n_spans;
            dsp::add_copy_runs(s->runs[0], st * s->carry_stride, pos * es, c0 * es, 0);
            dsp::add_copy_runs(s->runs[0], chunk_offsets[st] * es, (pos + c0) * es, len * es, 1);
            dsp::add_copy_runs(s->runs[1], (pos + nr * r.h) * es, st * s->carry_stride, (n1 - e1 * r.h) * es, 0);
            pos += round_up(c0 + len, align);
        } else if (len > 0) {      // no row yet: the chunk goes behind what is carried
            dsp::add_copy_runs(s->runs[1], chunk_offsets[st] * es, st * s->carry_stride + c0 * es, len * es, 1);
        }
        if (!s->scans || nr == 0) continue;
        const long w0 = r.windows(e0), w1 = r.windows(e1), k0 = e0 - w0 * r.hf;
        if (w1 > w0) {      // [carried rows | new rows] is one recording of the scans; the rows from window w1's start on are the new carry
            const long base = fo[n_scan], k1 = e1 - w1 * r.hf;
            dsp::add_copy_runs(s->runs[2], st * s->row_stride, base * rb, k0 * rb, 0);
            dsp::add_copy_runs(s->runs[2], ro[st] * rb, (base + k0) * rb, nr * rb, 1);
            dsp::add_copy_runs(s->runs[3], (base + k0 + nr - k1) * rb, st * s->row_stride, k1 * rb, 0);
            fo[++n_scan] = base + k0 + nr;
            scan_win += k0 + nr >= r.wf ? 1 + (k0 + nr - r.wf) / r.hf : 1;      // what the scans' own planner gives these rows (scan_plan)
        } else {            // no window: a stream with fewer rows than a window must not reach the scans (they would give it a short one)
            dsp::add_copy_runs(s->runs[3], ro[st] * rb, st * s->row_stride + k0 * rb, nr * rb, 1);
        }
    }
    if (scan_win != total_win) return capi_fail(DSP_EINVAL, "internal: the scans would write other windows than the push announced");
    size_t n_runs = 0;
    for (const auto &v : s->runs) n_runs += v.size();
    if (n_runs > 0) {
        DSP_ON_DEVICE(s->plan->device);
        hipStream_t st = (hipStream_t)stream;
        if (s->d_stage.reserve((size_t)(pos * es) + 64) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (stream staging)");
        if (!d_mfcc && s->d_new.reserve((size_t)(total_rows * rb) + 16) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (new rows)");
        if (s->d_scanmat.reserve((size_t)(fo[n_scan] * rb) + 16) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (scan matrix)");
        float *rows_out = d_mfcc ? d_mfcc : reinterpret_cast<float *>(s->d_new.get());
        dsp::SpanRing::Lease slot;
        DSP_CAPI_HIP(s->ring.acquire(n_runs * sizeof(CopyRun), slot));
        const CopyRun *d_run[4];
        {
            CopyRun *h = static_cast<CopyRun *>(slot.h());
            const CopyRun *d = static_cast<const CopyRun *>(slot.d());
            size_t at = 0;
            for (int k = 0; k < 4; ++k) {
                if (!s->runs[k].empty()) std::memcpy(h + at, s->runs[k].data(), s->runs[k].size() * sizeof(CopyRun));
                d_run[k] = d + at;
                at += s->runs[k].size();
            }
        }
        DSP_CAPI_HIP(slot.upload(n_runs * sizeof(CopyRun), st));
        if (const int rc = resample()) return rc;
        // ---- the launches: from here on a failure breaks the session
        const int g = es == 2 ? 2 : 4;
        DSP_STREAM_HIP(dsp::launch_stream_copy(d_run[0], (long)s->runs[0].size(), s->d_carry, d_chunks, s->d_stage, g, st));
        if (n_spans > 0) {
            // the ragged MFCC path (no frame cap) over spans of the staging buffer: span c = sample frames [starts[c], starts[c] + lengths[c])
            // (refused before anything of its own is enqueued where a kernel was switched since the session was created)
            const int rc = dsp::mfcc_clips_ragged(s->plan, s->d_stage, s->in_kind, n_spans, s->starts.data(), INT_MAX, rows_out, stream, s->lengths.data());
            if (rc < 0) { s->broken = true; return rc; }
        }
        DSP_STREAM_HIP(dsp::launch_stream_copy(d_run[1], (long)s->runs[1].size(), s->d_stage, d_chunks, s->d_carry, g, st));
        if (n_scan > 0) {
            DSP_STREAM_HIP(dsp::launch_stream_copy(d_run[2], (long)s->runs[2].size(), s->d_rowcarry, rows_out, s->d_scanmat, 4, st));
            const float *mat = reinterpret_cast<const float *>(s->d_scanmat.get());
            int rc = s->stop ? dsp_stop_scan_device(s->stop, mat, n_scan, fo, &s->scfg, d_prob, stream) : DSP_OK;
            if (rc >= 0 && s->spk) rc = dsp_speaker_scan_device(s->spk, mat, n_scan, fo, &s->scfg, d_llr_mean, d_labels, stream);
            if (rc < 0) { s->broken = true; return rc; }
        }
        DSP_STREAM_HIP(dsp::launch_stream_copy(d_run[3], (long)s->runs[3].size(), s->d_scanmat, rows_out, s->d_rowcarry, 4, st));
    } else if (const int rc = resample()) {
        return rc;
    }
    // ---- commit
    s->pushed = true;
    for (long st = 0; st < n; ++st) s->received[(size_t)st] += chunk_offsets[st + 1] - chunk_offsets[st];
    if (row_offsets) std::memcpy(row_offsets, ro, (size_t)(n + 1) * sizeof(long));
    if (window_offsets) std::memcpy(window_offsets, wo, (size_t)(n + 1) * sizeof(long));
    return DSP_OK;
}

int dsp_stream_session_attach_resampler(dsp_stream_session *s, dsp_stream_resampler *rs)
{
    if (!s) return capi_fail(DSP_EINVAL, "session is NULL");
    if (!rs) return capi_fail(DSP_EINVAL, "resampler is NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    if (s->pushed) return capi_fail(DSP_EINVAL, "a resampler is attached before the session's first push");
    if (s->rs) return capi_fail(DSP_EINVAL, "the session has a resampler already");
    if (s->in_kind != 0) return capi_fail(DSP_EINVAL, "a resampler writes float mono samples: create the session with pcm16 = 0 (the resampler decodes the int16)");
    const dsp::StreamResamplerInfo info = dsp::stream_resampler_info(rs);
    if (info.n_streams != s->n_streams)
        return capi_fail(DSP_EINVAL, "the resampler has " + std::to_string(info.n_streams) + " streams, the session " + std::to_string(s->n_streams));
    if (info.device != s->device) return capi_fail(DSP_EINVAL, "the resampler and the session's plan live on different devices");
    if (info.rate_out != s->plan->cfg.sample_rate)
        return capi_fail(DSP_EINVAL, "the resampler writes " + std::to_string(info.rate_out) + " Hz, the session's plan runs at " + std::to_string(s->plan->cfg.sample_rate));
    s->roo.assign((size_t)s->n_streams + 1, 0);
    s->rs = rs;
    return DSP_OK;
}

}  // extern "C"
