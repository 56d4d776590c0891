// capi_segments.cpp -- the C ABI of segments from window scores (include/dsp_amd.h dsp_segment*): argument checks, all
// of them before a device is touched, the host-only capacity bound and sample spans, the segmenter's grow-only workspace and the
// per-recording offsets (windows, words, chunks) that travel through its ring to the kernels of segment_kernels.hip.
#include <cmath>

#include "capi_util.hpp"
#include "mfcc_plan.hpp"
#include "segment_kernels.hpp"

using dsp::capi_fail;

struct dsp_segmenter : dsp::StageHandle {};      // ws: SegWorkspace (segment_kernels.hpp); spans: window | word | chunk | block offsets

namespace {

int check_config(const dsp_segment_config *cfg)
{
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_segment_config is NULL");
    if (std::isnan(cfg->on) || std::isnan(cfg->off)) return capi_fail(DSP_EINVAL, "dsp_segment_config: on and off must not be NaN");
    if (cfg->off > cfg->on) return capi_fail(DSP_EINVAL, "dsp_segment_config: off must be <= on");
    if (cfg->min_windows < 1) return capi_fail(DSP_EINVAL, "dsp_segment_config: min_windows must be >= 1");
    if (cfg->max_gap < 0) return capi_fail(DSP_EINVAL, "dsp_segment_config: max_gap must be >= 0");
    if (cfg->mode != DSP_SEG_INDEPENDENT && cfg->mode != DSP_SEG_EXCLUSIVE)
        return capi_fail(DSP_EINVAL, "dsp_segment_config: mode must be DSP_SEG_INDEPENDENT or DSP_SEG_EXCLUSIVE");
    return DSP_OK;
}

int check_window_offsets(const long *wo, long n)
{
    if (wo[0] < 0) return capi_fail(DSP_EINVAL, "window_offsets must be non-negative");
    for (long r = 0; r < n; ++r) {
        if (wo[r + 1] < wo[r]) return capi_fail(DSP_EINVAL, "window_offsets decrease at recording " + std::to_string(r));
        if (wo[r + 1] - wo[r] > INT32_MAX) return capi_fail(DSP_EINVAL, "recording " + std::to_string(r) + " has 2^31 windows or more");
    }
    return DSP_OK;
}

int check_columns(long n_columns)
{
    if (n_columns < 1 || n_columns > dsp::kSegMaxColumns) return capi_fail(DSP_EINVAL, "n_columns must be 1 .. 2^19");
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_segmenter_create(int device, dsp_segmenter **out) { return dsp::create_on_host(device, out); }

void dsp_segmenter_destroy(dsp_segmenter *s) { dsp::destroy(s); }

long dsp_segments_capacity(const dsp_segment_config *cfg, const long *window_offsets, long n_recordings, long n_columns)
{
    if (const int rc = check_config(cfg)) return rc;
    if (n_recordings < 0) return capi_fail(DSP_EINVAL, "n_recordings < 0");
    if (const int rc = check_columns(n_columns)) return rc;
    if (n_recordings == 0) return 0;
    if (!window_offsets) return capi_fail(DSP_EINVAL, "window_offsets is NULL");
    if (const int rc = check_window_offsets(window_offsets, n_recordings)) return rc;
    const long m = cfg->min_windows, g = cfg->max_gap;
    long per_column = 0;
    for (long r = 0; r < n_recordings; ++r) per_column += (window_offsets[r + 1] - window_offsets[r] + g + 1) / (m + g + 1);
    if (per_column > LONG_MAX / n_columns) return capi_fail(DSP_EINVAL, "the capacity does not fit a long");
    return per_column * n_columns;
}

int dsp_segments_device(dsp_segmenter *s, const float *d_scores, long n_recordings, const long *window_offsets, long n_columns, const dsp_segment_config *cfg,
                        dsp_segment *d_segments, long max_segments, int *d_track_counts, long *d_total, void *stream)
{
    if (!s) return capi_fail(DSP_EINVAL, "segmenter is NULL");
    if (const int rc = check_config(cfg)) return rc;
    if (n_recordings < 0) return capi_fail(DSP_EINVAL, "n_recordings < 0");
    if (const int rc = check_columns(n_columns)) return rc;
    if (d_segments && max_segments < 0) return capi_fail(DSP_EINVAL, "max_segments < 0");
    if (n_recordings == 0) return DSP_OK;
    if (!d_scores) return capi_fail(DSP_EINVAL, "d_scores is NULL");
    if (!window_offsets) return capi_fail(DSP_EINVAL, "window_offsets is NULL");
    if (!d_total) return capi_fail(DSP_EINVAL, "d_total is NULL");
    if (const int rc = check_window_offsets(window_offsets, n_recordings)) return rc;
    if (n_recordings > dsp::kSegMaxTracks / n_columns) return capi_fail(DSP_EINVAL, "at most 2^31 tracks (recordings times columns) per call");
    // the totals, and what they refuse, before a device is touched
    long windows = 0, words = 0, chunks = 0, blocks = 0;
    for (long r = 0; r < n_recordings; ++r) {
        const long W = window_offsets[r + 1] - window_offsets[r];
        windows += W;
        words += dsp::seg_words(W);
        chunks += dsp::seg_chunks(W);
        blocks += dsp::seg_blocks(W);
    }
    if (windows >= (1L << 32)) return capi_fail(DSP_EINVAL, "2^32 windows or more in one call");
    // (a chunk of a column is one wavefront of a grid of blocks of 4: 2^33 of them at most)
    if ((double)words * (double)n_columns > 9e15 || (double)chunks * (double)n_columns >= 8589934592.0)
        return capi_fail(DSP_EINVAL, "2^45 windows times columns, or more, in one call");
    const bool exclusive = cfg->mode == DSP_SEG_EXCLUSIVE;
    if (const int rc = dsp::check_device(s->device)) return rc;
    DSP_ON_DEVICE(s->device);
    hipStream_t st = (hipStream_t)stream;
    // wo (from 0) | word offsets | chunk offsets | block offsets, n + 1 longs each
    const size_t n1 = (size_t)n_recordings + 1, bytes = 4 * n1 * sizeof(long);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(s->spans, bytes, slot)) return rc;
    long *wo = static_cast<long *>(slot.h()), *wdo = wo + n1, *co = wdo + n1, *bo = co + n1;
    wo[0] = wdo[0] = co[0] = bo[0] = 0;
    for (long r = 0; r < n_recordings; ++r) {
        const long W = window_offsets[r + 1] - window_offsets[r];
        wo[r + 1] = wo[r] + W;
        wdo[r + 1] = wdo[r] + dsp::seg_words(W);
        co[r + 1] = co[r] + dsp::seg_chunks(W);
        bo[r + 1] = bo[r] + dsp::seg_blocks(W);
    }
    if (s->ws.reserve(dsp::seg_workspace_bytes(words * n_columns, chunks * n_columns, blocks * n_columns, windows, exclusive)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the segmenter's workspace");
    const dsp::SegWorkspace ws = dsp::seg_carve(s->ws.get(), words * n_columns, chunks * n_columns, blocks * n_columns, windows, exclusive);
    DSP_CAPI_HIP(slot.upload(bytes, st));
    dsp::SegCall call{d_scores + (size_t)window_offsets[0] * (size_t)n_columns, static_cast<const long *>(slot.d()), n_recordings, n_columns, windows, words, chunks,
                      blocks, cfg->on, cfg->off, cfg->min_windows, cfg->max_gap, exclusive, d_segments, d_segments ? max_segments : 0, d_track_counts, d_total};
    DSP_CAPI_HIP(dsp::launch_segments(call, ws, st));
    return DSP_OK;
}

long dsp_segment_sample_spans(const dsp_mfcc_config *mfcc, const dsp_scan_config *scan, const long *offsets, long n_recordings, const dsp_segment *segments,
                              long n_segments, long *starts, long *lengths)
{
    if (!mfcc) return capi_fail(DSP_EINVAL, "mfcc config is NULL");
    std::string why;
    if (!dsp::valid_cfg(*mfcc, why)) return capi_fail(DSP_EINVAL, why);
    if (const int rc = dsp::scan_args(scan, n_recordings)) return rc;
    if (n_segments < 0) return capi_fail(DSP_EINVAL, "n_segments < 0");
    if (n_segments == 0) return 0;
    if (!offsets || !segments) return capi_fail(DSP_EINVAL, "offsets and segments must not be NULL");
    const long wf = scan->window_frames, hf = scan->hop_frames, hop = mfcc->hop_length, half = mfcc->frame_length / 2;
    for (long i = 0; i < n_segments; ++i) {
        const dsp_segment &g = segments[i];
        if (g.recording < 0 || g.recording >= n_recordings) return capi_fail(DSP_EINVAL, "segment " + std::to_string(i) + ": no such recording");
        const long len = dsp::ragged_clip_length(offsets, g.recording);
        if (len < 0) return len;
        const long rows = dsp_mfcc_frames_for(mfcc, (int)len, INT_MAX);
        const long windows = rows >= wf ? 1 + (rows - wf) / hf : 1;
        if (g.first_window < 0 || g.n_windows < 1 || (long)g.first_window + g.n_windows > windows)
            return capi_fail(DSP_EINVAL, "segment " + std::to_string(i) + " lies outside the windows of its recording");
        const long first = g.first_window, last = first + g.n_windows - 1;
        long a, b;      // [a, b) within the recording
        if (mfcc->framing == DSP_FRAMING_CENTER) {
            const long last_row = last * hf + std::max<long>(std::min(wf, rows), 1) - 1;
            a = std::max<long>(0, first * hf * hop - half);
            b = std::min(len, last_row * hop + half);
        } else {
            const long span = mfcc->framing == DSP_FRAMING_STREAM ? wf * hop : mfcc->frame_length + (wf - 1) * hop;
            a = first * hf * hop;
            b = last * hf * hop + std::min(span, len - last * hf * hop);
        }
        if (starts) starts[i] = offsets[g.recording] + a;
        if (lengths) lengths[i] = b - a;
    }
    return n_segments;
}

}  // extern "C"
