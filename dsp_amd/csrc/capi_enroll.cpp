// capi_enroll.cpp -- the C ABI of sliding CMVN and of MAP speaker enrolment (include/dsp_amd.h dsp_cmvn_*, dsp_speaker_enroll*; DESIGN.md
// 3.11): argument checks, the spans of a ragged batch through the handle's ring, the enroller's grow-only workspace (the UBM: a GmmModel of
// gmm_model.hpp), and the launches of enroll_kernels.hip.
#include <cmath>
#include <cstdint>
#include <memory>

#include "capi_util.hpp"
#include "enroll_kernels.hpp"

using dsp::capi_fail;

struct dsp_cmvn : dsp::Handle {
    int d = 0, window = 0;
    dsp::SpanRing spans;
};

struct dsp_speaker_enroller : dsp::Handle {
    int k = 0, d = 0;
    dsp::DeviceBuf<float> model;         // log_consts[k], means[k][d], inv_covs[k][d], rounded once to float32
    dsp::DeviceBuf<float> partials;      // grow-only: [chunks of a call][k (d + 1) + 1]
    dsp::SpanRing spans;
};

namespace {

// spans of a ragged batch into a leased slot: unit0 = prefix sums of ceil(rows / unit_rows).  Returns the unit total, or < 0 (EINVAL: the
// offsets; EHIP: the ring).  refuse_rowless: DSP_EINVAL naming the first entry without rows (otherwise such entries own no unit).
long fill_spans(dsp::SpanRing &ring, dsp::SpanRing::Lease &slot, const long *fo, long n, int unit_rows, const char *what, bool refuse_rowless)
{
    if (const int rc = dsp::check_frame_offsets(fo, n, what)) return rc;
    if (refuse_rowless)
        if (const int rc = dsp::refuse_rowless(fo, n, " has no rows", what)) return rc;
    if (const int rc = dsp::lease(ring, (size_t)n * sizeof(dsp::RowSpan), slot)) return rc;
    dsp::RowSpan *h = static_cast<dsp::RowSpan *>(slot.h());
    long units = 0;
    for (long r = 0; r < n; ++r) {
        const long rows = fo[r + 1] - fo[r];
        h[r] = dsp::RowSpan{fo[r], units, rows};
        units += (rows + unit_rows - 1) / unit_rows;
    }
    return units;
}

}  // namespace

extern "C" {

int dsp_cmvn_create(int device, int d, int window, dsp_cmvn **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (d < 1 || d > dsp::kGmmMaxD) return capi_fail(DSP_EINVAL, "d must be 1 .. 16");
    if (window < 2 || window > dsp::kCmvnMaxWindow)
        return capi_fail(DSP_EINVAL, "window must be 2 .. " + std::to_string(dsp::kCmvnMaxWindow) + " rows (what one block's LDS image holds), got " + std::to_string(window));
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_cmvn &c) -> int {
        c.d = d;
        c.window = window;
        DSP_CAPI_HIP(dsp::prepare_cmvn());
        return DSP_OK;
    });
}

void dsp_cmvn_destroy(dsp_cmvn *c) { dsp::destroy(c); }

int dsp_cmvn_ragged_device(dsp_cmvn *c, const float *d_in, long n_recordings, const long *frame_offsets, float *d_out, void *stream)
{
    if (!c || n_recordings < 0) return capi_fail(DSP_EINVAL, "bad argument (cmvn NULL or n_recordings < 0)");
    if (n_recordings == 0) return DSP_OK;
    if (!frame_offsets || !d_in || !d_out) return capi_fail(DSP_EINVAL, "frame_offsets, d_in and d_out must not be NULL");
    if (d_in == d_out) return capi_fail(DSP_EINVAL, "d_out must not alias d_in: a row's window reads its neighbours' inputs");
    DSP_ON_DEVICE(c->device);
    dsp::SpanRing::Lease slot;
    const long tiles = fill_spans(c->spans, slot, frame_offsets, n_recordings, dsp::kCmvnTileRows, "recording", false);
    if (tiles <= 0) return (int)tiles;
    DSP_CAPI_HIP(slot.upload((size_t)n_recordings * sizeof(dsp::RowSpan), (hipStream_t)stream));
    DSP_CAPI_HIP(dsp::launch_cmvn(d_in, static_cast<const dsp::RowSpan *>(slot.d()), n_recordings, tiles, c->d, c->window, d_out, (hipStream_t)stream));
    return DSP_OK;
}

int dsp_speaker_enroller_create(const dsp_gmm_float_params *ubm, int device, dsp_speaker_enroller **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (const int rc = dsp::check_gmm_float_params(ubm, "ubm", "ubm: ")) return rc;
    std::vector<float> host;
    if (const int rc = dsp::pack_ubm(ubm, host)) return rc;
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_speaker_enroller &e) {
        e.k = ubm->k;
        e.d = ubm->d;
        return dsp::upload_ubm(host, e.model, "hipMemcpy(e->model, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice)");
    });
}

void dsp_speaker_enroller_destroy(dsp_speaker_enroller *e) { dsp::destroy(e); }

int dsp_speaker_enroll_ragged_device(dsp_speaker_enroller *e, const float *d_feats, long n_speakers, const long *frame_offsets,
                                     const dsp_enroll_config *cfg, float *d_means, int8_t *d_means_q6, float *d_counts, float *d_ll_mean,
                                     int *d_saturated, void *stream)
{
    if (!e || n_speakers < 0) return capi_fail(DSP_EINVAL, "bad argument (enroller NULL or n_speakers < 0)");
    if (n_speakers == 0) return DSP_OK;
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_enroll_config is NULL");
    float param;
    if (cfg->map_mode == DSP_MAP_RELEVANCE) {
        param = cfg->relevance_factor;
        if (!(param > 0.0f) || !std::isfinite(param)) return capi_fail(DSP_EINVAL, "dsp_enroll_config: relevance_factor must be > 0 and finite");
    } else if (cfg->map_mode == DSP_MAP_FIXED_ALPHA) {
        param = cfg->fixed_alpha;
        if (!(param >= 0.0f && param <= 1.0f)) return capi_fail(DSP_EINVAL, "dsp_enroll_config: fixed_alpha must lie in [0, 1]");
    } else
        return capi_fail(DSP_EINVAL, "dsp_enroll_config: map_mode must be DSP_MAP_RELEVANCE or DSP_MAP_FIXED_ALPHA");
    if (!d_means && !d_means_q6 && !d_counts && !d_ll_mean && !d_saturated) return capi_fail(DSP_EINVAL, "every output is NULL");
    if (n_speakers > (1L << 30)) return capi_fail(DSP_EINVAL, "at most 2^30 speakers per call");
    if (!frame_offsets || !d_feats) return capi_fail(DSP_EINVAL, "frame_offsets and d_feats must not be NULL");
    DSP_ON_DEVICE(e->device);
    dsp::SpanRing::Lease slot;
    const long chunks = fill_spans(e->spans, slot, frame_offsets, n_speakers, dsp::kEnrollChunkRows, "speaker", true);
    if (chunks < 0) return (int)chunks;
    if (e->partials.reserve((size_t)chunks * dsp::enroll_partial_floats(e->k, e->d) * sizeof(float)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the enroller's workspace");
    DSP_CAPI_HIP(slot.upload((size_t)n_speakers * sizeof(dsp::RowSpan), (hipStream_t)stream));
    DSP_CAPI_HIP(dsp::launch_enroll(d_feats, static_cast<const dsp::RowSpan *>(slot.d()), n_speakers, chunks, dsp::GmmModel{e->model, e->k, e->d}, e->partials,
                                    cfg->map_mode == DSP_MAP_FIXED_ALPHA, param, d_means, d_means_q6, d_counts, d_ll_mean, d_saturated, (hipStream_t)stream));
    return DSP_OK;
}

}  // extern "C"
